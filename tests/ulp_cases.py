"""Builders, float64 references and the half-ulp checker for the activation functions of the GEMM
epilogues and for the stand-alone normalisation kernels (tests/test_ulp_cases.py on the CPU,
tests/test_ulp_kernels_gpu.py on the GPU).

An aggregate ``rel_err`` of 5e-3 to 1e-2 cannot see a cancellation in an activation's tail, a
missing eps, a wrong 1 / H, a weight multiplied after the rounding, a row polluted by its
neighbour or a one-pass variance. Here every output element is compared with the float64 value
of the same operation: it must be the correctly rounded bf16 value up to a slack that is derived
from the fp32 operations a correct kernel performs, never from a measurement:

* activations, ``SLACK_ACT`` = 2^-7 ulp. The largest fp32 term is the rounding of the
  exponential's argument, |a| 2^-24 relative with |a| <= 88 before exp leaves the fp32 range;
  one ulp each of the hardware exp, the add, the divide and one multiply bring the total to about
  5.5e-6 relative = 1.4e-3 bf16 ulp. 2^-7 leaves a factor of 5.
* RMSNorm / LayerNorm, ``SLACK_NORM`` = 2^-6 ulp. A lane adds at most 256 squares in sequence at
  H = 8192, then 8 tree levels: at most 272 x 2^-24 relative on the sum; the square root halves
  it; rsqrtf and two multiplies bring the total to about 1e-5 relative = 2.6e-3 ulp. 2^-6 leaves
  a factor of 6. LayerNorm's final ``+ b`` can cancel, so its slack is taken relative to the
  largest magnitude that enters the element (``scale`` of assert_half_ulp).

The activation sees exactly known inputs: the weight is an identity (or one-hot rows), so the
GEMM result is the A element itself in every summation order, and A sweeps all 65536 bf16
patterns (bf16 denormals, NaN and Inf replaced by 0, where the output must be +-0). Everything
is drawn on the CPU from seeded generators, as in exact_cases.py.
"""
from __future__ import annotations

import functools
import math
from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch

import exact_cases as X
from llm_sharding_amd.ops import packing

SLACK_ACT = 2.0 ** -7
SLACK_NORM = 2.0 ** -6
TINY, TINY_BOUND = 2.0 ** -120, 2.0 ** -119   # flush-to-zero near the fp32 floor is not part of the contract
BF16_ROUNDS_TO_INF = (2.0 - 2.0 ** -8) * 2.0 ** 127  # half an ulp above the largest bf16 value
K_ACT = 4096
R_GELU, R_SWIGLU = 16, 17                      # rows that hold the 65536 patterns
SWIGLU_COLS = 4064                             # pattern columns of a SwiGLU row; columns 4064.. hold 1
UP_VALUES = (1.0, 3.0, -0.5, 0.15625)          # exact in bf16 and in e4m3
M_GEMM = 144
N_FINITE, N_NORMAL_OR_ZERO = 65280, 65280 - 2 * 127
GELU_C, GELU_K = math.sqrt(2.0 / math.pi), 0.044715


# ------------------------------------------------------------------------------ checker
def ulp_bf16(v: torch.Tensor) -> torch.Tensor:
    """2^(floor(log2 |v|) - 7), float64 (2^-8 for v = 0: such elements are not held to an ulp)."""
    _, e = torch.frexp(v.double().abs())  # |v| = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(v, dtype=torch.float64), e - 8)


def assert_half_ulp(out_bf16: torch.Tensor, exact_f64: torch.Tensor, slack: float, what: str,
                    scale: Optional[torch.Tensor] = None, inp: Optional[torch.Tensor] = None,
                    zero: Optional[torch.Tensor] = None) -> float:
    """Per element |out - exact| <= 0.5 ulp_bf16(exact) + slack ulp_bf16(scale or exact); elements
    with |exact| < 2^-120 are held to |out - exact| <= 2^-119 instead, and where ``zero`` (bool:
    the input was replaced by 0) the output must be +-0. No element is left out; a NaN fails, and
    so does an infinity that the exact value is not within reach of. Returns the worst excess over
    half an ulp, in ulps of ``scale or exact``."""
    assert out_bf16.dtype == torch.bfloat16 and out_bf16.shape == exact_f64.shape, (what, out_bf16.shape, exact_f64.shape)
    raw = out_bf16.detach().cpu().double()
    exact = exact_f64.detach().cpu().double()
    assert bool(torch.isfinite(exact).all()), what + ": the reference is not finite"
    # the top of the range (SwiGLU: 3 x gate): an exact value at or beyond BF16_ROUNDS_TO_INF rounds
    # to +-inf, which is then the one correct output; below it an infinite output counts as the
    # next grid point 2^128, so the same bound decides whether it was within reach
    over = exact.abs() >= BF16_ROUNDS_TO_INF
    out = torch.where(torch.isinf(raw), torch.copysign(torch.full_like(raw, 2.0 ** 128), raw), raw)
    err = (out - exact).abs()
    u_exact = ulp_bf16(exact)
    u_scale = u_exact if scale is None else ulp_bf16(scale.detach().cpu().double().expand_as(exact))
    tiny = exact.abs() < TINY
    bound = torch.where(tiny, torch.full_like(exact, TINY_BOUND), 0.5 * u_exact + slack * u_scale)
    bad = torch.where(over, raw != torch.copysign(torch.full_like(raw, float("inf")), exact), ~(err <= bound))  # (NaN fails)
    if zero is not None:
        z = zero.detach().cpu().expand_as(exact)
        bad |= z & (out != 0)
    # (elements judged by another rule count as -1/2, the least an excess can be)
    excess = torch.where(tiny | over, torch.full_like(err, -0.5), (err - 0.5 * u_exact) / u_scale)
    excess = torch.nan_to_num(excess, nan=float("inf"))
    worst = float(excess.max()) if excess.numel() else 0.0
    if bool(bad.any()):
        n = int(bad.sum())
        order = torch.where(bad, excess, torch.full_like(excess, -float("inf"))).reshape(-1).argsort(descending=True)[:6]
        lines = []
        for f in order.tolist():
            if not bool(bad.reshape(-1)[f]):
                continue
            p = tuple(int(i) for i in np.unravel_index(f, tuple(exact.shape)))
            s = f"{p}: "
            if inp is not None:
                s += f"input {float(inp.detach().cpu().double().expand_as(exact)[p])!r} "
            s += f"kernel {float(raw[p])!r} exact {float(exact[p])!r} ({float(err[p] / u_exact[p]):.4g} ulp away)"
            lines.append(s)
        raise AssertionError(f"{what}: {n} of {bad.numel()} element(s) outside 1/2 ulp + {slack:g} ulp, worst excess "
                             f"{worst:.4g} ulp; " + "; ".join(lines))
    return worst


# ------------------------------------------------------------------------------ bf16 patterns
def all_patterns() -> torch.Tensor:
    """int16 [65536]: every bf16 bit pattern once."""
    return (torch.arange(65536, dtype=torch.int32) - 32768).to(torch.int16)


def is_finite_pattern(p: torch.Tensor) -> torch.Tensor:
    return ((p.int() >> 7) & 0xFF) != 0xFF


def usable(p: torch.Tensor) -> torch.Tensor:
    """Neither NaN / Inf nor a bf16 denormal (MFMA units may flush those)."""
    e, m = (p.int() >> 7) & 0xFF, p.int() & 0x7F
    return (e != 0xFF) & ~((e == 0) & (m != 0))


def operand_of(p: torch.Tensor) -> torch.Tensor:
    """bf16 of the patterns with denormals, NaN and Inf replaced by +0."""
    return torch.where(usable(p), p, torch.zeros_like(p)).view(torch.bfloat16)


def repeat_rows(t: torch.Tensor, M: int) -> torch.Tensor:
    """[R, ...] -> [M, ...]: the rows repeated, every further copy rotated by one more row."""
    R = t.shape[0]
    m = torch.arange(M, device=t.device)
    return t[(m + m // R) % R]


# ------------------------------------------------------------------------------ references
def gelu64(x: torch.Tensor) -> torch.Tensor:
    x = x.double()
    u = GELU_C * (x + GELU_K * x * x * x)
    return x / (1.0 + torch.exp(-2.0 * u))


def silu64(g: torch.Tensor) -> torch.Tensor:
    g = g.double()
    return g / (1.0 + torch.exp(-g))


def rms_exact(x: torch.Tensor, w: Optional[torch.Tensor], eps: float) -> torch.Tensor:
    """float64 x rsqrt(mean(x^2) + eps) w with eps taken as the float32 value."""
    xd = x.double()
    r = torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + float(np.float32(eps)))
    return xd * r * (1.0 if w is None else w.double())


def layernorm_exact(x: torch.Tensor, g: torch.Tensor, b: torch.Tensor, eps: float):
    """(exact, scale): float64 (x - mu) / sigma g + b and |t| (1 + |mu| / sigma) + |b|."""
    xd = x.double()
    mu = xd.mean(-1, keepdim=True)
    sigma = torch.sqrt((xd - mu).pow(2).mean(-1, keepdim=True) + float(np.float32(eps)))
    t = (xd - mu) / sigma * g.double()
    return t + b.double(), t.abs() * (1.0 + mu.abs() / sigma) + b.double().abs()


# ------------------------------------------------------------------------------ float32 emulations
# What a correct (or a deliberately faulty) kernel computes, in float32 on the CPU: every
# operation rounds to float32 (torch CPU ops do not contract), the norms add strictly in sequence
# (numpy's cumsum: the worst order). tests/test_ulp_cases.py shows with them that the float64
# references stay inside the slacks and that the checker rejects each fault.
def _u32(x: torch.Tensor) -> torch.Tensor:
    c, k = torch.tensor(GELU_C, dtype=torch.float32), torch.tensor(GELU_K, dtype=torch.float32)
    return c * (x + k * x * x * x)


def gelu_f32(x: torch.Tensor) -> torch.Tensor:
    x = x.float()
    return x / (1.0 + torch.exp(-2.0 * _u32(x)))


def gelu_f32_cancelling(x: torch.Tensor) -> torch.Tensor:
    """0.5 x (2 - 2 / (exp(2u) + 1)): for negative x a difference of two numbers near 2."""
    x = x.float()
    return 0.5 * x * (2.0 - 2.0 / (torch.exp(2.0 * _u32(x)) + 1.0))


def silu_f32(g: torch.Tensor) -> torch.Tensor:
    g = g.float()
    return g / (1.0 + torch.exp(-g))


def _seq_sum(a: np.ndarray) -> np.ndarray:
    return np.cumsum(a.astype(np.float32), axis=1, dtype=np.float32)[:, -1]


def rms_f32(x: torch.Tensor, w: Optional[torch.Tensor], eps: float, fault: Optional[str] = None) -> torch.Tensor:
    """bf16 RMSNorm in float32. ``fault``: "no_eps", "h_plus_8", "weight_after" (the weight
    multiplies the rounded value) or "next_row" (row r takes row r + 1's sum of squares)."""
    xf = x.float().numpy()
    H = np.float32(xf.shape[1] + (8 if fault == "h_plus_8" else 0))
    ss = _seq_sum(xf * xf)
    if fault == "next_row":
        ss = np.roll(ss, -1)
    with np.errstate(divide="ignore", invalid="ignore"):
        rs = np.float32(1.0) / np.sqrt(ss / H + np.float32(0.0 if fault == "no_eps" else eps), dtype=np.float32)
        y = torch.from_numpy(xf * rs[:, None])
    wf = None if w is None else w.float()
    if fault == "weight_after":
        return (y.to(torch.bfloat16).float() * (1.0 if wf is None else wf)).to(torch.bfloat16)
    return (y if wf is None else y * wf).to(torch.bfloat16)


def layernorm_f32(x: torch.Tensor, g: torch.Tensor, b: torch.Tensor, eps: float, one_pass: bool = False) -> torch.Tensor:
    xf = x.float().numpy()
    H = np.float32(xf.shape[1])
    mu = (_seq_sum(xf) / H)[:, None]
    if one_pass:
        var = _seq_sum(xf * xf) / H - (mu * mu)[:, 0]
    else:
        var = _seq_sum((xf - mu) * (xf - mu)) / H
    rs = (np.float32(1.0) / np.sqrt(var + np.float32(eps), dtype=np.float32))[:, None]
    return torch.from_numpy((xf - mu) * rs * g.float().numpy() + b.float().numpy()).to(torch.bfloat16)


# ------------------------------------------------------------------------------ activation operands
class Weight:
    """A weight of small exact values in the forms the families take (scale 1 for fp8)."""

    def __init__(self, w: torch.Tensor, device):
        wb = w.to(torch.bfloat16)
        assert bool((wb.float() == w.float()).all())
        self.wp = packing.pack_b(wb).contiguous().to(device)
        self.wq = packing.pack_b_fp8(X.fp8_bytes(w)).view(-1).to(device)
        self.sc = torch.ones(w.shape[0], dtype=torch.float32, device=device)


def identity_rows() -> torch.Tensor:
    return torch.eye(K_ACT, dtype=torch.float32)


def swiglu_rows() -> torch.Tensor:
    """fp32 [2 x 4096, 4096] in the fused gate / up layout: gate n = one-hot of column n mod 4064,
    up n = u_n times the one-hot of column 4064."""
    n = torch.arange(K_ACT)
    wg = torch.zeros(K_ACT, K_ACT)
    wg[n, n % SWIGLU_COLS] = 1.0
    wu = torch.zeros(K_ACT, K_ACT)
    wu[n, SWIGLU_COLS] = up_values()
    return packing.fuse_gate_up(wg, wu)


def up_values() -> torch.Tensor:
    return torch.tensor(UP_VALUES, dtype=torch.float32)[torch.arange(K_ACT) % len(UP_VALUES)]


@functools.lru_cache(maxsize=None)
def weight(kind: str, device: str) -> Weight:
    return Weight(identity_rows() if kind == "store" else swiglu_rows(), device)


@functools.lru_cache(maxsize=None)
def gelu_grid():
    """A [16, 4096] = all 65536 bf16 patterns; W = identity, so y = A exactly."""
    p = all_patterns().view(R_GELU, K_ACT)
    a = operand_of(p)
    return SimpleNamespace(patterns=p, a=a, zero=a == 0, exact=gelu64(a), inp=a.double(), tag="gelu bf16 grid")


@functools.lru_cache(maxsize=None)
def gelu_bias(seed: int):
    """A = 0 and bias[n] = the input: 2048 values with magnitudes log-spaced over 2^-20 .. 2^7,
    random 23-bit mantissas and signs, and 2048 uniform in [-10, -2], shuffled."""
    g = X.gen(seed)
    h = K_ACT // 2
    e = torch.floor(torch.linspace(-20.0, 7.0, h)).to(torch.int32) + 127
    mant = torch.randint(0, 1 << 23, (h,), generator=g, dtype=torch.int32)
    sign = torch.randint(0, 2, (h,), generator=g, dtype=torch.int32)
    logs = ((sign << 31) | (e << 23) | mant).view(torch.float32)
    assert float(logs.abs().min()) >= 2.0 ** -20 and float(logs.abs().max()) < 2.0 ** 8
    tail = (-10.0 + 8.0 * torch.rand(h, generator=g, dtype=torch.float64)).float()
    bias = torch.cat([logs, tail])[torch.randperm(K_ACT, generator=g)].contiguous()
    a = torch.zeros(R_GELU, K_ACT, dtype=torch.bfloat16)
    v = (torch.zeros(K_ACT, dtype=torch.float32) + bias)  # the float32 sum y + bias
    return SimpleNamespace(a=a, bias=bias, exact=gelu64(v)[None, :].expand(R_GELU, K_ACT).contiguous(),
                           inp=v.double()[None, :], tag=f"gelu fp32 bias sweep seed {seed}")


BIAS_SEEDS = (20241, 20242)


@functools.lru_cache(maxsize=None)
def swiglu_grid():
    """A [17, 4096]: the patterns in columns 0 .. 4063 (4064 per row, wrapping), 1 beyond.
    out[m, n] = silu(A[m, n mod 4064]) u_n, rounded once."""
    idx = torch.arange(R_SWIGLU * SWIGLU_COLS) % 65536
    p = torch.zeros(R_SWIGLU, K_ACT, dtype=torch.int16)
    p[:, :SWIGLU_COLS] = all_patterns()[idx].view(R_SWIGLU, SWIGLU_COLS)
    a = operand_of(p)
    a[:, SWIGLU_COLS:] = 1.0
    n = torch.arange(K_ACT)
    gate = a[:, n % SWIGLU_COLS]
    u = up_values()
    return SimpleNamespace(patterns=p[:, :SWIGLU_COLS], a=a, gate=gate, up=u, zero=gate == 0,
                           exact=silu64(gate) * u.double()[None, :], inp=gate.double(), tag="swiglu bf16 grid")


# ------------------------------------------------------------------------------ norm cases
RMS_GENERIC, RMS_REG = (768, 3072), (2048, 4096, 6144, 8192)
RMS_EPS = (1e-5, 1e-6)
RMS_SCALES = (2.0 ** -9, 2.0 ** -4, 1.0, 2.0 ** 5)
LN_WIDTHS = (768, 1024, 1600)
LN_EPS = 1e-5
PARTIAL_CASES = tuple((H, S) for H in (2048, 8192) for S in (1, 4))


@functools.lru_cache(maxsize=None)
def rms_case(H: int):
    """Six rows, each with its own scale (2^-9: the mean square is below eps, so eps matters to
    first order), one row with a single non-zero element and one all-zero row; w = 1 + 0.1 randn."""
    g = X.gen(1000 + H)
    x = torch.zeros(len(RMS_SCALES) + 2, H, dtype=torch.float32)
    for r, s in enumerate(RMS_SCALES):
        x[r] = torch.randn(H, generator=g) * s
    x[len(RMS_SCALES), H // 3] = 3.0
    w = (1.0 + 0.1 * torch.randn(H, generator=g)).to(torch.bfloat16)
    xb = x.to(torch.bfloat16)
    assert float(xb[0].double().pow(2).mean()) < max(RMS_EPS)
    return SimpleNamespace(H=H, rows=x.shape[0], x=xb, w=w, zero_row=x.shape[0] - 1)


@functools.lru_cache(maxsize=None)
def partial_case(H: int, S: int):
    """Integer residual and partials (as exact_cases: h is known bitwise), one magnitude per row,
    the last row all zero."""
    g = X.gen(2000 + H + S)
    mags = (1, 3, 12, 40, 0)
    rows = len(mags)
    resid = torch.stack([torch.randint(-m, m + 1, (H,), generator=g) for m in mags])
    P = torch.stack([torch.stack([torch.randint(-m, m + 1, (H,), generator=g) for m in mags]) for _ in range(S)])
    hsum = resid + P.sum(0)
    assert int(hsum.abs().max()) <= X.BF16_INT_MAX
    w = (1.0 + 0.1 * torch.randn(H, generator=g)).to(torch.bfloat16)
    return SimpleNamespace(H=H, S=S, rows=rows, resid=resid.to(torch.bfloat16), P=P.float().contiguous(),
                           h=X.bf16_rne(hsum.double()), w=w, zero_row=rows - 1)


@functools.lru_cache(maxsize=None)
def layernorm_case(H: int, with_pos: bool):
    """Rows of several scales, a large-mean row (mean 8, std 0.25, on the bf16 grid) and a constant
    row x = 2 (variance 0, exact sum: the output is the bias bitwise). With the position add the
    two special rows take the all-zero table row 0. ``x`` is the kernel's input, ``xr`` the row
    after the add (bf16(x + pe[pos]): what the kernel writes back and normalises)."""
    g = X.gen(3000 + H + int(with_pos))
    scales = (2.0 ** -4, 1.0, 2.0 ** 5)
    rows = len(scales) + 2
    x = torch.zeros(rows, H)
    for r, s in enumerate(scales):
        x[r] = torch.randn(H, generator=g) * s + 0.25 * s
    big, const = len(scales), len(scales) + 1
    x[big] = 8.0 + 0.25 * torch.randn(H, generator=g)
    x[const] = 2.0
    x = x.to(torch.bfloat16)
    gw = (1.0 + 0.2 * torch.randn(H, generator=g)).to(torch.bfloat16)
    b = (0.2 * torch.randn(H, generator=g)).to(torch.bfloat16)
    pe = pos = None
    xr = x
    if with_pos:
        pe = (0.3 * torch.randn(16, H, generator=g)).to(torch.bfloat16)
        pe[0] = 0
        pos = torch.randint(1, 16, (rows + 8,), generator=g, dtype=torch.int32)
        pos[big] = pos[const] = 0
        xr = (x.float() + pe[pos[:rows].long()].float()).to(torch.bfloat16)
    assert bool((xr[const] == 2).all()) and abs(float(xr[big].double().mean()) - 8.0) < 0.05
    return SimpleNamespace(H=H, rows=rows, x=x, xr=xr, g=gw, b=b, pe=pe, pos=pos, big=big, const=const)
