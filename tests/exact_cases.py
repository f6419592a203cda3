"""Builders, integer references and bit checkers for the exact-arithmetic contract of the
projection kernels (tests/test_exact_cases.py on the CPU, tests/test_exact_gemm_gpu.py on the GPU).

A tolerance on Gaussian inputs cannot see one dropped (row, column, k) product, a residual add
rounded twice, a wrong rounding mode, a wrong arg-max tie rule or a wrong RoPE partner in the
upper frequencies. The inputs built here make the correct output ONE bit pattern:

* ``exact_int``: A is +-1, W is {-1, 0, +1}; every partial sum is an integer far below 2^24, so
  it is exact in fp32 in whatever order a kernel adds, and the builder asserts that every final
  value (with the residual and the bias) is at most 256 in magnitude, i.e. a bf16 value. (With
  fp8 weights and a per-row power-of-two scale s the same holds for result / s.)
* ``round_once``: A in [-4, 4], W in [-3, 3], dense. Partial sums stay below K * 12 < 2^24; the
  results are large enough that a share of them are exact round-to-nearest-even ties, and with a
  residual that rounding y first differs from rounding resid + y once. Both shares are asserted.

References are float64 products of small integers (exact), converted once. Everything is plain
torch, seeded by an explicit CPU generator, and runs on any device.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Optional

import torch

import contract_cases as C
from llm_sharding_amd.ops import packing

BF16_INT_MAX = 256       # every integer of magnitude <= 256 is a bf16 value
FP32_INT_MAX = 1 << 24
RESID_MAX = 64           # residual and bias integers lie in [-64, 64]
MIN_SHARE = 0.01         # round_once: least share of ties / of double-rounding differences
FP8_SCALES = (0.5, 1.0, 2.0, 4.0)
ROPE_PAIRS = ((1., 0.), (0., 1.), (-1., 0.), (0., -1.), (.5, .5), (.5, -.5), (-.5, .5), (-.5, -.5))
GATE_LO, GATE_HI, GATE_BLOCK = 24, 128, 64
PAD_BIAS = -3.0e38       # the engine's bias on padded lm_head rows


def gen(seed: int) -> torch.Generator:
    """Always a CPU generator: every random operand is drawn on the CPU and then moved, so a case
    holds the same integers on every device and the builders' conditions, checked without a GPU,
    hold on the GPU as well (all later arithmetic is exact)."""
    return torch.Generator(device="cpu").manual_seed(seed)


# ------------------------------------------------------------------------------ operands
def randint(lo: int, hi: int, shape, g, device) -> torch.Tensor:
    """int64 integers in [lo, hi], both ends included."""
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).to(device)


def signs(shape, g, device) -> torch.Tensor:
    return randint(0, 1, shape, g, device) * 2 - 1


def density_for(K: int) -> float:
    return min(1.0, 1024.0 / K)


def ternary(N: int, K: int, g, device, density: Optional[float] = None) -> torch.Tensor:
    """int64 [N, K] in {-1, 0, +1} with a non-zero share of ``density`` (default 1024 / K)."""
    d = density_for(K) if density is None else density
    keep = (torch.rand(N, K, generator=g) < d).to(device)
    return signs((N, K), g, device) * keep


def assert_all_k_used(w: torch.Tensor, what: str) -> None:
    unused = (w != 0).sum(0) == 0
    assert not bool(unused.any()), f"{what}: {int(unused.sum())} k column(s) of W are all zero"


def bf16_rne(x: torch.Tensor) -> torch.Tensor:
    """float64 -> bf16, rounded to nearest even once (the values are exact in fp32)."""
    assert float(x.abs().max()) < FP32_INT_MAX
    f = x.float()
    assert bool((f.double() == x).all()), "reference value is not an fp32 value"
    return f.to(torch.bfloat16)


def is_bf16(x: torch.Tensor) -> torch.Tensor:
    return x.float().to(torch.bfloat16).double() == x


def is_tie(x: torch.Tensor) -> torch.Tensor:
    """Exactly half way between two bf16 values (x exact in fp32)."""
    return (x.float().view(torch.int32) & 0xFFFF) == 0x8000


def bf16_trunc(x: torch.Tensor) -> torch.Tensor:
    """The faulty conversion: fp32 -> bf16 by dropping the low 16 bits."""
    b = x.float().view(torch.int32) & -65536
    return (b >> 16).to(torch.int16).view(torch.bfloat16)


def bf16_half_up(x: torch.Tensor) -> torch.Tensor:
    """The faulty conversion: round to nearest, ties away from zero (add 0x8000, truncate)."""
    b = (x.float().view(torch.int32) + 0x8000) & -65536
    return (b >> 16).to(torch.int16).view(torch.bfloat16)


def fp8_bytes(w: torch.Tensor) -> torch.Tensor:
    """OCP e4m3 encoding (uint8) of small integers, which the format holds exactly."""
    q = w.float().to(packing.FP8)
    assert bool((q.float() == w.float()).all())
    return q.view(torch.uint8)


def fp8_scales(N: int, g, device, choices=FP8_SCALES) -> torch.Tensor:
    c = torch.tensor(choices, dtype=torch.float32, device=device)
    return c[randint(0, len(choices) - 1, (N,), g, device)]


def matmul(a: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """float64 a @ w^T: exact for these operands (every partial sum is far below 2^53)."""
    return a.double() @ w.double().T


class Weight:
    """One weight in the forms the families take. ``ref`` float64 [N, K] in the kernel's (fused)
    row order is exactly what the kernel multiplies by; ``wp`` = pack_b bf16; ``wq`` / ``sc`` =
    packed e4m3 bytes and the fp32 per-row scale."""

    def __init__(self, w: torch.Tensor, scale: Optional[torch.Tensor] = None):
        if scale is None:
            self.ref, self.wq, self.sc = w.double(), None, None
            self.wp = packing.pack_b(w.to(torch.bfloat16))
            assert bool((self.wp.double() == packing.pack_b(self.ref)).all())
        else:
            self.ref = w.double() * scale.double()[:, None]
            self.wq, self.sc, self.wp = packing.pack_b_fp8(fp8_bytes(w)).view(-1), scale.float().contiguous(), None


# ------------------------------------------------------------------------------ checkers
_INT_VIEW = {torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(_INT_VIEW[t.dtype]) if t.dtype in _INT_VIEW else t


def assert_bits_equal(out: torch.Tensor, expected: torch.Tensor, what: str = "",
                      unit: Optional[torch.Tensor] = None, limit: int = 6) -> None:
    """``out`` and ``expected`` (same shape and dtype, bf16 / fp32 / int) are bit-identical.
    The message gives the count and the first positions with the kernel's and the expected value;
    ``unit`` (per column, or a scalar tensor: the value of one product, 1 for integer weights and
    the row scale for fp8) adds the difference in products, so one dropped product reads -1/+1
    and a K step of 32 / 64 as a multiple of it."""
    assert out.shape == expected.shape and out.dtype == expected.dtype, (what, out.shape, expected.shape, out.dtype)
    bad = _bits(out.contiguous()) != _bits(expected.contiguous().to(out.device))
    if not bool(bad.any()):
        return
    pos = bad.nonzero()[:limit].tolist()
    lines = []
    for p in pos:
        got, exp = float(out[tuple(p)]), float(expected[tuple(p)])
        s = f"{tuple(p)}: kernel {got!r} expected {exp!r}"
        if unit is not None:
            u = float(unit.reshape(-1)[p[-1]] if unit.numel() > 1 else unit)
            s += f" (difference {(got - exp) / u:+g} products)"
        lines.append(s)
    n = int(bad.sum())
    raise AssertionError(f"{what}: {n} of {bad.numel()} element(s) differ bitwise ({n / bad.numel():.2%}); " + "; ".join(lines))


def assert_within_one_ulp(out: torch.Tensor, expected: torch.Tensor, what: str = "") -> float:
    """bf16 ``out`` is ``expected`` or one of its two bf16 neighbours; returns the share of
    elements that differ."""
    a, b = C.bits(out.contiguous()).int(), C.bits(expected.contiguous().to(out.device)).int()
    d = (a - b).abs()  # for one sign the int16 patterns of bf16 are ordered by magnitude
    same_sign = ((a ^ b) & 0x8000) == 0
    zero = (a & 0x7FFF) + (b & 0x7FFF) <= 1
    bad = (~same_sign & ~zero) | (same_sign & (d > 1))
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} element(s) more than one bf16 ulp from the reference, first at " \
                                f"{bad.nonzero()[:5].tolist()}"
    return float((d != 0).float().mean())


# ------------------------------------------------------------------------------ linear
def build_linear(M: int, N: int, K: int, seed: int, device="cpu", mode: str = "exact_int", fp8: bool = False):
    """A [M, K], W [N, K], an integer residual and bias, and the expected bf16 output of every
    store / residual epilogue form: ``exp["store"]``, ``["store_bias"]``, ``["resid"]``,
    ``["resid_bias"]``. ``unit`` [N]: the value of one product in column n."""
    assert mode in ("exact_int", "round_once")
    g = gen(seed)
    if mode == "exact_int":
        a, w = signs((M, K), g, device), ternary(N, K, g, device)
    else:
        a, w = randint(-4, 4, (M, K), g, device), randint(-3, 3, (N, K), g, device)
        assert K * 12 < FP32_INT_MAX
    assert_all_k_used(w, f"linear {M}x{N}x{K}")
    scale = fp8_scales(N, g, device) if fp8 else None
    unit = scale.double() if fp8 else torch.ones(N, dtype=torch.float64, device=device)
    W = Weight(w, scale)
    y = matmul(a, W.ref)
    # residual and bias: integers in [-64, 64] times the column's unit, so the sums stay on its grid
    resid = (randint(-RESID_MAX, RESID_MAX, (M, N), g, device).double() * unit).to(torch.bfloat16)
    bias = (randint(-RESID_MAX, RESID_MAX, (N,), g, device).double() * unit).float()
    assert bool(is_bf16(resid.double()).all())
    forms = {"store": y, "store_bias": y + bias.double(), "resid": resid.double() + y,
             "resid_bias": resid.double() + y + bias.double()}
    tag = f"linear {mode} {M}x{N}x{K} fp8={fp8}"
    stats = {}
    if mode == "exact_int":
        for k, v in forms.items():
            worst = float((v / unit).abs().max())
            assert worst <= BF16_INT_MAX, f"{tag} {k}: max |result| {worst} > {BF16_INT_MAX}: lower the density"
            assert bool(is_bf16(v).all()), f"{tag} {k}: a result is not a bf16 value"
            stats["max_" + k] = worst
    else:
        stats["tie_share"] = float(is_tie(y).float().mean())
        assert stats["tie_share"] >= MIN_SHARE, f"{tag}: only {stats['tie_share']:.3%} of the outputs are RNE ties"
        twice = bf16_rne(bf16_rne(y).double() + resid.double())
        stats["double_rounding_share"] = float((C.bits(twice) != C.bits(bf16_rne(forms["resid"]))).float().mean())
        assert stats["double_rounding_share"] >= MIN_SHARE, \
            f"{tag}: rounding y first changes only {stats['double_rounding_share']:.3%} of the residual outputs"
    exp = {k: bf16_rne(v) for k, v in forms.items()}
    return SimpleNamespace(M=M, N=N, K=K, mode=mode, fp8=fp8, a=a.to(torch.bfloat16), w=w, W=W, y=y, resid=resid,
                           bias=bias, exp=exp, unit=unit, stats=stats, tag=tag)


def expected_ss(out_bf16: torch.Tensor) -> torch.Tensor:
    """fp32 [M, N / 64]: the per-64-column sums of squares of integer outputs, exact (< 2^24)."""
    M, N = out_bf16.shape
    ss = out_bf16.double().pow(2).view(M, N // 64, 64).sum(-1)
    assert float(ss.max()) < FP32_INT_MAX and bool((ss == ss.round()).all())
    return ss.float()


def norm_expected(y: torch.Tensor, eps: float) -> torch.Tensor:
    """The fused-RMSNorm reference for +-1 activations (mean(x^2) is exactly 1, unit norm weight):
    bf16_rne(float32(y) * float32(1 / sqrt(1 + eps)))."""
    r = torch.tensor(1.0 / (1.0 + eps) ** 0.5, dtype=torch.float32, device=y.device)
    return (y.float() * r).to(torch.bfloat16)


# ------------------------------------------------------------------------------ SwiGLU
def gate_density(K: int) -> float:
    """A quarter of the up density, lowered (never the check loosened) until the gate's random part
    has at most 48 non-zero terms per row: a +-40 window around the 64 of the final block is then
    5.8 standard deviations wide."""
    return min(density_for(K) / 4.0, 48.0 / max(K - GATE_BLOCK, 1))


def build_swiglu(M: int, I: int, K: int, seed: int, device="cpu", fp8: bool = False):
    """Saturated-gate SwiGLU: the final 64-wide K block has A = +1 and every gate weight +1, so
    every gate pre-activation is 64 + (a small integer) in [24, 128]: exp(-g) < 2^-24,
    1 + exp(-g) is exactly 1, silu(g) is exactly g and the output is bf16_rne(g * u)."""
    assert K > GATE_BLOCK
    g = gen(seed)
    a = signs((M, K), g, device)
    a[:, K - GATE_BLOCK:] = 1
    wu = ternary(I, K, g, device)
    wg = ternary(I, K, g, device, density=gate_density(K))
    wg[:, K - GATE_BLOCK:] = 1
    fused = packing.fuse_gate_up(wg, wu)
    assert_all_k_used(fused, f"swiglu {M}x{I}x{K}")
    scale = None
    if fp8:  # the gate rows keep scale 1 (their window is fixed), the up rows any power of two
        scale = packing.fuse_gate_up(torch.ones(I, 1, device=device), fp8_scales(I, g, device)[:, None])[:, 0]
    W = Weight(fused, scale)
    gu = matmul(a, W.ref).view(M, I // 16, 2, 16)
    gate, up = gu[:, :, 0].reshape(M, I), gu[:, :, 1].reshape(M, I)
    tag = f"swiglu {M}x{I}x{K} fp8={fp8}"
    lo, hi = float(gate.min()), float(gate.max())
    assert GATE_LO <= lo and hi <= GATE_HI, f"{tag}: gate pre-activations span [{lo}, {hi}], outside [{GATE_LO}, {GATE_HI}]"
    assert float((gate * up).abs().max()) < FP32_INT_MAX
    return SimpleNamespace(M=M, I=I, N=2 * I, K=K, fp8=fp8, a=a.to(torch.bfloat16), W=W, gate=gate, up=up,
                           exp=bf16_rne(gate * up), tag=tag, stats={"gate_min": lo, "gate_max": hi})


# ------------------------------------------------------------------------------ QKV
def rope_tables(t_max: int, hd: int, g, device):
    """Synthetic cos / sin [t_max, hd / 2] fp32 drawn from ROPE_PAIRS: every product with an
    integer and every sum of two is exact, with or without FMA contraction."""
    pairs = torch.tensor(ROPE_PAIRS, dtype=torch.float32, device=device)
    pick = pairs[randint(0, len(ROPE_PAIRS) - 1, (t_max, hd // 2), g, device)]
    return pick[..., 0].contiguous(), pick[..., 1].contiguous()


def rotate_half_split(z: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """z [M, heads, hd] float64; cos / sin [M, hd / 2]: (z1 c - z2 s | z2 c + z1 s)."""
    half = z.shape[-1] // 2
    c, s = cos.double()[:, None, :], sin.double()[:, None, :]
    z1, z2 = z[..., :half], z[..., half:]
    return torch.cat([z1 * c - z2 * s, z2 * c + z1 * s], -1)


def build_qkv(M: int, nh: int, nkv: int, hd: int, K: int, seed: int, device="cpu", rope: bool = True, slots: int = 2):
    """Integer q / k / v projections. ``rope``: fused with packing.fuse_qkv, a synthetic table,
    no bias; else the natural [q | k | v] order (GPT-2 layout) with an integer bias. Positions
    are a permutation prefix (no two rows share one) that includes 0 and t_max - 1."""
    g = gen(seed)
    N = (nh + 2 * nkv) * hd
    t_max = max(M, 2) + 5
    a = signs((M, K), g, device)
    wq, wk, wv = (ternary(n * hd, K, g, device) for n in (nh, nkv, nkv))
    nat = torch.cat([wq, wk, wv])
    assert_all_k_used(nat, f"qkv {M}x{N}x{K}")
    fused = packing.fuse_qkv(wq, wk, wv, nh, nkv, hd) if rope else nat
    W = Weight(fused)
    others = 1 + torch.randperm(t_max - 2, generator=g).to(device)[:max(M - 2, 0)]
    pos = torch.cat([torch.tensor([0, t_max - 1], device=device), others])[:M]   # 0 and t_max - 1 first
    pos = pos[torch.randperm(M, generator=g).to(device)]
    assert pos.unique().numel() == M and (M < 2 or {0, t_max - 1} <= set(pos.tolist()))
    slot = randint(0, slots - 1, (M,), g, device)
    z = matmul(a, nat)
    bias = None
    if not rope:
        bias = randint(-RESID_MAX, RESID_MAX, (N,), g, device).float()
        z = z + bias.double()
    tag = f"qkv {M} rows nh {nh} nkv {nkv} hd {hd} K {K} rope={rope}"
    assert float(z.abs().max()) <= BF16_INT_MAX, f"{tag}: max |projection| {float(z.abs().max())} > {BF16_INT_MAX}"
    zq, zk, zv = z[:, :nh * hd].view(M, nh, hd), z[:, nh * hd:(nh + nkv) * hd].view(M, nkv, hd), z[:, (nh + nkv) * hd:].view(M, nkv, hd)
    cos = sin = None
    if rope:
        cos, sin = rope_tables(t_max, hd, g, device)
        zq, zk = rotate_half_split(zq, cos[pos], sin[pos]), rotate_half_split(zk, cos[pos], sin[pos])
    return SimpleNamespace(M=M, N=N, K=K, nh=nh, nkv=nkv, hd=hd, t_max=t_max, slots=slots, rope=rope, a=a.to(torch.bfloat16),
                           W=W, fused=fused, z=z, bias=bias, cos=cos, sin=sin, pos=pos.to(torch.int32), slot=slot.to(torch.int32),
                           exp_q=bf16_rne(zq.reshape(M, nh * hd)), exp_k=bf16_rne(zk), exp_v=bf16_rne(zv), tag=tag)


def qkv_epilogue_model(case, zp: torch.Tensor, partner_xor: int = 8, sin_flip_from: Optional[int] = None):
    """What csrc/kernels/epilogue.h::epi_qkv_store computes from the GEMM's fp32 result ``zp``
    [M, N] in the kernel's column order, in torch: (q [M, nh * hd], k [M, nkv, hd], v [M, nkv, hd])
    bf16. ``partner_xor`` / ``sin_flip_from``: the faulty variants (partner at n ^ 4; sin negated
    for frequency indices >= sin_flip_from)."""
    M, nh, nkv, hd = case.M, case.nh, case.nkv, case.hd
    qs, ks = nh * hd, nkv * hd
    zp = zp.double()
    if not case.rope:
        q, k, v = zp[:, :qs], zp[:, qs:qs + ks], zp[:, qs + ks:]
        return bf16_rne(q), bf16_rne(k.reshape(M, nkv, hd)), bf16_rne(v.reshape(M, nkv, hd))
    n = torch.arange(qs + ks, device=zp.device)
    c = torch.where(n < qs, n, n - qs) % hd
    tt, cc = c // 16, c % 16
    fi = 8 * tt + (cc % 8)
    dim = torch.where(cc < 8, fi, hd // 2 + fi)
    head = torch.where(n < qs, n, n - qs) // hd
    p = case.pos.long()
    cs, sn = case.cos[p][:, fi].double(), case.sin[p][:, fi].double()       # [M, qs + ks]
    if sin_flip_from is not None:
        sn = torch.where((fi >= sin_flip_from)[None, :], -sn, sn)
    v_, vp = zp[:, :qs + ks], zp[:, (n ^ partner_xor)]
    r = torch.where((cc < 8)[None, :], v_ * cs - vp * sn, v_ * cs + vp * sn)
    dst = head * hd + dim
    q = torch.zeros(M, qs, dtype=torch.float64, device=zp.device)
    k = torch.zeros(M, ks, dtype=torch.float64, device=zp.device)
    q[:, dst[:qs]] = r[:, :qs]
    k[:, dst[qs:]] = r[:, qs:]
    return bf16_rne(q), bf16_rne(k.view(M, nkv, hd)), bf16_rne(zp[:, qs + ks:].reshape(M, nkv, hd))


def check_qkv(case, q: torch.Tensor, kflat, kc, vflat, vc, what: str = "") -> None:
    """q and the addressed cache cells bitwise; every other cache cell still the initial pattern."""
    sl, pl = case.slot.long(), case.pos.long()
    assert_bits_equal(q, case.exp_q, what + " q")
    assert_bits_equal(kc[sl, :, pl], case.exp_k, what + " k_cache")
    assert_bits_equal(vc[sl, :, pl], case.exp_v, what + " v_cache")
    C.assert_cache_footprint(kflat, kc, sl, pl, what=what + " k_cache")
    C.assert_cache_footprint(vflat, vc, sl, pl, what=what + " v_cache")


# ------------------------------------------------------------------------------ arg-max ties
def planted_columns(V: int, M: int) -> list:
    """Per row the 3 to 5 columns that share the row maximum, chosen from the kernels' geometry
    (16-column tiles; a wave / workgroup / ragged deal owns runs of tiles):
      row 0: column 0, another column of tile 0 and the last column (a column-0 tie, one tile,
             the first and the last column);
      row 1: the first tile again without column 0, and two columns of the last tile;
      the others by turns two columns of one tile, two columns of adjacent tiles, the two columns
      on either side of a tile edge - each with one to three more columns a third / half / two
      thirds of the vocabulary away (other waves, workgroups and deals).
    No column belongs to two rows."""
    T = V // 16
    npairs = (T - 4) // 2
    assert V % 16 == 0 and npairs >= 8 and M - 2 <= 2 * npairs, (V, M)
    near = {(0, 0): (2, 9), (0, 1): (3, 10), (1, 0): (12, 17), (1, 1): (13, 18), (2, 0): (15, 16), (2, 1): (14, 19)}
    f3_off = (4, 5, 6, 7, 8, 11)
    out = []
    for m in range(M):
        if m == 0:
            cols = [0, 7, V - 1]
        elif m == 1:
            cols = [5, V - 16, V - 2]
        else:
            i = m - 2
            j, s, kind = i % npairs, i // npairs, i % 3
            ks = kind * 2 + s
            base = lambda jj: 32 + 32 * (jj % npairs)
            cols = [base(j) + o for o in near[(kind, s)]]
            cols.append(base(j + npairs // 3) + 20 + ks)
            extra = (i // 3) % 3  # 3, 4 or 5 planted columns, independent of the kind
            if extra >= 1:
                cols.append(base(j + npairs // 2) + 26 + ks)
            if extra >= 2:
                cols.append(base(j + 2 * npairs // 3) + f3_off[ks])
        out.append(sorted(cols))
    flat = [c for cols in out for c in cols]
    assert len(set(flat)) == len(flat) and min(flat) >= 0 and max(flat) < V, "planted columns collide"
    assert all(3 <= len(c) <= 5 for c in out)
    return out


def build_argmax(M: int, V: int, K: int, seed: int, device="cpu", fp8: bool = False, negative: bool = False):
    """Integer lm_head with exact ties at the row maximum. Every planted column of row m holds a
    copy of one W row, ``A[m] * mask`` (``mask`` keeps min(K, 512) k's), so its logit is the number
    of kept k's, strictly above every other column; the smallest planted column is the token.
    ``negative``: an integer bias below every logit, so every row's logits are all negative.
    fp8: the planted rows carry the largest scale, so their logits stay on top."""
    g = gen(seed)
    a = signs((M, K), g, device)
    w = ternary(V, K, g, device)
    D = min(K, 512)
    mask = torch.zeros(K, dtype=torch.int64, device=device)
    mask[torch.randperm(K, generator=g).to(device)[:D]] = 1
    cols = planted_columns(V, M)
    scale = fp8_scales(V, g, device) if fp8 else None
    for m, cs in enumerate(cols):
        w[cs] = a[m] * mask
        if fp8:
            scale[cs] = max(FP8_SCALES)
    assert_all_k_used(w, f"argmax {M}x{V}x{K}")
    W = Weight(w, scale)
    logits = matmul(a, W.ref)
    bias = None
    if negative:
        bias = torch.full((V,), -float(1 << 14), dtype=torch.float32, device=device)
        logits = logits + bias.double()
        assert float(logits.max()) < 0
    assert float(logits.abs().max()) < FP32_INT_MAX
    top = logits.max(-1).values
    tag = f"argmax {M}x{V}x{K} fp8={fp8} negative={negative}"
    assert bool((top != 0).all()), f"{tag}: a planted maximum is zero (+0 / -0 key order would decide)"
    tied = logits == top[:, None]
    for m, cs in enumerate(cols):
        assert tied[m].nonzero()[:, 0].tolist() == cs, f"{tag}: row {m} ties at {tied[m].nonzero()[:, 0].tolist()}, planted {cs}"
    expected = torch.tensor([c[0] for c in cols], dtype=torch.int32, device=device)
    return SimpleNamespace(M=M, V=V, N=V, K=K, fp8=fp8, a=a.to(torch.bfloat16), w=w, scale=scale, W=W, logits=logits,
                           bias=bias, cols=cols, expected=expected, tag=tag,
                           largest=torch.tensor([c[-1] for c in cols], dtype=torch.int32, device=device))


def build_padded_head(M: int, V: int, V_pad: int, K: int, seed: int, device="cpu"):
    """The engine's padded lm_head: rows V .. V_pad - 1 are copies of row 0 behind a -3e38 bias,
    and token 0 holds every row's maximum, so each padded row ties with it before the bias."""
    assert V_pad > V and V_pad % 16 == 0
    g = gen(seed)
    D = min(K, 512)
    mask = torch.zeros(K, dtype=torch.int64, device=device)
    mask[torch.randperm(K, generator=g).to(device)[:D]] = 1
    a = signs((M, K), g, device)
    a = torch.where(mask.bool()[None, :], a[0:1], a)
    w = ternary(V_pad, K, g, device)
    w[0] = a[0] * mask
    w[V:] = w[0]
    bias = torch.zeros(V_pad, dtype=torch.float32, device=device)
    bias[V:] = PAD_BIAS
    raw = matmul(a, w)
    assert bool((raw[:, V:] == raw[:, 0:1]).all()) and bool((raw[:, 1:V].max(-1).values < raw[:, 0]).all())
    assert bool((raw[:, 0] != 0).all())
    return SimpleNamespace(M=M, V=V, N=V_pad, K=K, a=a.to(torch.bfloat16), W=Weight(w), bias=bias,
                           expected=torch.zeros(M, dtype=torch.int32, device=device), tag=f"padded head {M}x{V}+{V_pad - V}x{K}")


def assert_tokens(tok: torch.Tensor, case, what: str = "", offset: int = 0) -> None:
    exp = case.expected.to(tok.device) + offset
    bad = tok != exp
    if bool(bad.any()):
        m = int(bad.nonzero()[0])
        cols = getattr(case, "cols", None)
        raise AssertionError(f"{what}: {int(bad.sum())} row(s) took the wrong token; row {m}: kernel {int(tok[m])}, expected "
                             f"{int(exp[m])}" + (f" (tied columns {[c + offset for c in cols[m]]})" if cols else ""))


# ------------------------------------------------------------------------------ the GPU file's shapes
# A case is named by a key, (kind, rows, ...): tests/test_exact_gemm_gpu.py asks for cases by key
# only, and case() refuses a key that gpu_keys() does not list. tests/test_exact_cases.py builds
# every listed key on the CPU and so checks the builders' conditions (the bound of 256, every k
# used, the tie and double-rounding shares, the gate window) without a GPU.
QKV_GEOMS = {64: (8, 2, 64), 128: (4, 1, 128)}   # head_dim -> (n_heads, n_kv, head_dim): N = 768 for both
N_LIN, I_SWIGLU, V_ARGMAX, V_RAGGED, N_RAGGED = 768, 384, 4096, 32000, 4800
N_PARTIAL = 2048                                  # lsa_resid_rmsnorm_partials is built for H = 2048 n
N_EDGE, I_EDGE = 640, 320                         # 640 = 3 x 192 + 64: gemm_sk's bn = 192 ends in a partial column tile
V_COOP = 3072                                     # 192 tiles: every cooperative config (3 and 6 waves too) divides them
GEMV_ROWS = {1: (1, 7, 16), 2: (29,), 4: (50,)}   # by packing.row_blocks
COOP_ROWS = {2: 17, 4: 50, 8: 128}
GEMM_ROWS = {"gemm": (17, 150, 333), "gemm_sk": (129, 300, 777), "gemm_wr": (193, 300, 512)}
K_DECODE, K_GEMM, K_WR = (768, 1216, 11008), (256, 1216), (256, 320, 1216)
K_COOP = (768, 1216, 1024)                        # 1024: four 256-deep chunks for the kf = 8, kw = 2 configs
K_COOP_EPI = (768, 1024)                          # QKV and arg-max of the cooperative configs
K_EPI = 768                                       # QKV, arg-max and every fp8 case of the decode families
K_ROUND_MIN = 768                                 # below it too few results leave the bf16 integers


def _seed(key) -> int:
    import zlib
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


_BUILDERS = {
    "linear": lambda k, s, d: build_linear(k[1], k[2], k[3], s, d),
    "round_once": lambda k, s, d: build_linear(k[1], k[2], k[3], s, d, mode="round_once"),
    "linear_fp8": lambda k, s, d: build_linear(k[1], k[2], k[3], s, d, fp8=True),
    "round_once_fp8": lambda k, s, d: build_linear(k[1], k[2], k[3], s, d, mode="round_once", fp8=True),
    "swiglu": lambda k, s, d: build_swiglu(k[1], k[2], k[3], s, d),
    "swiglu_fp8": lambda k, s, d: build_swiglu(k[1], k[2], k[3], s, d, fp8=True),
    "qkv": lambda k, s, d: build_qkv(k[1], *QKV_GEOMS[k[2]], k[3], s, d, rope=k[4]),
    "argmax": lambda k, s, d: build_argmax(k[1], k[2], k[3], s, d),
    "argmax_neg": lambda k, s, d: build_argmax(k[1], k[2], k[3], s, d, negative=True),
    "argmax_fp8": lambda k, s, d: build_argmax(k[1], k[2], k[3], s, d, fp8=True),
    "padded_head": lambda k, s, d: build_padded_head(k[1], 1000, 1024, 256, s, d),
}


def gpu_keys() -> list:
    keys = []
    decode_rows = sorted({m for ms in GEMV_ROWS.values() for m in ms} | set(COOP_ROWS.values()))
    for M in decode_rows:
        for K in K_DECODE:
            keys += [("linear", M, N_LIN, K), ("round_once", M, N_LIN, K), ("swiglu", M, I_SWIGLU, K)]
        if M in COOP_ROWS.values():
            keys += [("linear", M, N_LIN, 1024), ("round_once", M, N_LIN, 1024), ("swiglu", M, I_SWIGLU, 1024)]
        for K in (K_COOP_EPI if M in COOP_ROWS.values() else (K_EPI,)):
            keys += [("qkv", M, 64, K, True), ("qkv", M, 128, K, True), ("qkv", M, 64, K, False)]
            if M in COOP_ROWS.values():
                keys += [("argmax", M, V_COOP, K), ("argmax_neg", M, V_COOP, K)]
        keys += [("argmax", M, V_ARGMAX, K_EPI), ("argmax_neg", M, V_ARGMAX, K_EPI)]
        K = K_EPI
        keys += [("argmax_fp8", M, V_ARGMAX, K)]
        keys += [("linear_fp8", M, N_LIN, K), ("round_once_fp8", M, N_LIN, K), ("swiglu_fp8", M, I_SWIGLU, K)]
    keys += [("argmax", 50, V_RAGGED, 256), ("linear", 50, N_RAGGED, 256)]
    for M in tuple(COOP_ROWS.values()) + GEMM_ROWS["gemm_sk"]:
        keys.append(("linear", M, N_PARTIAL, 512))
    for fam, rows in GEMM_ROWS.items():
        for M in rows:
            for K in (K_WR if fam == "gemm_wr" else K_GEMM):
                keys += [("linear", M, N_LIN, K), ("swiglu", M, I_SWIGLU, K)]
                if K >= K_ROUND_MIN:
                    keys.append(("round_once", M, N_LIN, K))
                else:
                    keys += [("qkv", M, 64, K, True), ("qkv", M, 128, K, True), ("qkv", M, 64, K, False)]
    for M in GEMM_ROWS["gemm_sk"]:
        for K in K_GEMM:
            keys += [("linear", M, N_EDGE, K), ("swiglu", M, I_EDGE, K)]
        keys.append(("round_once", M, N_EDGE, 1216))
    keys += [("padded_head", 1), ("padded_head", 7)]
    out = []
    for k in keys:
        if k not in out:
            out.append(k)
    return out


GPU_KEYS = gpu_keys()
_CACHE = {}


def case(key, device="cpu"):
    """The case named ``key``, built once per device and shared (treat it as read-only)."""
    assert key in GPU_KEYS, f"{key} is not listed in exact_cases.gpu_keys(): its conditions are not checked on the CPU"
    ck = (key, str(device))
    if ck not in _CACHE:
        _CACHE[ck] = _BUILDERS[key[0]](key, _seed(key), device)
    return _CACHE[ck]
