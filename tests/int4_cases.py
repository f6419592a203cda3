"""Builders and integer references for the exact-arithmetic contract of the int4 (W4A16) decode
kernel, in the style of tests/exact_cases.py (tests/test_int4.py on the CPU, tests/test_int4_gpu.py
on the GPU).

The kernel's contract is  y[m, n] = sum_g s[n, g] * (sum_{k in g} a[m, k] * q[n, k]),  fp32
throughout, rounded to bf16 once after the epilogue's adds. The operands here make that ONE bit
pattern: activations are integers in [-4, 4], weights integers over the whole int4 range [-7, 7],
group scales powers of two from {0.5, 1, 2, 4} drawn per (column, group). Every partial sum is
then a multiple of 0.5 far below 2^24 (asserted, also for the kernel's own offset form, whose
products are a * (q + 24)), so it is exact in fp32 in whatever order a kernel adds, and the only
correct output is the float64 result rounded to bf16 once, to nearest even.

Everything is plain torch, drawn on the CPU from seeded generators, and runs on any device."""
from __future__ import annotations

from types import SimpleNamespace

import torch

import contract_cases as C
import exact_cases as X
from llm_sharding_amd.ops import int4, packing

GROUP = int4.INT4_GROUP
INT4_SCALES = (0.5, 1.0, 2.0, 4.0)
A_MAX, Q_MAX = 4, 7
KERNEL_OFFSET = 24            # gemv_int4.hip multiplies by q + 24 and subtracts 24 * sum(a) per group
MIN_SHARE = X.MIN_SHARE
ROWS = (1, 7, 16, 17, 33, 64)
KS = (128, 384, 1024)         # one group (idle waves); an odd group count against 4 and 8 waves; 8 groups
K_ROUND_MIN = 384             # at K = 128 most results are still bf16 values (|y| < 256 on the 0.5 grid): too few ties
QKV_GEOM = (4, 1, 32)         # n_heads, n_kv, head_dim: N = 192 = 16 * 4 * 3 (every tn divides its 12 tiles)


def all_codes(N: int, K: int) -> torch.Tensor:
    """int8 [N, K] cycling through the 15 code values -7..7 so that every value occurs in every
    nibble position of the packed 16-byte word, for every lane (the code at (n, k) is
    (k + 3 n + 5 (k // 32)) mod 15 - 7: 15 consecutive groups of 32 k shift it through all)."""
    n = torch.arange(N)[:, None]
    k = torch.arange(K)[None, :]
    return (((k + 3 * n + 5 * (k // 32)) % 15) - 7).to(torch.int8)


def group_scales(N: int, K: int, g, device) -> torch.Tensor:
    """fp32 [N, K / 128] from INT4_SCALES, drawn per (column, group)."""
    c = torch.tensor(INT4_SCALES, dtype=torch.float32, device=device)
    return c[X.randint(0, len(INT4_SCALES) - 1, (N, K // GROUP), g, device)]


class Weight:
    """An int4 weight in the forms the kernel and the references take: ``q`` int8 [N, K],
    ``scale`` fp32 [N, K/128], ``ref`` float64 = q * scale (what the kernel multiplies by),
    ``wq`` / ``sc`` the packed nibbles and packed scales."""

    def __init__(self, q: torch.Tensor, scale: torch.Tensor):
        self.q, self.scale = q.to(torch.int8), scale.float()
        self.ref = int4.dequantize_int4_groups(self.q, self.scale).double()
        self.wq = int4.pack_b_int4(self.q)
        self.sc = int4.pack_scales_int4(self.scale)
        self.wp = None


def assert_partial_sums(a: torch.Tensor, W: Weight, what: str) -> None:
    """Every partial sum a kernel can form, in any order, is below 2^24: the sum of the
    magnitudes of all terms of an output (contract form), and of the offset form's terms."""
    aa = a.double().abs()
    worst = float((aa @ W.ref.abs().T).max())
    assert worst < X.FP32_INT_MAX, f"{what}: sum of |a q s| reaches {worst}"
    smax = float(W.scale.max())
    worst_off = float(aa.sum(-1).max()) * (Q_MAX + 8 + 16 + KERNEL_OFFSET) * smax
    assert worst_off < X.FP32_INT_MAX, f"{what}: the offset form's partial sums reach {worst_off}"


def build_linear(M: int, N: int, K: int, seed: int, device="cpu", mode: str = "exact"):
    """A [M, K], W, a residual and a bias on the 0.5 grid, and the expected bf16 output of every
    store / residual epilogue form. ``round_once`` also asserts the shares of exact bf16 ties
    among the outputs and of residual outputs that rounding y first would change."""
    assert mode in ("exact", "round_once") and K % GROUP == 0
    g = X.gen(seed)
    a = X.randint(-A_MAX, A_MAX, (M, K), g, device)
    q = X.randint(-Q_MAX, Q_MAX, (N, K), g, device)
    X.assert_all_k_used(q, f"int4 linear {M}x{N}x{K}")
    W = Weight(q, group_scales(N, K, g, device))
    tag = f"int4 linear {mode} {M}x{N}x{K}"
    assert_partial_sums(a, W, tag)
    y = X.matmul(a, W.ref)
    resid = (X.randint(-2 * X.RESID_MAX, 2 * X.RESID_MAX, (M, N), g, device).double() * 0.5).to(torch.bfloat16)
    bias = (X.randint(-2 * X.RESID_MAX, 2 * X.RESID_MAX, (N,), g, device).double() * 0.5).float()
    assert bool(X.is_bf16(resid.double()).all())
    forms = {"store": y, "store_bias": y + bias.double(), "resid": resid.double() + y,
             "resid_bias": resid.double() + y + bias.double()}
    stats = {"tie_share": float(X.is_tie(y).float().mean())}
    twice = X.bf16_rne(X.bf16_rne(y).double() + resid.double())
    stats["double_rounding_share"] = float((C.bits(twice) != C.bits(X.bf16_rne(forms["resid"]))).float().mean())
    if mode == "round_once":
        assert stats["tie_share"] >= MIN_SHARE, f"{tag}: only {stats['tie_share']:.3%} of the outputs are RNE ties"
        assert stats["double_rounding_share"] >= MIN_SHARE, \
            f"{tag}: rounding y first changes only {stats['double_rounding_share']:.3%} of the residual outputs"
    exp = {k: X.bf16_rne(v) for k, v in forms.items()}
    unit = torch.full((N,), 0.5, dtype=torch.float64, device=device)
    return SimpleNamespace(M=M, N=N, K=K, mode=mode, a=a.to(torch.bfloat16), W=W, y=y, resid=resid, bias=bias, exp=exp,
                           unit=unit, stats=stats, tag=tag)


def build_one_hot(device="cpu"):
    """Every code value in every position: N = 16, K = 128, W = all_codes with one scale per
    column, and A = the 128 one-hot rows (row k selects k), to be run in batches of up to 64
    rows. Output row k, column n is exactly q[n, k] * s[n]."""
    N, K = 16, GROUP
    q = all_codes(N, K).to(device)
    per_pos = q.view(N, 4, 4, 8)  # [n, fragment h, k-quarter, j]: the nibble position is fixed by (h, j)
    for v in range(-Q_MAX, Q_MAX + 1):
        assert bool((per_pos == v).any(0).any(1).all()), f"code {v} misses a nibble position"
    scale = torch.tensor(INT4_SCALES, dtype=torch.float32, device=device)[torch.arange(N, device=device) % 4][:, None]
    W = Weight(q, scale)
    a = torch.eye(K, dtype=torch.bfloat16, device=device)
    return SimpleNamespace(M=K, N=N, K=K, a=a, W=W, exp=X.bf16_rne(W.ref.T.contiguous()), tag="int4 one-hot 128x16x128")


def build_swiglu(M: int, I: int, K: int, seed: int, device="cpu"):
    """The saturated-gate construction of exact_cases.build_swiglu (A = +-1, the last 64 k all
    +1 in A and in every gate row, scale 1 on the gate rows), with up rows over the full int4
    range and their own group scales: the output is bf16_rne(gate * up)."""
    assert K > X.GATE_BLOCK and K % GROUP == 0
    g = X.gen(seed)
    a = X.signs((M, K), g, device)
    a[:, K - X.GATE_BLOCK:] = 1
    wu = X.randint(-Q_MAX, Q_MAX, (I, K), g, device)
    wg = X.ternary(I, K, g, device, density=X.gate_density(K))
    wg[:, K - X.GATE_BLOCK:] = 1
    fused = packing.fuse_gate_up(wg, wu)
    X.assert_all_k_used(fused, f"int4 swiglu {M}x{I}x{K}")
    G = K // GROUP
    scale = packing.fuse_gate_up(torch.ones(I, G, device=device), group_scales(I, K, g, device))
    W = Weight(fused, scale)
    tag = f"int4 swiglu {M}x{I}x{K}"
    assert_partial_sums(a, W, tag)
    gu = X.matmul(a, W.ref).view(M, I // 16, 2, 16)
    gate, up = gu[:, :, 0].reshape(M, I), gu[:, :, 1].reshape(M, I)
    lo, hi = float(gate.min()), float(gate.max())
    assert X.GATE_LO <= lo and hi <= X.GATE_HI, f"{tag}: gate pre-activations span [{lo}, {hi}]"
    assert float((gate * up).abs().max()) < X.FP32_INT_MAX
    return SimpleNamespace(M=M, I=I, N=2 * I, K=K, a=a.to(torch.bfloat16), W=W, gate=gate, up=up,
                           exp=X.bf16_rne(gate * up), tag=tag, stats={"gate_min": lo, "gate_max": hi})


def build_qkv(M: int, K: int, seed: int, device="cpu", rope: bool = True, slots: int = 2):
    """exact_cases.build_qkv with int4 weights over the full range and group scales: ``rope``
    with packing.fuse_qkv and a table from exact_cases.ROPE_PAIRS, else the natural [q | k | v]
    order with a bias on the 0.5 grid. Every value is a multiple of 1/4 below 2^24, so the
    rotation is exact in fp32 with or without contraction."""
    nh, nkv, hd = QKV_GEOM
    g = X.gen(seed)
    N = (nh + 2 * nkv) * hd
    t_max = max(M, 2) + 5
    a = X.randint(-A_MAX, A_MAX, (M, K), g, device)
    wq, wk, wv = (X.randint(-Q_MAX, Q_MAX, (n * hd, K), g, device) for n in (nh, nkv, nkv))
    sq, sk, sv = (group_scales(n * hd, K, g, device) for n in (nh, nkv, nkv))
    nat = Weight(torch.cat([wq, wk, wv]), torch.cat([sq, sk, sv]))
    if rope:
        W = Weight(packing.fuse_qkv(wq, wk, wv, nh, nkv, hd), packing.fuse_qkv(sq, sk, sv, nh, nkv, hd))
    else:
        W = nat
    tag = f"int4 qkv {M} rows K {K} rope={rope}"
    assert_partial_sums(a, W, tag)
    others = 1 + torch.randperm(t_max - 2, generator=g).to(device)[:max(M - 2, 0)]
    pos = torch.cat([torch.tensor([0, t_max - 1], device=device), others])[:M]
    pos = pos[torch.randperm(M, generator=g).to(device)]
    assert pos.unique().numel() == M
    slot = X.randint(0, slots - 1, (M,), g, device)
    z = X.matmul(a, nat.ref)
    bias = None
    if not rope:
        bias = (X.randint(-2 * X.RESID_MAX, 2 * X.RESID_MAX, (N,), g, device).double() * 0.5).float()
        z = z + bias.double()
    zq, zk, zv = z[:, :nh * hd].view(M, nh, hd), z[:, nh * hd:(nh + nkv) * hd].view(M, nkv, hd), z[:, (nh + nkv) * hd:].view(M, nkv, hd)
    cos = sin = None
    if rope:
        cos, sin = X.rope_tables(t_max, hd, g, device)
        zq, zk = X.rotate_half_split(zq, cos[pos], sin[pos]), X.rotate_half_split(zk, cos[pos], sin[pos])
    return SimpleNamespace(M=M, N=N, K=K, nh=nh, nkv=nkv, hd=hd, t_max=t_max, slots=slots, rope=rope,
                           a=a.to(torch.bfloat16), W=W, z=z, bias=bias, cos=cos, sin=sin, pos=pos.to(torch.int32),
                           slot=slot.to(torch.int32), exp_q=X.bf16_rne(zq.reshape(M, nh * hd)), exp_k=X.bf16_rne(zk),
                           exp_v=X.bf16_rne(zv), tag=tag)


def build_gelu(M: int, N: int, K: int, seed: int, device="cpu"):
    """STORE + bias + GELU with an exactly known pre-activation: sparse +-1 activations and
    weights keep y small, the bias (multiples of 1/64 in [-4, 4]) spreads y + bias over the range
    where GELU bends; y + bias is exact in fp32. ``exact`` = ulp_cases.gelu64 of it."""
    import ulp_cases as U
    g = X.gen(seed)
    a = X.signs((M, K), g, device)
    q = X.ternary(N, K, g, device, density=min(1.0, 8.0 / K)) * X.randint(1, Q_MAX, (N, K), g, device)
    W = Weight(q, group_scales(N, K, g, device) * 0.125)  # scales 1/16 .. 1/2: y on the 1/16 grid
    assert_partial_sums(a, W, f"int4 gelu {M}x{N}x{K}")
    bias = (X.randint(-256, 256, (N,), g, device).double() / 64.0).float()
    v = X.matmul(a, W.ref) + bias.double()
    assert bool((v.float().double() == v).all())
    bend = float(((v.abs() < 6) & (v != 0)).float().mean())
    assert bend >= 0.25, f"int4 gelu {M}x{N}x{K}: only {bend:.1%} of the pre-activations lie where GELU bends"
    return SimpleNamespace(M=M, N=N, K=K, a=a.to(torch.bfloat16), W=W, bias=bias, inp=v, exact=U.gelu64(v),
                           tag=f"int4 gelu {M}x{N}x{K}")


def norm_case(M: int, N: int, K: int, seed: int, device="cpu"):
    """norm=True: +-2 activations, so mean(x^2) is exactly 4; with eps = 12 the RMSNorm factor is
    exactly 1 / 4 and y / 4 stays on a binary grid: the output is bf16_rne(y / 4) bitwise (an
    rsqrt a few 2^-23 off cannot move a multiple of 1/8 below 2^15 across a rounding boundary
    unless it is a tie, and ties are excluded by the builder)."""
    g = X.gen(seed)
    a = X.signs((M, K), g, device) * 2
    q = X.randint(-Q_MAX, Q_MAX, (N, K), g, device)
    W = Weight(q, group_scales(N, K, g, device))
    assert_partial_sums(a, W, f"int4 norm {M}x{N}x{K}")
    y = X.matmul(a, W.ref) / 4.0
    # an element is kept in the bitwise comparison unless it sits within 16 fp32 ulps of a bf16
    # rounding boundary (an exact tie included): there a few 2^-23 of error in the factor could decide
    assert bool((y.float().double() == y).all())
    low = y.float().view(torch.int32) & 0xFFFF
    safe = (low - 0x8000).abs() > 16
    assert float(safe.float().mean()) > 0.5
    return SimpleNamespace(M=M, N=N, K=K, a=a.to(torch.bfloat16), W=W, exp=X.bf16_rne(y), safe=safe, eps=12.0,
                           tag=f"int4 norm {M}x{N}x{K}")


def n_for(tn: int) -> int:
    return 16 * tn * 3


_CACHE = {}


def case(kind: str, *args, device="cpu"):
    """Built once per (kind, shape, device) and shared: treat it as read-only."""
    import zlib
    key = (kind,) + args + (str(device),)
    if key not in _CACHE:
        seed = zlib.crc32(repr((kind,) + args).encode()) & 0x7FFFFFFF
        b = {"linear": lambda: build_linear(*args, seed, device), "round_once": lambda: build_linear(*args, seed, device, mode="round_once"),
             "swiglu": lambda: build_swiglu(*args, seed, device), "qkv": lambda: build_qkv(args[0], args[1], seed, device, rope=args[2]),
             "gelu": lambda: build_gelu(*args, seed, device), "norm": lambda: norm_case(*args, seed, device),
             "one_hot": lambda: build_one_hot(device)}[kind]
        _CACHE[key] = b()
    return _CACHE[key]
