"""Half-ulp contract of the activation functions in the GEMM epilogues and of the stand-alone
normalisation kernels (tests/ulp_cases.py).

Every output element is compared with the float64 value of the same operation and must be its
correctly rounded bf16 value, up to 2^-7 ulp (activations) or 2^-6 ulp (norms): slacks derived in
ulp_cases.py from the fp32 operations a correct kernel performs, not from a measurement. The
activations see exactly known inputs (identity / one-hot weights, so the GEMM result is the A
element in every summation order) that sweep all bf16 patterns, plus fp32 values through the
bias; the norms see rows of very different scales side by side, with eps of first-order weight,
with a single non-zero element, all zero, of large mean and constant. tests/test_ulp_cases.py
shows on the CPU that the checker accepts a float32 emulation of the correct formulas and rejects
a cancelling GELU, truncation, an early rounding, a missing eps, a wrong 1 / H, a weight applied
after the rounding, a neighbour's sum and a one-pass variance. Every test prints its worst excess
over half an ulp."""
from collections import Counter

import pytest
import torch

import contract_cases as C
import exact_cases as X
import ulp_cases as U
from llm_sharding_amd.ops import packing
from test_footprint_gpu import l_fp8, l_gemv, l_proj_fp8, l_wr

pytestmark = pytest.mark.gpu
DEV = "cuda"
K = N = U.K_ACT
M_COOP = {"gelu": 2 * U.R_GELU, "swiglu": 2 * U.R_SWIGLU}  # the cooperative kernels take 17 .. 128 rows


def hip():
    from llm_sharding_amd.ops import hip as h
    h.lib()
    return h


@pytest.fixture(scope="module")
def coop_ws():
    return hip().CoopWorkspace(DEV, slab_floats=1 << 24, groups=1 << 10)


@pytest.fixture(scope="module")
def sk_ws():
    return hip().SkWorkspace(DEV, grid=256, bn=256)


# ------------------------------------------------------------------------------ one legal config per family
def _families(h, kind, coop_ws, sk_ws):
    """name -> (launcher, rows): every family that carries the epilogue, at one legal config."""
    swiglu = kind == "swiglu"
    R = U.R_SWIGLU if swiglu else U.R_GELU
    n_tiles = (2 * N if swiglu else N) // 16
    tn, nw, u = packing.gemv_candidates(n_tiles, K, R, swiglu)[0]
    Mc = M_COOP[kind]
    coop = next(c for c in packing.coop_candidates(n_tiles, K, Mc, swiglu) if c[3] >= 1)
    coop8 = next(c for c in packing.coop_fp8_candidates(n_tiles, K, Mc) if not swiglu or (c[0] * c[1]) % 2 == 0)

    def legacy(x, w, M, N_, K_, epi, ep, ar, norm):
        h.gemm(x, w.wp, M, N_, K_, epi, ep, legacy=True)

    def sk(x, w, M, N_, K_, epi, ep, ar, norm):
        h.gemm_sk(x, w.wp, M, N_, K_, epi, ep, ws=sk_ws)

    fams = {"gemv": (l_gemv(h, tn=tn, nw=nw, u=u), R), "gemv_coop": (l_gemv(h, coop=coop, ws=coop_ws), Mc),
            "gemv_fp8": (l_fp8(h), R), "coop_fp8": (l_proj_fp8(h, ("coop_fp8", coop8), coop_ws), Mc),
            "gemm": (legacy, U.M_GEMM), "gemm_sk": (sk, U.M_GEMM)}
    if swiglu:
        fams["gemm_wr"] = (l_wr(h, 128), U.M_GEMM)
    return fams


GELU_FAMILIES = ("gemv", "gemv_coop", "gemv_fp8", "coop_fp8", "gemm", "gemm_sk")
SWIGLU_FAMILIES = GELU_FAMILIES + ("gemm_wr",)


def _rows(t, M):
    return U.repeat_rows(t, M).contiguous()


@pytest.mark.parametrize("family", GELU_FAMILIES)
def test_gelu(family, coop_ws, sk_ws):
    """STORE + GELU: the bf16 grid with no bias and with a zero bias array, then two fp32 sweeps
    through the bias (A = 0), whose rows must also be bitwise equal."""
    h = hip()
    launch, M = _families(h, "gelu", coop_ws, sk_ws)[family]
    w = U.weight("store", DEV)
    ran = Counter()
    g = U.gelu_grid()
    a, exact, zero, inp = (_rows(t, M) for t in (g.a, g.exact, g.zero, g.inp))
    a = a.to(DEV)
    for bias in (None, torch.zeros(N, dtype=torch.float32, device=DEV)):
        obuf, out = C.guarded(M, N, device=DEV)
        launch(a, w, M, N, K, h.EPI_STORE, h.make_epi(out=out, ldo=out.stride(0), bias=bias, act=h.ACT_GELU), None, False)
        torch.cuda.synchronize()
        tag = f"{family} {g.tag} M {M} bias {'zero' if bias is not None else 'none'}"
        C.assert_footprint(obuf, out, what=tag)
        worst = U.assert_half_ulp(out, exact, U.SLACK_ACT, tag, inp=inp, zero=zero)
        print(f"{tag}: worst excess over 1/2 ulp {worst:.3g} ulp")
        ran["grid"] += 1
    a0 = torch.zeros(M, K, dtype=torch.bfloat16, device=DEV)
    for seed in U.BIAS_SEEDS:
        c = U.gelu_bias(seed)
        obuf, out = C.guarded(M, N, device=DEV)
        ep = h.make_epi(out=out, ldo=out.stride(0), bias=c.bias.to(DEV), act=h.ACT_GELU)
        launch(a0, w, M, N, K, h.EPI_STORE, ep, None, False)
        torch.cuda.synchronize()
        tag = f"{family} {c.tag} M {M}"
        C.assert_footprint(obuf, out, what=tag)
        worst = U.assert_half_ulp(out, c.exact[:1].expand(M, N), U.SLACK_ACT, tag, inp=c.inp)
        X.assert_bits_equal(out, out[:1].expand(M, N).contiguous(), tag + " rows equal")
        print(f"{tag}: worst excess over 1/2 ulp {worst:.3g} ulp")
        ran["bias"] += 1
    assert ran == {"grid": 2, "bias": len(U.BIAS_SEEDS)}, (family, dict(ran))
    assert int(coop_ws.counters.abs().sum()) == 0 and int(sk_ws.counters.abs().sum()) == 0


@pytest.mark.parametrize("family", SWIGLU_FAMILIES)
def test_swiglu(family, coop_ws, sk_ws):
    """silu(gate) u with the gate sweeping the bf16 grid and u in {1, 3, -0.5, 0.15625}: the
    product is rounded once."""
    h = hip()
    launch, M = _families(h, "swiglu", coop_ws, sk_ws)[family]
    w = U.weight("swiglu", DEV)
    s = U.swiglu_grid()
    a, exact, zero, inp = (_rows(t, M) for t in (s.a, s.exact, s.zero, s.inp))
    obuf, out = C.guarded(M, N, device=DEV)
    launch(a.to(DEV), w, M, 2 * N, K, h.EPI_SWIGLU, h.make_epi(out=out, ldo=out.stride(0)), None, False)
    torch.cuda.synchronize()
    tag = f"{family} {s.tag} M {M}"
    C.assert_footprint(obuf, out, what=tag)
    worst = U.assert_half_ulp(out, exact, U.SLACK_ACT, tag, inp=inp, zero=zero)
    print(f"{tag}: worst excess over 1/2 ulp {worst:.3g} ulp")
    assert int(coop_ws.counters.abs().sum()) == 0 and int(sk_ws.counters.abs().sum()) == 0


# ------------------------------------------------------------------------------ norms
def _zero_rows(rows, H, r):
    z = torch.zeros(rows, H, dtype=torch.bool)
    z[r] = True
    return z


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("H", U.RMS_GENERIC + U.RMS_REG)
def test_rmsnorm(H, weighted):
    """lsa_rmsnorm: the generic loop (768: most threads idle; 3072: some take two chunks) and the
    four register-resident widths, ldx = H + 64, ldo = H + 128, eps = 1e-5 and 1e-6."""
    h = hip()
    c = U.rms_case(H)
    xbuf, x = C.guarded(c.rows, H, device=DEV)
    x.copy_(c.x)
    w = c.w.to(DEV) if weighted else None
    for eps in U.RMS_EPS:
        obuf, out = C.guarded(c.rows, H, device=DEV, guard_cols=128)
        assert x.stride(0) == H + 64 and out.stride(0) == H + 128
        h.rmsnorm(x, w, out, c.rows, eps, H)
        torch.cuda.synchronize()
        tag = f"rmsnorm H {H} eps {eps} weighted {weighted}"
        C.assert_footprint(obuf, out, what=tag)
        X.assert_bits_equal(x, c.x.to(DEV), tag + " x unchanged")
        worst = U.assert_half_ulp(out, U.rms_exact(c.x, c.w if weighted else None, eps), U.SLACK_NORM, tag,
                                  zero=_zero_rows(c.rows, H, c.zero_row))
        print(f"{tag}: worst excess over 1/2 ulp {worst:.3g} ulp")


@pytest.mark.parametrize("mode", ["weighted", "unweighted", "no_out"])
@pytest.mark.parametrize("H,S", U.PARTIAL_CASES)
def test_resid_rmsnorm_partials(H, S, mode):
    """h bitwise (integer partials and residual), out against the float64 norm of the rounded h."""
    h = hip()
    c = U.partial_case(H, S)
    hbuf, hw = C.guarded(c.rows, H, device=DEV)
    hw.copy_(c.resid)
    obuf, out = C.guarded(c.rows, H, device=DEV, guard_cols=128)
    w = c.w.to(DEV) if mode == "weighted" else None
    h.resid_rmsnorm_partials(hw, c.P.to(DEV), S, c.rows, 1e-5, out=None if mode == "no_out" else out, w=w)
    torch.cuda.synchronize()
    tag = f"resid_rmsnorm_partials H {H} S {S} {mode}"
    C.assert_footprint(hbuf, hw, what=tag + " h")
    X.assert_bits_equal(hw, c.h.to(DEV), tag + " h")
    if mode == "no_out":
        assert bool(C.is_sentinel(obuf).all())
        return
    C.assert_footprint(obuf, out, what=tag + " out")
    worst = U.assert_half_ulp(out, U.rms_exact(c.h, c.w if mode == "weighted" else None, 1e-5), U.SLACK_NORM, tag,
                              zero=_zero_rows(c.rows, H, c.zero_row))
    print(f"{tag}: worst excess over 1/2 ulp {worst:.3g} ulp")


@pytest.mark.parametrize("with_pos", [False, True])
@pytest.mark.parametrize("H", U.LN_WIDTHS)
def test_layernorm(H, with_pos):
    """lsa_layernorm: the written-back x bitwise, out within the slack counted in ulps of
    |t| (1 + |mu| / sigma) + |b|, the constant row equal to the bias bitwise."""
    h = hip()
    c = U.layernorm_case(H, with_pos)
    xbuf, x = C.guarded(c.rows, H, device=DEV)
    x.copy_(c.x)
    obuf, out = C.guarded(c.rows, H, device=DEV, guard_cols=128)
    h.layernorm(x, out, c.g.to(DEV), c.b.to(DEV), c.rows, U.LN_EPS, pos_emb=c.pe.to(DEV) if with_pos else None,
                pos=c.pos.to(DEV) if with_pos else None)
    torch.cuda.synchronize()
    tag = f"layernorm H {H} pos add {with_pos}"
    C.assert_footprint(obuf, out, what=tag + " out")
    C.assert_footprint(xbuf, x, what=tag + " x")
    X.assert_bits_equal(x, c.xr.to(DEV), tag + " x")
    exact, scale = U.layernorm_exact(c.xr, c.g, c.b, U.LN_EPS)
    worst = U.assert_half_ulp(out, exact, U.SLACK_NORM, tag, scale=scale)
    X.assert_bits_equal(out[c.const], c.b.to(DEV), tag + " constant row")
    print(f"{tag}: worst excess over 1/2 ulp {worst:.3g} ulp of the scale")
