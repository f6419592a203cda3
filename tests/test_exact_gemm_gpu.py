"""Exact-arithmetic contract of every projection kernel and epilogue (tests/exact_cases.py).

The operands are small integers, so every fp32 partial sum is exact in whatever order a kernel
adds and the only correct output is one bit pattern: the integer result itself (``exact_int``),
or the exact result rounded to bf16 once, to nearest even (``round_once``: a share of the
results are exact ties, and with a residual rounding y first gives other bits). Every family,
config, split plan and epilogue must produce those bits: one dropped or duplicated (row, column,
k) product, a K step taken from the wrong tile, a residual add rounded twice, truncation, a
wrong arg-max tie rule or a wrong RoPE partner / sign in any frequency is a failed comparison
here, and the message reads off how many products an element is away. Nothing below depends on
a number measured on a GPU; tests/test_exact_cases.py shows on the CPU that the checkers reject
each of those faults and that the builders' conditions hold at every shape used here.

The one comparison that is not bitwise is the fused RMSNorm (one bf16 ulp, see test_fused_rmsnorm).
"""
from collections import Counter

import pytest
import torch

import contract_cases as C
import exact_cases as X
from llm_sharding_amd.ops import packing
from test_footprint_gpu import l_fp8, l_gemv, l_proj_fp8, l_wr

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-5
LINEAR_FORMS = ("store", "store_bias", "resid", "resid_bias")


def hip():
    from llm_sharding_amd.ops import hip as h
    h.lib()
    return h


class NoConfig(Exception):
    """The launcher has no legal plan of its config for this shape (the caller counts what ran)."""


# ------------------------------------------------------------------------------ one launch, one check
def run_linear(h, launch, key, forms=LINEAR_FORMS, what=""):
    c = X.case(key, DEV)
    n = 0
    for form in forms:
        obuf, out = C.guarded(c.M, c.N, device=DEV)
        bias = c.bias if form.endswith("bias") else None
        if form.startswith("store"):
            ep = h.make_epi(out=out, ldo=out.stride(0), bias=bias)
            launch(c.a, c.W, c.M, c.N, c.K, h.EPI_STORE, ep, None, False)
        else:
            ep = h.make_epi(out=out, resid=c.resid, ldo=out.stride(0), ldr=c.resid.stride(0), bias=bias)
            launch(c.a, c.W, c.M, c.N, c.K, h.EPI_RESID, ep, None, False)
        torch.cuda.synchronize()
        tag = f"{what} {c.tag} {form}"
        C.assert_footprint(obuf, out, what=tag)
        X.assert_bits_equal(out, c.exp[form], tag, unit=c.unit)
        n += 1
    return n


def run_swiglu(h, launch, key, what=""):
    c = X.case(key, DEV)
    obuf, out = C.guarded(c.M, c.I, device=DEV)
    launch(c.a, c.W, c.M, c.N, c.K, h.EPI_SWIGLU, h.make_epi(out=out, ldo=out.stride(0)), None, False)
    torch.cuda.synchronize()
    C.assert_footprint(obuf, out, what=f"{what} {c.tag}")
    X.assert_bits_equal(out, c.exp, f"{what} {c.tag}")
    return 1


def run_qkv(h, launch, key, what=""):
    c = X.case(key, DEV)
    qbuf, q = C.guarded(c.M, c.nh * c.hd, device=DEV)
    kflat, kc = C.guarded_cache(c.slots, c.nkv, c.t_max, c.hd, DEV)
    vflat, vc = C.guarded_cache(c.slots, c.nkv, c.t_max, c.hd, DEV)
    ep = h.make_epi(out=q, k_cache=kc, v_cache=vc, slot=c.slot, pos=c.pos, cos=c.cos, sin=c.sin, ldo=q.stride(0),
                    n_heads=c.nh, n_kv=c.nkv, head_dim=c.hd, t_max=c.t_max, bias=c.bias)
    launch(c.a, c.W, c.M, c.N, c.K, h.EPI_QKV, ep, None, False)
    torch.cuda.synchronize()
    C.assert_footprint(qbuf, q, what=f"{what} {c.tag} q")
    X.check_qkv(c, q, kflat, kc, vflat, vc, f"{what} {c.tag}")
    return 1


_HALVES = {}


def _halves(key):
    """The lm_head of an arg-max case as two vocabulary chunks (weights, bias, column offset)."""
    if key not in _HALVES:
        c = X.case(key, DEV)
        half = c.V // 2
        _HALVES[key] = [(X.Weight(c.w[lo:hi], None if c.scale is None else c.scale[lo:hi]),
                         None if c.bias is None else c.bias[lo:hi].contiguous(), lo) for lo, hi in ((0, half), (half, c.V))]
    return _HALVES[key]


def run_argmax(h, launch, key, what="", chunked=False):
    """EPI_ARGMAX + argmax_finalize: the smallest tied column. ``chunked``: the vocabulary in two
    launches with their column offsets into one keys array, the upper half first; then the lower
    half alone shifted by a column offset (the expected token moves with it)."""
    c = X.case(key, DEV)
    tok = torch.empty(c.M, dtype=torch.int32, device=DEV)
    keys = torch.zeros(c.M, dtype=torch.int64, device=DEV)
    if not chunked:
        launch(c.a, c.W, c.M, c.N, c.K, h.EPI_ARGMAX, h.make_epi(keys=keys, bias=c.bias), None, False)
        h.argmax_finalize(keys, c.M, tok)
        torch.cuda.synchronize()
        X.assert_tokens(tok, c, f"{what} {c.tag}")
        assert bool((keys == 0).all())
        return 1
    parts = _halves(key)
    for W, bias, off in reversed(parts):
        launch(c.a, W, c.M, c.V // 2, c.K, h.EPI_ARGMAX, h.make_epi(keys=keys, bias=bias, col_offset=off), None, False)
    h.argmax_finalize(keys, c.M, tok)
    torch.cuda.synchronize()
    X.assert_tokens(tok, c, f"{what} {c.tag} two chunks")
    # the lower chunk alone at an offset: rows whose smallest tied column lies in it give offset + column
    W, bias, _ = parts[0]
    launch(c.a, W, c.M, c.V // 2, c.K, h.EPI_ARGMAX, h.make_epi(keys=keys, bias=bias, col_offset=1000), None, False)
    h.argmax_finalize(keys, c.M, tok)
    torch.cuda.synchronize()
    lo = torch.tensor([min([x for x in cs if x < c.V // 2], default=-1) for cs in c.cols], dtype=torch.int32, device=DEV)
    tied = lo >= 0  # (a row with no planted column in this chunk has some other, untied maximum)
    assert bool(tied[0]) and torch.equal(tok[tied], lo[tied] + 1000), \
        f"{what} {c.tag} col_offset 1000: {tok[tied].tolist()} != {(lo[tied] + 1000).tolist()}"
    return 2


def _try(fn, *a, **kw):
    try:
        return fn(*a, **kw)
    except NoConfig:
        return 0


def require(ran: Counter, kinds, what) -> None:
    """Every epilogue kind in ``kinds`` ran at least one check (a launcher without a legal plan
    for a shape raises NoConfig and counts nothing, so a total alone would hide a kind that never ran)."""
    missing = [k for k in kinds if ran[k] <= 0]
    assert not missing, f"{what}: no check ran for {missing} (ran: {dict(ran)})"


DECODE_KINDS = ("linear", "round_once", "qkv", "argmax", "argmax_neg", "argmax_chunked")
FP8_KINDS = ("linear", "round_once", "argmax", "argmax_chunked")
GEMM_KINDS = ("linear", "round_once", "qkv")


def decode_suite(h, launch, M, K, what, swiglu=True, fp8=False, epi=None, V=X.V_ARGMAX) -> Counter:
    """Every epilogue of a decode family at (M, K); returns the checks that ran, per kind. QKV and
    arg-max run where ``epi`` says so (default: at K = 768 only)."""
    s = "_fp8" if fp8 else ""
    n = Counter()
    n["linear"] += _try(run_linear, h, launch, ("linear" + s, M, X.N_LIN, K), what=what)
    if K >= X.K_ROUND_MIN:
        n["round_once"] += _try(run_linear, h, launch, ("round_once" + s, M, X.N_LIN, K), forms=("store", "resid", "resid_bias"),
                                what=what)
    if swiglu:
        n["swiglu"] += _try(run_swiglu, h, launch, ("swiglu" + s, M, X.I_SWIGLU, K), what=what)
    if not (K == X.K_EPI if epi is None else epi):
        return n
    if not fp8:
        for hd, rope in ((64, True), (128, True), (64, False)):
            n["qkv"] += _try(run_qkv, h, launch, ("qkv", M, hd, K, rope), what=what)
        n["argmax_neg"] += _try(run_argmax, h, launch, ("argmax_neg", M, V, K), what=what)
    akey = ("argmax" + s, M, V, K)
    n["argmax"] += _try(run_argmax, h, launch, akey, what=what)
    n["argmax_chunked"] += _try(run_argmax, h, launch, akey, what=what, chunked=True)
    return n


def gemm_suite(h, launch, M, K, what, resid=True, bias=True, swiglu=True, N=X.N_LIN, I=X.I_SWIGLU, suffix="") -> Counter:
    """Every epilogue of a GEMM family at (M, K): QKV at the short K, round_once at the long ones
    (too few results leave the bf16 integers below K = 768); a family without a bias takes the
    RoPE form of QKV only (the GPT-2 form carries one). ``N`` / ``I`` other than the defaults: the
    store / residual / SwiGLU forms at that width (no QKV geometry), counted under kind + suffix."""
    forms = [f for f in LINEAR_FORMS if (resid or f.startswith("store")) and (bias or not f.endswith("bias"))]
    n = Counter()
    n["linear" + suffix] += _try(run_linear, h, launch, ("linear", M, N, K), forms=forms, what=what)
    if swiglu:
        n["swiglu" + suffix] += _try(run_swiglu, h, launch, ("swiglu", M, I, K), what=what)
    if K >= X.K_ROUND_MIN:
        n["round_once" + suffix] += _try(run_linear, h, launch, ("round_once", M, N, K), forms=[f for f in forms if f != "store_bias"],
                                         what=what)
    elif N == X.N_LIN:
        for hd, rope in ((64, True), (128, True), (64, False)):
            if rope or bias:
                n["qkv"] += _try(run_qkv, h, launch, ("qkv", M, hd, K, rope), what=what)
    return n


# ------------------------------------------------------------------------------ launchers
def l_coop(h, ws, cfg, pick):
    """The cooperative kernel with config ``cfg`` = (tnw, nw, kf, kw, d) at its smallest / largest
    legal K split (``pick`` = min / max) for the launch's own shape."""
    def f(x, w, M, N, K, epi, ep, ar, norm):
        cands = [c for c in packing.coop_candidates(N // 16, K, M, epi == h.EPI_SWIGLU)
                 if (c[0], c[1], c[2], c[4], c[5]) == cfg and c[3] >= 1]
        if not cands:
            raise NoConfig
        c = pick(cands, key=lambda c: c[3])
        f.used.add((N, K, c[3]))
        f.choice |= len({c[3] for c in cands}) > 1
        h.gemv(x, w.wp, M, N, K, epi, ep, norm=norm, eps=EPS, a_rows=ar, coop=c, ws=ws)
    f.used, f.choice = set(), False
    return f


def l_coop_fp8(h, ws, cfg, pick):
    def f(x, w, M, N, K, epi, ep, ar, norm):
        cands = [c for c in packing.coop_fp8_candidates(N // 16, K, M) if c[:3] == cfg]
        if not cands or (epi == h.EPI_SWIGLU and (cfg[0] * cfg[1]) % 2):
            raise NoConfig
        c = pick(cands, key=lambda c: c[3])
        f.used.add((N, K, c[3]))
        f.choice |= len({c[3] for c in cands}) > 1
        h.proj_fp8(x, w.wq, w.sc, M, N, K, epi, ep, norm=norm, eps=EPS, a_rows=ar, algo=("coop_fp8", c), ws=ws)
    f.used, f.choice = set(), False
    return f


def require_two_splits(lo, hi, what) -> None:
    """The min and the max launcher both ran, and where a shape offered more than one K split
    they ran different ones."""
    assert lo.used and hi.used, what
    assert not lo.choice or lo.used != hi.used, f"{what}: smallest and largest split are the same launches {sorted(lo.used)}"


def l_legacy(h, sk):
    def f(x, w, M, N, K, epi, ep, ar, norm):
        assert ar is None and not norm
        h.gemm(x, w.wp, M, N, K, epi, ep, sk=sk, legacy=True)
    return f


def l_sk_cfg(h, ws, bm, cfg):
    """gemm_sk with one (bn, grid, dp, split) of tests/test_gemm_sk_gpu.py::CFGS, skipped for a
    shape exactly where that file skips it."""
    bn, grid, dp, split = cfg

    def f(x, w, M, N, K, epi, ep, ar, norm):
        assert ar is None and not norm
        tiles = -(-M // bm) * -(-N // (bn or 256))
        if (bn and N % (16 if bn == 192 else bn)) or (split > 0 and tiles * split > grid):
            raise NoConfig
        h.gemm_sk(x, w.wp, M, N, K, epi, ep, bn=bn, grid=grid, dp=dp, split=split, nb=2 if (bn, grid) == (128, 96) else 0,
                  ws=ws, bm=bm if bn else 0)
    return f


@pytest.fixture(scope="module")
def coop_ws():
    return hip().CoopWorkspace(DEV, slab_floats=1 << 24, groups=1 << 10)


@pytest.fixture(scope="module")
def sk_ws():
    return hip().SkWorkspace(DEV, grid=1024, bn=256)


# ------------------------------------------------------------------------------ decode families
@pytest.mark.parametrize("cfg", packing.GEMV_CONFIGS)
def test_gemv_every_config(cfg):
    """Every instantiated streaming-GEMV config, K = 768 and 11008 (uneven per-wave K splits),
    every epilogue."""
    h = hip()
    tn, mb, nw, u = cfg
    tested = Counter()
    for M in X.GEMV_ROWS[mb]:
        for K in (768, 11008):
            if (K // 32) % u:
                continue
            tested += decode_suite(h, l_gemv(h, tn=tn, nw=nw, u=u), M, K, f"gemv {cfg}", swiglu=tn % 2 == 0)
    require(tested, DECODE_KINDS + (("swiglu",) if tn % 2 == 0 else ()), cfg)


@pytest.mark.parametrize("cfg", packing.COOP_CONFIGS)
def test_coop_every_config(cfg, coop_ws):
    """Every instantiated cooperative config (k-groups kw > 1 included) at its smallest and its
    largest legal K split, every epilogue; the arrival counters are zero afterwards."""
    h = hip()
    mb, tnw, nw, kf, kw, d = cfg
    M = X.COOP_ROWS[mb]
    tested, Ls = Counter(), []
    for pick in (min, max):
        L = l_coop(h, coop_ws, (tnw, nw, kf, kw, d), pick)
        Ls.append(L)
        for K in X.K_COOP:
            tested += decode_suite(h, L, M, K, f"coop {cfg} {pick.__name__} split", epi=K in X.K_COOP_EPI, V=X.V_COOP)
    # (SwiGLU needs an even number of tiles per workgroup: one gate / up pair at least)
    require(tested, DECODE_KINDS + (("swiglu",) if (tnw * nw) % 2 == 0 else ()), cfg)
    require_two_splits(*Ls, cfg)
    assert int(coop_ws.counters.abs().sum()) == 0


def test_coop_ragged(coop_ws):
    """The ragged mode (sk = 0: the tiles dealt to one workgroup per CU): a residual projection of
    300 tiles and the 32000-column lm_head with ties across deals."""
    h = hip()
    tested = 0
    for key, run in ((("linear", 50, X.N_RAGGED, 256), run_linear), (("argmax", 50, X.V_RAGGED, 256), run_argmax)):
        c = X.case(key, DEV)
        ragged = [cand for cand in packing.coop_candidates(c.N // 16, c.K, c.M) if cand[3] == 0]
        assert len(ragged) > 0, key
        for cand in ragged[:3]:
            tested += run(h, l_gemv(h, coop=cand, ws=coop_ws), key, what=f"coop ragged {cand}")
    assert tested > 0
    assert int(coop_ws.counters.abs().sum()) == 0


@pytest.mark.parametrize("M", sorted(X.COOP_ROWS.values()))
def test_coop_partial(M, coop_ws):
    """EPI_PARTIAL: every split's fp32 partial is an integer matrix, their float64 sum is the
    integer result, and lsa_resid_rmsnorm_partials leaves the updated residual stream bitwise."""
    h = hip()
    c = X.case(("linear", M, X.N_PARTIAL, 512), DEV)
    tested = 0
    seen = set()
    for cand in packing.coop_candidates(c.N // 16, c.K, M):
        if not 2 <= cand[3] <= 8 or (cand[3], cand[4]) in seen or tested >= 4:
            continue
        seen.add((cand[3], cand[4]))
        _check_partials(h, c, cand[3], f"coop partial {cand}",
                        lambda ep, n: h.gemv(c.a, c.W.wp, M, c.N, c.K, h.EPI_PARTIAL, ep, coop=cand, ws=coop_ws, out_numel=n))
        tested += 1
    assert tested > 0
    assert int(coop_ws.counters.abs().sum()) == 0


def _check_partials(h, c, S, tag, launch):
    pbuf, P = C.guarded_flat(S * c.M * c.N, torch.float32, DEV)
    launch(h.make_epi(out=P, ldo=c.N), P.numel())
    torch.cuda.synchronize()
    C.assert_footprint(pbuf, P, what=tag)
    Pv = P.view(S, c.M, c.N)
    assert bool((Pv == Pv.round()).all()), tag + ": a split's partial is not an integer matrix"
    X.assert_bits_equal(Pv.double().sum(0), c.y, tag + " sum of the partials", unit=c.unit)
    hb = c.resid.clone()
    h.resid_rmsnorm_partials(hb, Pv, S, c.M, EPS)
    torch.cuda.synchronize()
    X.assert_bits_equal(hb, c.exp["resid"], tag + " resid_rmsnorm_partials h", unit=c.unit)


@pytest.mark.parametrize("cfg", packing.FP8_CONFIGS)
def test_gemv_fp8_every_config(cfg):
    h = hip()
    tn, mb, nw, u2 = cfg
    tested = Counter()
    for M in X.GEMV_ROWS[mb]:
        assert (X.K_EPI // 32) % (2 * u2) == 0
        tested += decode_suite(h, l_fp8(h, (tn, nw, u2)), M, X.K_EPI, f"fp8 {cfg}", swiglu=tn % 2 == 0, fp8=True)
    require(tested, FP8_KINDS + (("swiglu",) if tn % 2 == 0 else ()), cfg)


@pytest.mark.parametrize("cfg", packing.COOP_FP8_CONFIGS)
def test_coop_fp8_every_config(cfg, coop_ws):
    h = hip()
    mb, tnw, nw, kf = cfg
    tested, Ls = Counter(), []
    for pick in (min, max):
        L = l_coop_fp8(h, coop_ws, (tnw, nw, kf), pick)
        Ls.append(L)
        tested += decode_suite(h, L, X.COOP_ROWS[mb], X.K_EPI, f"coop_fp8 {cfg} {pick.__name__} split", fp8=True)
    require(tested, FP8_KINDS + ("swiglu",), cfg)
    require_two_splits(*Ls, cfg)
    assert int(coop_ws.counters.abs().sum()) == 0


@pytest.mark.parametrize("M", [1, 16, 17, 50, 128])
def test_default_dispatch(M, coop_ws):
    """hip.gemv's and hip.proj_fp8's own choice of kernel and config."""
    h = hip()
    require(decode_suite(h, l_gemv(h, ws=coop_ws), M, X.K_EPI, "gemv dispatch"), DECODE_KINDS + ("swiglu",), M)
    require(decode_suite(h, l_proj_fp8(h, None, coop_ws), M, X.K_EPI, "proj_fp8 dispatch", fp8=True), FP8_KINDS + ("swiglu",), M)
    assert int(coop_ws.counters.abs().sum()) == 0


# ------------------------------------------------------------------------------ GEMMs
@pytest.mark.parametrize("sk", [0, 3])
def test_gemm_legacy(sk):
    """gemm.hip with its own split (1 at K = 256, 2 at K = 1216) and a forced uneven 3-way split."""
    h = hip()
    tested = Counter()
    for M in X.GEMM_ROWS["gemm"]:
        for K in X.K_GEMM:
            tested += gemm_suite(h, l_legacy(h, sk), M, K, f"gemm legacy sk {sk}")
    require(tested, GEMM_KINDS + ("swiglu",), sk)
    assert int(h.default_workspace().counters.abs().sum()) == 0


def _sk_cfgs():
    from test_gemm_sk_gpu import BMS, CFGS
    return [(bm, cfg) for bm in BMS for cfg in CFGS if cfg[0] or bm == 256]


@pytest.mark.parametrize("bm,cfg", _sk_cfgs())
def test_gemm_sk(bm, cfg, sk_ws):
    """BMS x CFGS of tests/test_gemm_sk_gpu.py: whole tiles, stream-K, equal 2 / 3 / 8-way splits,
    odd grids, bn 128 / 192 / 256 - store, resid (+ bias), SwiGLU, QKV. The bn = 192 plans also
    run N = 640 = 3 x 192 + 64 (SwiGLU: 2 x 320), where the last column tile is partial."""
    h = hip()
    tested = Counter()
    kinds = GEMM_KINDS + ("swiglu",)
    for M in X.GEMM_ROWS["gemm_sk"]:
        for K in X.K_GEMM:
            L = l_sk_cfg(h, sk_ws, bm, cfg)
            tested += gemm_suite(h, L, M, K, f"gemm_sk bm {bm} cfg {cfg}")
            if cfg[0] == 192:
                tested += gemm_suite(h, L, M, K, f"gemm_sk bm {bm} cfg {cfg} partial tile", N=X.N_EDGE, I=X.I_EDGE, suffix="@640")
    if cfg[0] == 192:
        assert X.N_EDGE % 192 and (2 * X.I_EDGE) % 192
        kinds += ("linear@640", "round_once@640", "swiglu@640")
    require(tested, kinds, (bm, cfg))
    assert int(sk_ws.counters.abs().sum()) == 0


@pytest.mark.parametrize("bn", [128, 256])  # (ss_out has no 192-wide form)
@pytest.mark.parametrize("bm", [128, 256])
def test_gemm_sk_ss_out_and_partial(bm, bn, sk_ws):
    """EPI_RESID with ss_out: exactly the per-64-column sums of squares of the integer outputs.
    EPI_PARTIAL: integer partials whose sum is the integer result, then the updated h bitwise."""
    h = hip()
    tested = 0
    for M in X.GEMM_ROWS["gemm_sk"]:
        c = X.case(("linear", M, X.N_LIN, 1216), DEV)
        for (grid, dp, split) in ((256, 1, 1), (256, 1, 2), (37, 0, 0), (256, 0, 3)):
            if split > 0 and -(-M // bm) * (c.N // bn) * split > grid:
                continue
            obuf, out = C.guarded(M, c.N, device=DEV)
            sbuf, ss = C.guarded(M, c.N // 64, torch.float32, DEV, guard_cols=0)
            ep = h.make_epi(out=out, resid=c.resid, ldo=out.stride(0), ldr=c.N, ss_out=ss)
            h.gemm_sk(c.a, c.W.wp, M, c.N, c.K, h.EPI_RESID, ep, bn=bn, grid=grid, dp=dp, split=split, ws=sk_ws, bm=bm)
            torch.cuda.synchronize()
            tag = f"gemm_sk ss_out bm {bm} bn {bn} M {M} plan {(grid, dp, split)}"
            C.assert_footprint(obuf, out, what=tag)
            C.assert_footprint(sbuf, ss, what=tag + " ss")
            X.assert_bits_equal(out, c.exp["resid"], tag, unit=c.unit)
            X.assert_bits_equal(ss.contiguous(), X.expected_ss(c.exp["resid"]), tag + " ss")
            tested += 1
        p = X.case(("linear", M, X.N_PARTIAL, 512), DEV)
        for S in (2, 3, 8):
            if -(-M // bm) * (p.N // bn) * S > 1024:
                continue
            _check_partials(h, p, S, f"gemm_sk partial bm {bm} bn {bn} M {M} split {S}",
                            lambda ep, n: h.gemm_sk(p.a, p.W.wp, M, p.N, p.K, h.EPI_PARTIAL, ep, bn=bn, grid=1024, dp=0,
                                                    split=S, ws=sk_ws, bm=bm, out_numel=n))
            tested += 1
    assert tested > 0
    assert int(sk_ws.counters.abs().sum()) == 0


@pytest.mark.parametrize("bm", [128, 256])
def test_gemm_sk_partial_bn192(bm, sk_ws):
    """EPI_PARTIAL at bn = 192: 2048 = 10 x 192 + 128, so every split ends in a partial column tile."""
    h = hip()
    tested = 0
    for M in X.GEMM_ROWS["gemm_sk"]:
        p = X.case(("linear", M, X.N_PARTIAL, 512), DEV)
        assert p.N % 192
        for S in (2, 3, 8):
            if -(-M // bm) * -(-p.N // 192) * S > 1024:
                continue
            _check_partials(h, p, S, f"gemm_sk partial bm {bm} bn 192 M {M} split {S}",
                            lambda ep, n: h.gemm_sk(p.a, p.W.wp, M, p.N, p.K, h.EPI_PARTIAL, ep, bn=192, grid=1024, dp=0,
                                                    split=S, ws=sk_ws, bm=bm, out_numel=n))
            tested += 1
    assert tested > 0
    assert int(sk_ws.counters.abs().sum()) == 0


@pytest.mark.parametrize("bn", [128, 192, 256])
def test_gemm_wr(bn):
    """gemm_wr.hip in the forms it has (store, QKV with RoPE, SwiGLU at bn 128 / 256; no bias, no
    residual), K = 320 (a multiple of 64 but not of 128) among them."""
    h = hip()
    tested = Counter()
    for M in X.GEMM_ROWS["gemm_wr"]:
        for K in X.K_WR:
            tested += gemm_suite(h, l_wr(h, bn), M, K, f"gemm_wr bn {bn}", resid=False, bias=False, swiglu=bn != 192)
    require(tested, GEMM_KINDS + (("swiglu",) if bn != 192 else ()), bn)


@pytest.mark.parametrize("fam", ["gemm", "gemm_sk", "gemm_wr"])
def test_gemm_default_dispatch(fam, sk_ws):
    """hip.gemm's own route (gemm_wr / gemm_sk by the route table and the planner)."""
    h = hip()

    def launch(x, w, M, N, K, epi, ep, ar, norm):
        h.gemm(x, w.wp, M, N, K, epi, ep, sk_ws=sk_ws)
    tested = Counter()
    for M in X.GEMM_ROWS[fam]:
        tested += gemm_suite(h, launch, M, 1216, "gemm dispatch") + gemm_suite(h, launch, M, 256, "gemm dispatch")
    require(tested, GEMM_KINDS + ("swiglu",), fam)
    assert int(sk_ws.counters.abs().sum()) == 0


# ------------------------------------------------------------------------------ further checks
def test_row_ss():
    h = hip()
    x = X.case(("linear", 50, X.N_LIN, 768), DEV).exp["resid"]              # an integer matrix
    sbuf, ss = C.guarded(x.shape[0], x.shape[1] // 64, torch.float32, DEV, guard_cols=0)
    h.row_ss(x, x.shape[0], ss)
    torch.cuda.synchronize()
    C.assert_footprint(sbuf, ss, what="row_ss")
    X.assert_bits_equal(ss.contiguous(), X.expected_ss(x), "row_ss")


HALF_EPS = 3.0  # mean(x^2) + eps = 4 exactly, so the RMSNorm factor is exactly 1 / 2


@pytest.mark.parametrize("family", ["gemv", "coop", "fp8", "coop_fp8"])
def test_fused_rmsnorm(family, coop_ws):
    """norm=True with +-1 activations: mean(x^2) is exactly 1 and the norm weight is an unfolded 1.

    eps = 1e-5: the expected output is bf16_rne(float32(y) * float32(1 / sqrt(1 + eps))), and the
    kernel may differ from it by at most one bf16 ulp per element (the fp32 rsqrt and multiply are
    good to a few 2^-23, far inside bf16's 2^-9 half-ulp, so a difference can appear only on a
    rounding boundary). The share of elements that differ is printed, not gated. Every y here is a
    bf16 value and the factor moves it by 5e-6, so this form pins a wrong divisor or a gross rsqrt
    error only: a kernel that left the norm out would pass it.

    eps = 3: the factor is 1 / sqrt(4) = 1 / 2, y / 2 is again a bf16 value, and an rsqrt that is
    off by a few 2^-23 still rounds to it: the output is y / 2 bitwise. This is the launch that
    shows the norm is applied, with the row's own sum of squares, K and eps."""
    h = hip()
    fp8 = family.endswith("fp8")
    rows = (1, 7, 16, 50) if family in ("gemv", "fp8") else (17, 50, 128)

    def launch(c, M, ep, eps):
        if family == "fp8":
            h.gemv_fp8(c.a, c.W.wq, c.W.sc, M, c.N, c.K, h.EPI_STORE, ep, norm=True, eps=eps)
        elif family == "coop_fp8":
            assert packing.fp8_proj_config(c.N // 16, M, k=c.K)[0] == "coop_fp8"
            h.proj_fp8(c.a, c.W.wq, c.W.sc, M, c.N, c.K, h.EPI_STORE, ep, norm=True, eps=eps, ws=coop_ws)
        elif family == "gemv" and M > 16:  # the streaming kernel at 4 row blocks
            h.gemv(c.a, c.W.wp, M, c.N, c.K, h.EPI_STORE, ep, norm=True, eps=eps, tn=2, nw=4, u=2)
        else:
            assert packing.proj_config(c.N // 16, M, k=c.K)[0] == ("coop" if family == "coop" else "gemv")
            h.gemv(c.a, c.W.wp, M, c.N, c.K, h.EPI_STORE, ep, norm=True, eps=eps, ws=coop_ws)

    tested = 0
    for M in rows:
        c = X.case(("linear_fp8" if fp8 else "linear", M, X.N_LIN, X.K_EPI), DEV)
        obuf, out = C.guarded(M, c.N, device=DEV)
        launch(c, M, h.make_epi(out=out, ldo=out.stride(0)), EPS)
        torch.cuda.synchronize()
        C.assert_footprint(obuf, out, what=f"{family} norm M {M}")
        share = X.assert_within_one_ulp(out, X.norm_expected(c.y, EPS), f"{family} fused norm M {M}")
        print(f"fused RMSNorm {family} M={M}: {share:.4%} of {out.numel()} elements differ from the reference (by one bf16 ulp)")
        C.sentinel_fill(obuf)
        launch(c, M, h.make_epi(out=out, ldo=out.stride(0)), HALF_EPS)
        torch.cuda.synchronize()
        C.assert_footprint(obuf, out, what=f"{family} norm eps {HALF_EPS} M {M}")
        assert bool(X.is_bf16(c.y / 2).all())
        X.assert_bits_equal(out, X.bf16_rne(c.y / 2), f"{family} fused norm eps {HALF_EPS} M {M}", unit=c.unit / 2)
        tested += 2
    assert tested > 0
    assert int(coop_ws.counters.abs().sum()) == 0


def test_graph_replay(coop_ws, sk_ws):
    """One coop split-K residual launch and one gemm_sk stream-K launch, each captured in a graph
    and replayed three times: the exact_int bits on every replay, the counters zero afterwards."""
    h = hip()
    c = X.case(("linear", 50, X.N_LIN, 768), DEV)
    cand = max((x for x in packing.coop_candidates(c.N // 16, c.K, c.M) if x[3] >= 2 and x[4] == 1), key=lambda x: x[3])
    g = X.case(("linear", 300, X.N_LIN, 1216), DEV)
    jobs = [(c, "coop", lambda ep: h.gemv(c.a, c.W.wp, c.M, c.N, c.K, h.EPI_RESID, ep, coop=cand, ws=coop_ws)),
            (g, "gemm_sk", lambda ep: h.gemm_sk(g.a, g.W.wp, g.M, g.N, g.K, h.EPI_RESID, ep, bn=256, grid=37, dp=0, split=0,
                                                ws=sk_ws, bm=256))]
    tested = 0
    for case, name, launch in jobs:
        obuf, out = C.guarded(case.M, case.N, device=DEV)
        ep = h.make_epi(out=out, resid=case.resid, ldo=out.stride(0), ldr=case.N)
        launch(ep)  # once eagerly: workspaces and modules are set up outside the capture
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            launch(ep)
        for i in range(3):
            C.sentinel_fill(obuf)
            graph.replay()
            torch.cuda.synchronize()
            C.assert_footprint(obuf, out, what=f"{name} replay {i}")
            X.assert_bits_equal(out, case.exp["resid"], f"{name} replay {i}", unit=case.unit)
            tested += 1
    assert tested == 6
    assert int(coop_ws.counters.abs().sum()) == 0 and int(sk_ws.counters.abs().sum()) == 0


@pytest.mark.parametrize("M", [1, 7])
def test_padded_lm_head(M):
    """The engine pads the lm_head with copies of row 0 behind a -3e38 bias: with the maximum at
    token 0 every padded row ties with it before the bias, and token 0 must win."""
    h = hip()
    c = X.case(("padded_head", M), DEV)
    keys = torch.zeros(M, dtype=torch.int64, device=DEV)
    tok = torch.empty(M, dtype=torch.int32, device=DEV)
    tested = 0
    for tn, nw, u in [(0, 0, 0)] + packing.gemv_candidates(c.N // 16, c.K, M)[:3]:
        h.gemv(c.a, c.W.wp, M, c.N, c.K, h.EPI_ARGMAX, h.make_epi(keys=keys, bias=c.bias), tn=tn, nw=nw, u=u)
        h.argmax_finalize(keys, M, tok)
        torch.cuda.synchronize()
        X.assert_tokens(tok, c, f"{c.tag} gemv {(tn, nw, u)}")
        tested += 1
    assert tested > 0
