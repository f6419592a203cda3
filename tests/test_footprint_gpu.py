"""Write and read footprints of every kernel with an output (tests/contract_cases.py).

Every output is a window inside a sentinel-filled buffer with guard rows (one full largest row
tile) and guard columns (ld = N + 64): after the launch every element outside the window is
still the bit-identical sentinel and every element inside is not, and the window agrees with the
fp32 reference at the tolerance of the matching numerics test. Every operand carries NaN where
the kernel has no business reading: A rows >= M and columns >= K (ldx = K + 64), the padding of
resid and bias, the rows that the tail of a longer ``a_rows`` points at. The KV caches are
sentinel-filled views with guard bands: an EPI_QKV launch writes exactly the cells
(slot[m], head, pos[m], :) for m < M - not a row >= M through the longer slot / pos arrays, not
one position late, nothing for a position outside [0, t_max).

Any index a wrong kernel could misuse still lands in the test's own allocations, so a wrong
kernel gives an assertion and never a fault. (The attention kernels' output windows, split
workspaces and counters are checked in tests/test_attn_membership_gpu.py.)"""
import pytest
import torch
import torch.nn.functional as F

import contract_cases as C
from llm_sharding_amd.ops import packing
from llm_sharding_amd.utils.numerics import rel_err  # global + per-16x16-tile + per-row

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-5
DECODE_ROWS = [1, 15, 16, 17, 63, 64, 65, 127, 128]
GEMM_ROWS = [1, 129, 255, 256, 257, 300]


def hip():
    from llm_sharding_amd.ops import hip as h
    h.lib()
    return h


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _rnd(*shape, scale=1.0, gen=None):
    return (torch.randn(*shape, device=DEV, generator=gen) * scale).to(torch.bfloat16)


class W:
    """A weight in every form the families take: fp32 reference values, pack_b bf16, packed fp8."""

    def __init__(self, w, fp8=False):
        if fp8:
            q, self.sc = packing.quantize_fp8_rows(w)
            self.ref = packing.dequantize_fp8_rows(q, self.sc)  # exactly what the kernel multiplies by
            self.wq = packing.pack_b_fp8(q).view(-1)
            self.wp = None
        else:
            self.ref, self.wp, self.wq, self.sc = w.float(), packing.pack_b(w), None, None


def _bias(N, gen):
    """fp32 [N] bias inside a NaN buffer (contiguous, 16-byte aligned)."""
    buf, win = C.guarded_flat(N, torch.float32, DEV, guard=64)
    win.copy_(torch.randn(N, device=DEV, generator=gen) * 0.5)
    return win


def _activations(M, K, gen, a_rows):
    """(x, a_rows, effective rows): x has NaN rows beyond its own and NaN columns beyond K;
    with ``a_rows`` the index array is longer than M and its tail points at NaN rows."""
    if not a_rows:
        xbuf, x = C.operand(M, K, DEV, gen=gen)
        return x, None, x
    R = M + 5
    xbuf, x = C.operand(R, K, DEV, gen=gen)
    idx = torch.randint(0, R, (M,), device=DEV, generator=gen)
    tail = R + torch.arange(8, device=DEV)  # NaN guard rows below the window, inside the allocation
    return x, torch.cat([idx, tail]).to(torch.int32), x[idx]


def _norm(xr, norm):
    xf = xr.float()
    return xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + EPS) if norm else xf


def run_epi(h, launch, kind, M, N, K, seed, fp8=False, a_rows=False, norm=False, bias=False, what=""):
    """One launch of ``launch(x, W, M, N, K, epi, ep, a_rows, norm)`` with epilogue ``kind``
    (N = the GEMM's column count), every buffer guarded; asserts footprint and numerics."""
    g = _gen(seed)
    x, ar, xr = _activations(M, K, g, a_rows)
    xn = _norm(xr, norm)
    b = _bias(N, g) if bias else None
    tag = f"{what} {kind} M={M} N={N} K={K}"
    if kind == "swiglu":
        I = N // 2
        wg, wu = _rnd(I, K, scale=0.05, gen=g), _rnd(I, K, scale=0.05, gen=g)
        w = W(packing.fuse_gate_up(wg, wu), fp8)
        obuf, out = C.guarded(M, I, device=DEV)
        launch(x, w, M, N, K, h.EPI_SWIGLU, h.make_epi(out=out, ldo=out.stride(0)), ar, norm)
        gu = (xn @ w.ref.T).view(M, I // 16, 2, 16)
        ref, tol = (F.silu(gu[:, :, 0]) * gu[:, :, 1]).reshape(M, I), 1e-2
    else:
        w = W(_rnd(N, K, scale=0.02, gen=g), fp8)
        obuf, out = C.guarded(M, N, device=DEV)
        ref, tol = xn @ w.ref.T, 8e-3
        if bias:
            ref = ref + b
        if kind == "store":
            launch(x, w, M, N, K, h.EPI_STORE, h.make_epi(out=out, ldo=out.stride(0), bias=b), ar, norm)
        else:
            rbuf, resid = C.operand(M, N, DEV, gen=g)  # its own NaN padding, ldr = N + 64
            ep = h.make_epi(out=out, resid=resid, ldo=out.stride(0), ldr=resid.stride(0), bias=b)
            launch(x, w, M, N, K, h.EPI_RESID, ep, ar, norm)
            ref = resid.float() + ref
    torch.cuda.synchronize()
    C.assert_footprint(obuf, out, what=tag)
    assert bool(torch.isfinite(out.float()).all()), tag + ": NaN padding of an operand reached the output"
    err = rel_err(out, ref)
    assert err < tol, (tag, err)


def run_argmax(h, launch, M, V, K, seed, fp8=False, a_rows=True, what=""):
    """EPI_ARGMAX with a keys array longer than M (the tail must not change), then
    argmax_finalize into guarded token / position arrays."""
    g = _gen(seed)
    x, ar, xr = _activations(M, K, g, a_rows)
    w = W(_rnd(V, K, scale=0.02, gen=g), fp8)
    kbuf, keys = C.guarded_flat(M, torch.int64, DEV, guard=64)
    keys.zero_()
    launch(x, w, M, V, K, h.EPI_ARGMAX, h.make_epi(keys=keys), ar, False)
    torch.cuda.synchronize()
    C.assert_footprint(kbuf, keys, what=what + " argmax keys")
    assert bool((keys != 0).all())
    tbuf, tok = C.guarded_flat(M, torch.int32, DEV, guard=64)
    h.argmax_finalize(keys, M, tok)
    torch.cuda.synchronize()
    C.assert_footprint(tbuf, tok, what=what + " tokens")
    C.assert_footprint(kbuf, keys, what=what + " keys after finalize")
    assert bool((keys == 0).all())  # finalize resets the keys
    logits = xr.float() @ w.ref.T
    assert bool(((tok >= 0) & (tok < V)).all())
    chosen = logits.gather(1, tok.long()[:, None])[:, 0]
    assert bool(torch.all(logits.max(-1).values - chosen < 2e-2 * logits.abs().max())), what


# ------------------------------------------------------------------------------ launchers
def l_gemv(h, **kw):
    def f(x, w, M, N, K, epi, ep, ar, norm):
        h.gemv(x, w.wp, M, N, K, epi, ep, norm=norm, eps=EPS, a_rows=ar, **kw)
    return f


def l_fp8(h, cfg=None):
    def f(x, w, M, N, K, epi, ep, ar, norm):
        h.gemv_fp8(x, w.wq, w.sc, M, N, K, epi, ep, norm=norm, eps=EPS, a_rows=ar, cfg=cfg)
    return f


def l_proj_fp8(h, algo=None, ws=None):
    def f(x, w, M, N, K, epi, ep, ar, norm):
        h.proj_fp8(x, w.wq, w.sc, M, N, K, epi, ep, norm=norm, eps=EPS, a_rows=ar, algo=algo, ws=ws)
    return f


def l_legacy(h):
    def f(x, w, M, N, K, epi, ep, ar, norm):
        assert ar is None and not norm
        h.gemm(x, w.wp, M, N, K, epi, ep, legacy=True)
    return f


def l_sk(h, ws, bm, bn, grid, dp, split):
    def f(x, w, M, N, K, epi, ep, ar, norm):
        assert ar is None and not norm
        h.gemm_sk(x, w.wp, M, N, K, epi, ep, bn=bn, grid=grid, dp=dp, split=split, ws=ws, bm=bm)
    return f


def l_wr(h, bn):
    def f(x, w, M, N, K, epi, ep, ar, norm):
        assert ar is None and not norm
        h.gemm_wr(x, w.wp, M, N, K, epi, ep, bn=bn)
    return f


@pytest.fixture(scope="module")
def sk_ws():
    return hip().SkWorkspace(DEV, grid=256, bn=256)


# (grid, dp, split) for gemm_sk at <= 18 tiles: every tile whole (one K range), two equal K
# splits per tile, and stream-K over 37 workgroups (tiles cut at arbitrary K steps)
SK_PLANS = [(256, 1, 1), (256, 1, 2), (37, 0, 0)]


# ------------------------------------------------------------------------------ decode GEMV
@pytest.mark.parametrize("kind", ["store", "resid", "swiglu", "argmax"])
@pytest.mark.parametrize("M", DECODE_ROWS)
def test_gemv_default_dispatch(M, kind):
    """hip.gemv's own choice (streaming GEMV up to 16 rows, cooperative split-K above) at every
    edge row count, with and without a longer a_rows array."""
    h = hip()
    ws = h.CoopWorkspace(DEV, slab_floats=1 << 22, groups=1 << 10)
    tested = 0
    for ar in (False, True):
        if kind == "argmax":
            run_argmax(h, l_gemv(h, ws=ws), M, 512, 256, seed=M, a_rows=ar, what="gemv")
        else:
            N, K = (1024, 256) if kind == "swiglu" else (512, 768 if M % 2 else 256)
            run_epi(h, l_gemv(h, ws=ws), kind, M, N, K, seed=M, a_rows=ar, norm=(kind == "resid"),
                    bias=ar and kind != "swiglu", what="gemv")
        tested += 1
    assert tested > 0
    assert int(ws.counters.abs().sum()) == 0


@pytest.mark.parametrize("cfg", packing.GEMV_CONFIGS)
def test_gemv_every_config(cfg):
    h = hip()
    tn, mb, nw, u = cfg
    M, N = {1: 7, 2: 29, 4: 50}[mb], 256  # the rows of test_kernels_gpu.test_gemv_every_config
    tested = 0
    for K in (256, 768):
        if (K // 32) % u:
            continue
        run_epi(h, l_gemv(h, tn=tn, nw=nw, u=u), "store", M, N, K, seed=K, a_rows=True, what=f"gemv {cfg}")
        tested += 1
    assert tested > 0, cfg


def _coop_pick(cands, key):
    """The candidate of one instantiated config with the most K splits."""
    c = [c for c in cands if key(c) and c[3] >= 1]
    return max(c, key=lambda c: c[3]) if c else None


@pytest.mark.parametrize("cfg", packing.COOP_CONFIGS)
def test_coop_every_config(cfg):
    """Every instantiated cooperative config at one legal split (the largest), fused RMSNorm +
    residual; the workspace counters are all zero afterwards."""
    h = hip()
    mb, tnw, nw, kf, kw, d = cfg
    M, N = {2: 29, 4: 50, 8: 100}[mb], 16 * tnw * nw * 3
    ws = h.CoopWorkspace(DEV, slab_floats=1 << 22, groups=1 << 10)
    tested = 0
    for K in (1216, 512):  # 38 / 16 chunks of 32: uneven over the splits where kf allows it
        c = _coop_pick(packing.coop_candidates(N // 16, K, M), lambda c: c[:3] == (tnw, nw, kf) and c[4:] == (kw, d))
        if c is None:
            continue
        run_epi(h, l_gemv(h, coop=c, ws=ws), "resid", M, N, K, seed=K, a_rows=True, norm=True, what=f"coop {c}")
        tested += 1
    assert tested > 0, cfg
    assert int(ws.counters.abs().sum()) == 0


def test_coop_ragged_and_partial():
    """The ragged mode (sk = 0: tiles dealt to one workgroup per CU) and EPI_PARTIAL, whose fp32
    partial buffer [sk][M][ldo] is written in full and not beyond."""
    h = hip()
    ws = h.CoopWorkspace(DEV, slab_floats=1 << 22, groups=1 << 10)
    M, N, K = 40, 4800, 256
    ragged = [c for c in packing.coop_candidates(N // 16, K, M) if c[3] == 0][:1]
    assert len(ragged) > 0
    for c in ragged:
        run_epi(h, l_gemv(h, coop=c, ws=ws), "resid", M, N, K, seed=3, a_rows=True, norm=True, what=f"coop ragged {c}")
    M, N, K = 40, 512, 512
    g = _gen(11)
    x, ar, xr = _activations(M, K, g, True)
    w = W(_rnd(N, K, scale=0.02, gen=g))
    tested = 0
    for c in packing.coop_candidates(N // 16, K, M):
        if not 2 <= c[3] <= 8 or tested >= 3:
            continue
        pbuf, P = C.guarded_flat(c[3] * M * N, torch.float32, DEV)
        h.gemv(x, w.wp, M, N, K, h.EPI_PARTIAL, h.make_epi(out=P, ldo=N), a_rows=ar, coop=c, ws=ws, out_numel=P.numel())
        torch.cuda.synchronize()
        C.assert_footprint(pbuf, P, what=f"coop partial {c}")
        assert rel_err(P.view(c[3], M, N).sum(0), xr.float() @ w.ref.T) < 8e-3, c
        tested += 1
    assert tested > 0
    assert int(ws.counters.abs().sum()) == 0


@pytest.mark.parametrize("cfg", packing.FP8_CONFIGS)
def test_gemv_fp8_every_config(cfg):
    h = hip()
    tn, mb, nw, u2 = cfg
    M, N, K = {1: 7, 2: 29, 4: 50}[mb], 16 * tn * 6, 64 * 2 * u2 * 3
    assert (K // 32) % (2 * u2) == 0
    run_epi(h, l_fp8(h, (tn, nw, u2)), "resid", M, N, K, seed=K, fp8=True, a_rows=True, norm=True, what=f"fp8 {cfg}")


@pytest.mark.parametrize("cfg", packing.COOP_FP8_CONFIGS)
def test_coop_fp8_every_config(cfg):
    h = hip()
    mb, tnw, nw, kf = cfg
    M, N, K = {2: 29, 4: 50, 8: 100}[mb], 16 * tnw * nw * 3, 64 * kf * 3
    ws = h.CoopWorkspace(DEV, slab_floats=1 << 22, groups=1 << 10)
    c = _coop_pick(packing.coop_fp8_candidates(N // 16, K, M), lambda c: c[:3] == (tnw, nw, kf))
    assert c is not None, cfg
    run_epi(h, l_proj_fp8(h, ("coop_fp8", c), ws), "resid", M, N, K, seed=K, fp8=True, a_rows=True, norm=True,
            what=f"coop_fp8 {c}")
    assert int(ws.counters.abs().sum()) == 0


# ------------------------------------------------------------------------------ GEMMs
@pytest.mark.parametrize("kind", ["store", "resid", "swiglu"])
def test_gemm_legacy(kind):
    h = hip()
    tested = 0
    for M in GEMM_ROWS:
        N, K = (768, 512) if kind == "swiglu" else ((384, 256) if M % 2 else (320, 1216))  # 320: tn = 1
        run_epi(h, l_legacy(h), kind, M, N, K, seed=M, bias=kind != "swiglu" and M % 2 == 0, what="gemm legacy")
        tested += 1
    assert tested > 0
    assert int(h.default_workspace().counters.abs().sum()) == 0


@pytest.mark.parametrize("kind", ["store", "resid", "swiglu"])
@pytest.mark.parametrize("bn", [128, 192, 256])
@pytest.mark.parametrize("bm", [128, 256])
def test_gemm_sk(bm, bn, kind, sk_ws):
    """Whole-tile, equal-split and stream-K plans at every edge row count."""
    h = hip()
    tested = 0
    for M in GEMM_ROWS:
        for (grid, dp, split) in SK_PLANS:
            N, K = 768, (1216 if M % 2 else 256)
            assert -(-M // bm) * (N // bn) * max(split, 1) <= grid or split == 0
            run_epi(h, l_sk(h, sk_ws, bm, bn, grid, dp, split), kind, M, N, K, seed=M + grid,
                    bias=kind != "swiglu" and M % 2 == 0, what=f"gemm_sk bm {bm} bn {bn} plan {(grid, dp, split)}")
            tested += 1
    assert tested > 0
    assert int(sk_ws.counters.abs().sum()) == 0


@pytest.mark.parametrize("bn", [128, 256])  # (ss_out has no 192-wide form: lsa_gemm_sk refuses it)
@pytest.mark.parametrize("bm", [128, 256])
def test_gemm_sk_resid_ss_out_and_partial(bm, bn, sk_ws):
    """EPI_RESID with the fused-norm partial sums (ss rows >= M untouched) and EPI_PARTIAL (the
    fp32 buffer written for exactly split x M x ldo values)."""
    h = hip()
    N, K = 768, 256
    tested = 0
    for M in (129, 256, 300):
        for (grid, dp, split) in SK_PLANS:
            g = _gen(M + grid)
            xbuf, x = C.operand(M, K, DEV, gen=g)
            w = W(_rnd(N, K, scale=0.02, gen=g))
            rbuf, resid = C.operand(M, N, DEV, gen=g)
            obuf, out = C.guarded(M, N, device=DEV)
            sbuf, ss = C.guarded(M, N // 64, torch.float32, DEV, guard_cols=0)
            ep = h.make_epi(out=out, resid=resid, ldo=out.stride(0), ldr=resid.stride(0), ss_out=ss)
            h.gemm_sk(x, w.wp, M, N, K, h.EPI_RESID, ep, bn=bn, grid=grid, dp=dp, split=split, ws=sk_ws, bm=bm)
            torch.cuda.synchronize()
            tag = f"gemm_sk ss_out bm {bm} bn {bn} M {M} plan {(grid, dp, split)}"
            C.assert_footprint(obuf, out, what=tag)
            C.assert_footprint(sbuf, ss, what=tag + " ss")
            assert rel_err(out, resid.float() + x.float() @ w.ref.T) < 8e-3, tag
            assert rel_err(ss, out.float().pow(2).view(M, N // 64, 64).sum(-1)) < 1e-5, tag
            tested += 1
        S = 2
        pbuf, P = C.guarded_flat(S * M * N, torch.float32, DEV)
        h.gemm_sk(x, w.wp, M, N, K, h.EPI_PARTIAL, h.make_epi(out=P, ldo=N), bn=bn, grid=256, dp=0, split=S, ws=sk_ws,
                  bm=bm, out_numel=P.numel())
        torch.cuda.synchronize()
        C.assert_footprint(pbuf, P, what=f"gemm_sk partial bm {bm} bn {bn} M {M}")
        assert rel_err(P.view(S, M, N).sum(0), x.float() @ w.ref.T) < 1e-5
        tested += 1
    assert tested > 0
    assert int(sk_ws.counters.abs().sum()) == 0


# (SwiGLU at bn 192 is left out: hip.gemm_wr needs whole gate / up pairs per wave, bn 128 / 256;
# gemm_wr takes no bias)
@pytest.mark.parametrize("bn,kind", [(128, "store"), (192, "store"), (256, "store"), (128, "swiglu"), (256, "swiglu")])
def test_gemm_wr(bn, kind):
    h = hip()
    tested = 0
    for M in (193, 256, 300):
        run_epi(h, l_wr(h, bn), kind, M, 768, 320 if M % 2 else 256, seed=M, what=f"gemm_wr bn {bn}")
        tested += 1
    assert tested > 0


# ------------------------------------------------------------------------------ KV append
NH, NKV, HD, H_IN, SLOTS, T_MAX = 8, 2, 64, 256, 4, 300
QKV_N = (NH + 2 * NKV) * HD  # 768: tiles by 128, 192 and 256


def _rope_ref(t, pos, cos, sin):
    half = t.shape[-1] // 2
    c, s = cos[pos][:, None, :], sin[pos][:, None, :]
    t1, t2 = t[..., :half], t[..., half:]
    return torch.cat([t1 * c - t2 * s, t2 * c + t1 * s], dim=-1)


def _rope_tables():
    """cos / sin with 8 rows before and 64 rows after the [0, T_MAX) range (views into a longer
    table), so the out-of-range positions of the bad-pos case index inside the allocation."""
    from llm_sharding_amd.config import tiny
    from llm_sharding_amd.models.rope import rope_table
    cos, sin = rope_table(tiny(head_dim=HD), T_MAX + 72, DEV)
    return cos[8:], sin[8:]


def run_qkv(h, launch, M, seed, rope, bias=False, fp8=False, bad_pos=False, what=""):
    """EPI_QKV into sentinel-filled caches: slot / pos arrays longer than M whose tail points at
    valid, otherwise unused cells. ``bad_pos``: three rows get pos -1, t_max and t_max + 5; their
    K/V are written nowhere, the other rows are unaffected."""
    g = _gen(seed)
    xbuf, x = C.operand(M, H_IN, DEV, gen=g)
    wq, wk, wv = (_rnd(n * HD, H_IN, scale=0.05, gen=g) for n in (NH, NKV, NKV))
    fused = packing.fuse_qkv(wq, wk, wv, NH, NKV, HD) if rope else torch.cat([wq, wk, wv])
    w = W(fused, fp8)
    if fp8:  # the reference multiplies by the dequantised rows, un-permuted
        full = w.ref
        if rope:
            inv_q = torch.argsort(packing.rope_rows_perm(NH, HD)).to(DEV)
            inv_k = torch.argsort(packing.rope_rows_perm(NKV, HD)).to(DEV)
            rq, rk = full[:NH * HD][inv_q], full[NH * HD:(NH + NKV) * HD][inv_k]
        else:
            rq, rk = full[:NH * HD], full[NH * HD:(NH + NKV) * HD]
        rv = full[(NH + NKV) * HD:]
    else:
        rq, rk, rv = wq.float(), wk.float(), wv.float()
    cells = torch.randperm(SLOTS * T_MAX, device=DEV, generator=g)[:M + 8]  # distinct (slot, pos) cells
    slot, pos = (cells // T_MAX).to(torch.int32), (cells % T_MAX).to(torch.int32)
    ok = torch.ones(M, dtype=torch.bool, device=DEV)
    if bad_pos:
        for m, p in zip((1 % M, M // 2, M - 1), (-1, T_MAX, T_MAX + 5)):
            pos[m], ok[m] = p, False
    b = _bias(QKV_N, g) if bias else None
    cos, sin = _rope_tables() if rope else (None, None)
    qbuf, q = C.guarded(M, NH * HD, device=DEV)
    kflat, kc = C.guarded_cache(SLOTS, NKV, T_MAX, HD, DEV)
    vflat, vc = C.guarded_cache(SLOTS, NKV, T_MAX, HD, DEV)
    ep = h.make_epi(out=q, k_cache=kc, v_cache=vc, slot=slot, pos=pos, cos=cos, sin=sin, ldo=q.stride(0), n_heads=NH,
                    n_kv=NKV, head_dim=HD, t_max=T_MAX, bias=b)
    launch(x, w, M, QKV_N, H_IN, h.EPI_QKV, ep, None, False)
    torch.cuda.synchronize()
    tag = f"{what} qkv M={M} rope={rope} bias={bias} bad_pos={bad_pos}"
    sl, pl = slot[:M][ok].long(), pos[:M][ok].long()
    C.assert_cache_footprint(kflat, kc, sl, pl, what=tag + " k_cache")
    C.assert_cache_footprint(vflat, vc, sl, pl, what=tag + " v_cache")
    # q: rows with a bad position may or may not be written (nothing is asserted about them)
    C.assert_footprint(qbuf, q, optional=(~ok)[:, None].expand(M, NH * HD), what=tag + " q")
    xf = x.float()[ok]
    z = [xf @ r.T for r in (rq, rk, rv)]
    if bias:
        z = [z[0] + b[:NH * HD], z[1] + b[NH * HD:(NH + NKV) * HD], z[2] + b[(NH + NKV) * HD:]]
    n = int(ok.sum())
    zq, zk, zv = z[0].view(n, NH, HD), z[1].view(n, NKV, HD), z[2].view(n, NKV, HD)
    if rope:
        zq, zk = _rope_ref(zq, pl, cos, sin), _rope_ref(zk, pl, cos, sin)
    assert bool(torch.isfinite(q[ok].float()).all()), tag
    assert rel_err(q[ok], zq.reshape(n, -1)) < 1e-2, tag
    assert rel_err(kc[sl, :, pl], zk) < 1e-2, tag
    assert rel_err(vc[sl, :, pl], zv) < 1e-2, tag


def _qkv_families(h, sk_ws):
    """(name, launcher, rows, fp8, takes a bias)."""
    ws = h.CoopWorkspace(DEV, slab_floats=1 << 22, groups=1 << 10)
    fams = [("gemv", l_gemv(h, ws=ws), (1, 5, 16), False, True),
            ("coop", l_gemv(h, ws=ws), (17, 40, 128), False, True),
            ("fp8", l_fp8(h), (7, 50), True, True),
            ("coop_fp8", l_proj_fp8(h, None, ws), (29, 100), True, True),
            ("gemm_legacy", l_legacy(h), (150, 257), False, True),
            ("gemm_sk_128", l_sk(h, sk_ws, 128, 128, 256, 1, 2), (129, 300), False, True),
            ("gemm_sk_256", l_sk(h, sk_ws, 256, 256, 37, 0, 0), (300,), False, True),
            ("gemm_sk_192", l_sk(h, sk_ws, 256, 192, 256, 1, 1), (257,), False, True),
            # gemm_wr takes no bias epilogue (hip.gemm_wr_plan routes a bias to gemm_sk)
            ("gemm_wr_128", l_wr(h, 128), (193,), False, False),
            ("gemm_wr_192", l_wr(h, 192), (300,), False, False),
            ("gemm_wr_256", l_wr(h, 256), (256,), False, False)]
    return ws, fams


FAMILIES = ["gemv", "coop", "fp8", "coop_fp8", "gemm_legacy", "gemm_sk_128", "gemm_sk_256", "gemm_sk_192",
            "gemm_wr_128", "gemm_wr_192", "gemm_wr_256"]


@pytest.mark.parametrize("family", FAMILIES)
def test_kv_append_footprint(family, sk_ws):
    h = hip()
    ws, fams = _qkv_families(h, sk_ws)
    name, launch, rows, fp8, takes_bias = next(f for f in fams if f[0] == family)
    if name == "coop":  # the cooperative kernel, whatever the tuning table says about the shape
        assert all(packing.proj_config(QKV_N // 16, M, k=H_IN)[0] == "coop" for M in rows)
    if name == "coop_fp8":
        assert all(packing.fp8_proj_config(QKV_N // 16, M, k=H_IN)[0] == "coop_fp8" for M in rows)
    tested = 0
    for M in rows:
        run_qkv(h, launch, M, seed=M, rope=True, fp8=fp8, what=name)
        tested += 1
        if takes_bias:
            run_qkv(h, launch, M, seed=M + 1, rope=False, bias=True, fp8=fp8, what=name)
            tested += 1
    M = rows[-1] if rows[-1] >= 5 else 5
    run_qkv(h, launch, M, seed=99, rope=True, fp8=fp8, bad_pos=True, what=name)
    tested += 1
    assert tested > 0
    assert int(ws.counters.abs().sum()) == 0 and int(sk_ws.counters.abs().sum()) == 0


# ------------------------------------------------------------------------------ elementwise
def test_embed():
    h = hip()
    V, H, rows = 300, 512, 37
    table = _rnd(V, H, gen=_gen(1))
    ids = torch.randint(0, V, (rows + 8,), device=DEV, dtype=torch.int32)  # the tail: valid ids, not to be used
    obuf, out = C.guarded(rows, H, device=DEV)
    h.embed(ids, table, out, rows)
    torch.cuda.synchronize()
    C.assert_footprint(obuf, out, what="embed")
    assert torch.equal(out, table[ids[:rows].long()])


@pytest.mark.parametrize("H", [2048, 4096, 3072])  # register-resident widths, the generic loop
@pytest.mark.parametrize("weighted", [True, False])
def test_rmsnorm(H, weighted):
    h = hip()
    rows = 37
    g = _gen(H)
    xbuf, x = C.operand(rows, H, DEV, gen=g)
    w = (1 + 0.1 * torch.randn(H, device=DEV, generator=g)).to(torch.bfloat16)
    obuf, out = C.guarded(rows, H, device=DEV)
    h.rmsnorm(x, w if weighted else None, out, rows, EPS, H)
    torch.cuda.synchronize()
    C.assert_footprint(obuf, out, what=f"rmsnorm {H}")
    xf = x.float()
    ref = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + EPS) * (w.float() if weighted else 1.0)
    assert rel_err(out, ref) < 5e-3


@pytest.mark.parametrize("rows,H", [(1, 768), (7, 768), (130, 1024), (3, 1600)])
@pytest.mark.parametrize("with_pos", [False, True])
def test_layernorm(rows, H, with_pos):
    """The in-place position add writes x: its window is guarded too (and x is bit-unchanged
    without the add)."""
    h = hip()
    g = _gen(rows + H)
    xbuf, x = C.operand(rows, H, DEV, scale=3.0, gen=g)
    w, b = _rnd(H, scale=0.2, gen=g) + 1.0, _rnd(H, scale=0.2, gen=g)
    pe = _rnd(64, H, scale=0.3, gen=g) if with_pos else None
    pos = torch.randint(0, 64, (rows + 8,), device=DEV, dtype=torch.int32, generator=g)
    xin = x.clone()
    obuf, out = C.guarded(rows, H, device=DEV)
    h.layernorm(x, out, w, b, rows, EPS, pos_emb=pe, pos=pos if with_pos else None)
    torch.cuda.synchronize()
    C.assert_footprint(obuf, out, what="layernorm out")
    C.assert_footprint(xbuf, x, what="layernorm x")
    xr = (xin.float() + pe[pos[:rows].long()].float()).to(torch.bfloat16) if with_pos else xin
    assert torch.equal(x, xr)
    assert rel_err(out, F.layer_norm(xr.float(), (H,), w.float(), b.float(), EPS)) < 8e-3


@pytest.mark.parametrize("with_out", [True, False])
def test_resid_rmsnorm_partials(with_out):
    """h (in place) and out are guarded; the partial buffer is NaN beyond the S x rows x H
    values the GEMM wrote (a bigger allocation in both leading dims)."""
    h = hip()
    S, rows, H = 3, 37, 2048  # (the kernel is built for H = 2048 * n)
    g = _gen(5)
    hbuf, hw = C.operand(rows, H, DEV, gen=g)
    h0 = hw.clone()
    P = C.sentinel_fill(torch.empty(S + 1, rows + 3, H, dtype=torch.float32, device=DEV))
    vals = torch.randn(S, rows, H, device=DEV, generator=g) * 0.3
    P.view(-1)[:S * rows * H] = vals.view(-1)  # partial k at k * rows * H, as the GEMM lays them out
    obuf, out = C.guarded(rows, H, device=DEV)
    h.resid_rmsnorm_partials(hw, P, S, rows, EPS, out=out if with_out else None)
    torch.cuda.synchronize()
    C.assert_footprint(hbuf, hw, what="resid_rmsnorm_partials h")
    want = h0.float() + vals.sum(0)
    assert rel_err(hw, want) < 8e-3
    if with_out:
        C.assert_footprint(obuf, out, what="resid_rmsnorm_partials out")
        hf = hw.float()
        assert rel_err(out, hf * torch.rsqrt(hf.pow(2).mean(-1, keepdim=True) + EPS)) < 8e-3
    else:
        assert bool(C.is_sentinel(obuf).all())


def test_row_ss():
    h = hip()
    rows, H = 37, 1024
    xbuf, x = C.operand(rows, H, DEV, gen=_gen(9))
    sbuf, ss = C.guarded(rows, H // 64, torch.float32, DEV, guard_cols=0)
    h.row_ss(x, rows, ss)
    torch.cuda.synchronize()
    C.assert_footprint(sbuf, ss, what="row_ss")
    assert rel_err(ss, x.float().pow(2).view(rows, H // 64, 64).sum(-1)) < 1e-5


def test_argmax_finalize_and_pos_advance():
    """tokens, pos and history are longer than ``rows``: their entries >= rows do not change."""
    h = hip()
    rows, H, V = 5, 128, 256
    hid = torch.zeros(rows, H, dtype=torch.bfloat16, device=DEV)
    lm = torch.zeros(V, H, dtype=torch.bfloat16, device=DEV)
    want = [3, 100, 7, 255, 0]
    for r, t in enumerate(want):
        hid[r, r] = 1.0
        lm[t, r] = 1.0
    kbuf, keys = C.guarded_flat(rows, torch.int64, DEV, guard=64)
    keys.zero_()
    h.gemv(hid, packing.pack_b(lm), rows, V, H, h.EPI_ARGMAX, h.make_epi(keys=keys))
    tbuf, tok = C.guarded_flat(rows, torch.int32, DEV, guard=64)
    pbuf, pos = C.guarded_flat(rows, torch.int32, DEV, guard=64)
    pos.zero_()
    hbuf, hist = C.guarded(4, rows, torch.int32, DEV, guard_rows=4)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    h.argmax_finalize(keys, rows, tok, pos, 1, hist, step)
    torch.cuda.synchronize()
    for buf, win, name in ((kbuf, keys, "keys"), (tbuf, tok, "tokens"), (pbuf, pos, "pos")):
        C.assert_footprint(buf, win, what="argmax_finalize " + name)
    C.assert_footprint(hbuf, hist[0:1], what="argmax_finalize history")  # step 0 only
    assert tok.tolist() == want and hist[0].tolist() == want and pos.tolist() == [1] * rows and int(step) == 1
    h.pos_advance(pos, rows, 2)
    torch.cuda.synchronize()
    C.assert_footprint(pbuf, pos, what="pos_advance")
    assert pos.tolist() == [3] * rows
