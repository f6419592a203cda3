"""The W4A8 GEMM (csrc/quant/gemm_mx4.hip) on the GPU: the activation pre-pass against its torch
statement, exact arithmetic for every built config and K split, the same bits as the GEMV, Gaussian
operands through the fused-RMSNorm epilogues, graph replay, the refusals, and an mxfp4 engine at a
200-row prefill and 256 decode rows (LSA_MX4_GEMM=1) with a dequantise kernel that raises."""
import pytest
import torch
import torch.nn.functional as F

import contract_cases as C
import exact_cases as X
import test_footprint_gpu as FP
import test_mx4_gpu as T
from llm_sharding_amd.ops import mx4, packing
from llm_sharding_amd.utils.numerics import rel_err
from test_int4_gpu import ENGINE_TOL, EPS, hip

pytestmark = pytest.mark.gpu
DEV = "cuda"
BN = mx4.MX4_GEMM_CONFIGS[0][0]


def _image(x, M, K):
    """(guarded int32 buffer, A8, EA) of the pre-pass on ``x``."""
    n = sum(mx4.a_image_bytes(M, K))
    buf, win = C.guarded_flat(n // 4, torch.int32, DEV)
    return buf, *mx4.quant_act_mx8(x, M, K, win.view(torch.uint8))


def _gemm(h, x, q, e, M, epi, ep, cfg=None, ws=None):
    N, K = q.shape
    _, a8, ea = _image(x.to(DEV), M, K)
    mx4.gemm_mx4(a8, ea, mx4.pack_b_mx4(q).to(DEV), mx4.pack_scales_mx4(e).to(DEV), M, N, K, epi, ep, cfg=cfg, ws=ws)
    torch.cuda.synchronize()


def _row_ss(h, t):
    ss = torch.zeros(t.shape[0], t.shape[1] // 64, dtype=torch.float32, device=DEV)
    h.row_ss(t, t.shape[0], ss)
    return ss


def _store(h, x, q, e, cfg=None):
    M = x.shape[0]
    obuf, out = C.guarded(M, q.shape[0], device=DEV)
    _gemm(h, x, q, e, M, h.EPI_STORE, h.make_epi(out=out, ldo=out.stride(0)), cfg=cfg)
    C.assert_footprint(obuf, out, what=f"gemm_mx4 store {tuple(x.shape)} x {tuple(q.shape)} cfg {cfg}")
    return out.cpu()


@pytest.mark.parametrize("K", [128, 640])
@pytest.mark.parametrize("M", [1, 17, 129])
def test_prepass_is_pack_a_mx8(M, K):
    hip()
    x = torch.randn(M, K, generator=X.gen(M + K)) * torch.logspace(-2, 2, M)[:, None]
    x[0, :32] = torch.arange(32) * 8 / 128 + 4 / 128              # e4m3 ties, the maximum last
    if M > 3:
        x[1, :32] = torch.arange(32, 0, -1) * 8 / 128 - 4 / 128   # the same, the maximum first
        x[2, 32:64] = 0                                            # an all-zero block
        x[3, 64:96] = torch.arange(32) * 2.0 ** -133               # a block of bf16 subnormals
    x = x.to(torch.bfloat16)
    buf, a8, ea = _image(x.to(DEV), M, K)
    torch.cuda.synchronize()
    wa, we = mx4.pack_a_mx8(x)
    assert torch.equal(a8.cpu(), wa) and torch.equal(ea.cpu(), we)
    assert bool(C.is_sentinel(buf[:4096]).all()) and bool(C.is_sentinel(buf[-4096:]).all())


@pytest.mark.parametrize("K", [128, 640, 4224])  # shorter than the ring; a short last group; nine groups, eight splits
def test_exact_every_config_and_split(K):
    h, N, ties = hip(), 2 * BN, 0
    for M in (1, 128, 129, 257):
        x, q, e, ref = T._exact_case(M, N, K, M + K)
        want = X.bf16_rne(ref)
        ties += int(X.is_tie(ref).sum()) if M >= 128 else 0
        cfgs = mx4.mx4_gemm_candidates(M, N, K)
        assert {sk for _, sk in cfgs} == {s for s in mx4.MX4_GEMM_SPLITS if s <= mx4.scale_groups(K)}
        for cfg in cfgs:
            X.assert_bits_equal(_store(h, x, q, e, cfg=cfg), want, f"gemm_mx4 exact M={M} K={K} cfg {cfg}")
    assert ties > 100


@pytest.mark.parametrize("epi", ["store", "resid"])
def test_same_bits_as_the_gemv(epi):
    h, M, N, K = hip(), 128, 2 * BN, 640
    x, q, e, _ = T._exact_case(M, N, K, 11)
    resid = torch.randint(-8, 9, (M, N), generator=X.gen(3)).to(torch.bfloat16).to(DEV)
    outs = []
    for run in (T._launch, _gemm):
        out = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
        ep = h.make_epi(out=out, ldo=N) if epi == "store" else h.make_epi(out=out, resid=resid, ldo=N, ldr=N)
        run(h, x.to(DEV), q, e, M, h.EPI_STORE if epi == "store" else h.EPI_RESID, ep)
        outs.append(out)
    X.assert_bits_equal(outs[1], outs[0], f"gemm_mx4 vs gemv_mx4 {epi}")


def test_gaussian_resid_ss_out_and_swiglu_ss_in():
    h, M = hip(), 129
    # RESID + ss_out: the sums of squares are those of the kernel's own rounded outputs
    N, K = 256, 384
    g, x, q, e, y, _ = T._gauss(M, N, K, 21)
    resid = torch.randn(M, N, generator=g).to(torch.bfloat16).to(DEV)
    obuf, out = C.guarded(M, N, device=DEV)
    sbuf, ss = C.guarded(M, N // 64, torch.float32, DEV, guard_cols=0)
    _gemm(h, x, q, e, M, h.EPI_RESID, h.make_epi(out=out, resid=resid, ldo=out.stride(0), ldr=N, ss_out=ss))
    C.assert_footprint(obuf, out, what="gemm_mx4 resid")
    C.assert_footprint(sbuf, ss, what="gemm_mx4 ss_out")
    assert rel_err(out.cpu(), (resid.cpu().double() + y).float()) < 8e-3
    X.assert_bits_equal(ss, _row_ss(h, out), "gemm_mx4 ss_out")
    # SWIGLU + ss_in
    N, K = 512, 256
    g, x, q, e, y, rstd = T._gauss(M, N, K, 22, 0.05)
    ssi = _row_ss(h, x.to(DEV))
    obuf, out = C.guarded(M, N // 2, device=DEV)
    _gemm(h, x, q, e, M, h.EPI_SWIGLU, h.make_epi(out=out, ldo=out.stride(0), ss_in=ssi, ss_eps=EPS))
    C.assert_footprint(obuf, out, what="gemm_mx4 swiglu")
    gu = (y * rstd).view(M, N // 32, 2, 16)
    assert rel_err(out.cpu(), (F.silu(gu[:, :, 0]) * gu[:, :, 1]).reshape(M, N // 2).float()) < 1e-2


def test_gaussian_qkv_rope_ss_in():
    h, M = hip(), 129
    NH, NKV, HD, K, SLOTS, T_MAX = FP.NH, FP.NKV, FP.HD, FP.H_IN, FP.SLOTS, FP.T_MAX
    assert (NH + 2 * NKV) * HD % BN == 0 and K % 256 == 0
    g = X.gen(M)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    wq, wk, wv = (torch.randn(n * HD, K, generator=g) * 0.05 for n in (NH, NKV, NKV))
    q4, e4 = mx4.quantize_mx4(packing.fuse_qkv(wq, wk, wv, NH, NKV, HD))
    y = mx4.linear_reference(x, q4, e4) * torch.rsqrt(x.double().pow(2).mean(-1, keepdim=True) + EPS)
    inv_q, inv_k = torch.argsort(packing.rope_rows_perm(NH, HD)), torch.argsort(packing.rope_rows_perm(NKV, HD))
    zq, zk, zv = y[:, :NH * HD][:, inv_q], y[:, NH * HD:(NH + NKV) * HD][:, inv_k], y[:, (NH + NKV) * HD:]
    cells = torch.randperm(SLOTS * T_MAX, generator=g)[:M]
    slot, pos = (cells // T_MAX).to(torch.int32).to(DEV), (cells % T_MAX).to(torch.int32).to(DEV)
    cos, sin = FP._rope_tables()
    qbuf, qo = C.guarded(M, NH * HD, device=DEV)
    kflat, kc = C.guarded_cache(SLOTS, NKV, T_MAX, HD, DEV)
    vflat, vc = C.guarded_cache(SLOTS, NKV, T_MAX, HD, DEV)
    ssi = _row_ss(h, x.to(DEV))
    ep = h.make_epi(out=qo, k_cache=kc, v_cache=vc, slot=slot, pos=pos, cos=cos, sin=sin, ldo=qo.stride(0), n_heads=NH,
                    n_kv=NKV, head_dim=HD, t_max=T_MAX, ss_in=ssi, ss_eps=EPS)
    _gemm(h, x, q4, e4, M, h.EPI_QKV, ep)
    C.assert_footprint(qbuf, qo, what="gemm_mx4 qkv q")
    C.assert_cache_footprint(kflat, kc, slot.long(), pos.long(), what="gemm_mx4 qkv k_cache")
    C.assert_cache_footprint(vflat, vc, slot.long(), pos.long(), what="gemm_mx4 qkv v_cache")
    pl, c64, s64 = pos.long().cpu(), cos.cpu().double(), sin.cpu().double()
    rq, rk = FP._rope_ref(zq.view(M, NH, HD), pl, c64, s64), FP._rope_ref(zk.view(M, NKV, HD), pl, c64, s64)
    assert rel_err(qo.cpu(), rq.reshape(M, -1).float()) < 1e-2
    assert rel_err(kc[slot.long(), :, pos.long()].cpu(), rk.float()) < 1e-2
    assert rel_err(vc[slot.long(), :, pos.long()].cpu(), zv.view(M, NKV, HD).float()) < 1e-2


def test_replay_in_a_captured_graph():
    h, M, N, K = hip(), 257, 2 * BN, 2048
    x, q, e, ref = T._exact_case(M, N, K, 9)
    xd, wq, sc = x.to(DEV), mx4.pack_b_mx4(q).to(DEV), mx4.pack_scales_mx4(e).to(DEV)
    ws = h.CoopWorkspace(DEV, slab_floats=mx4.mx4_gemm_slab_floats(M, N, 4), groups=6)
    scratch = torch.zeros(sum(mx4.a_image_bytes(M, K)), dtype=torch.uint8, device=DEV)
    out = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)

    def run():
        mx4.gemm_mx4(*mx4.quant_act_mx8(xd, M, K, scratch), wq, sc, M, N, K, h.EPI_STORE, h.make_epi(out=out, ldo=N),
                     ws=ws, cfg=(BN, 4))
    run()
    torch.cuda.synchronize()
    X.assert_bits_equal(out.cpu(), X.bf16_rne(ref), "gemm_mx4 eager")
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        run()
    for i in range(3):
        out.zero_()
        scratch.zero_()
        gr.replay()
        torch.cuda.synchronize()
        X.assert_bits_equal(out.cpu(), X.bf16_rne(ref), f"gemm_mx4 replay {i}")
        assert int(ws.counters.abs().sum()) == 0


def test_refusals_and_declined_dispatch(monkeypatch):
    h, M, N, K = hip(), 129, 2 * BN, 640
    x, q, e, _ = T._exact_case(M, N, K, 4)
    xd, wq, sc = x.to(DEV), mx4.pack_b_mx4(q).to(DEV), mx4.pack_scales_mx4(e).to(DEV)
    scratch = torch.zeros(sum(mx4.a_image_bytes(M, K)) + 16, dtype=torch.uint8, device=DEV)
    a8, ea = mx4.quant_act_mx8(xd, M, K, scratch)
    obuf, out = C.guarded(M, N, device=DEV)
    ep = h.make_epi(out=out, ldo=out.stride(0))
    args = (M, N, K, h.EPI_STORE, ep)
    odd = torch.zeros(M + 1, K + 8, dtype=torch.bfloat16, device=DEV)
    small = h.CoopWorkspace(DEV, slab_floats=1024, groups=64)
    for bad in (lambda: mx4.gemm_mx4(a8, ea, wq[:64 * K // 2], sc[:64 * 2 * 16], M, 64, K, h.EPI_STORE, ep),   # N % BN
                lambda: mx4.gemm_mx4(a8, ea, wq, sc, M, N, K - 64, h.EPI_STORE, ep),                          # K % 128
                lambda: mx4.quant_act_mx8(odd.view(-1)[4:4 + M * (K + 8)].view(M, K + 8), M, K, scratch),     # misaligned rows
                lambda: mx4.gemm_mx4(scratch[8:], ea, wq, sc, *args),                                         # misaligned image
                lambda: mx4.gemm_mx4(a8, ea, wq, sc, M, N, K, h.EPI_ARGMAX,
                                     h.make_epi(keys=torch.zeros(M, dtype=torch.int64, device=DEV))),
                lambda: mx4.gemm_mx4(a8, ea, wq, sc, M, N, K, h.EPI_PARTIAL, ep),
                lambda: mx4.gemm_mx4(a8, ea, wq, sc, *args, cfg=(BN, 2), ws=small),                           # workspace
                lambda: mx4.gemm_mx4(a8, ea, wq, sc, *args, cfg=(BN, 4)),                                     # 2 groups, 4 splits
                lambda: mx4.gemm_mx4(a8, ea, wq, sc, *args, cfg=(64, 1))):                                    # not built
        with pytest.raises(ValueError):
            bad()
    assert mx4.proj_gemm_mx4(xd, wq, sc, *args, a_scratch=scratch) is False                       # the switch is off
    monkeypatch.setenv("LSA_MX4_GEMM", "1")
    assert mx4.proj_gemm_mx4(xd, wq[:192 * K // 2], sc[:192 * 2 * 16], M, 192, K, h.EPI_STORE, ep, a_scratch=scratch) is False
    assert mx4.proj_gemm_mx4(xd, wq, sc, *args, a_scratch=scratch[:1024]) is False                # no room for the image
    torch.cuda.synchronize()
    assert bool(C.is_sentinel(obuf).all())                                                        # nothing launched


def test_engine_runs_prefill_and_256_decode_rows_without_dequantising(monkeypatch):
    """W4A8 above 128 rows: against the bf16 engine on the dequantised weights the hidden state
    stays within what activation quantisation alone causes plus ENGINE_TOL, the bound of
    test_mx4_gpu's decode rows, for the same reason."""
    monkeypatch.setenv("LSA_MX4_GEMM", "1")
    cfg, e16, (e4,) = T._engines(max_slots=256, max_seq=256, max_prefill_rows=256)
    assert e4.part_k is None and e4.a_mx8 is not None
    for l16 in e16.layers:
        for name in ("qkv", "o", "gate_up", "down"):
            wp = getattr(l16, name)
            wp.copy_(packing.pack_b(mx4.dequantize_mx4(*mx4.quantize_mx4(packing.unpack_b(wp)))))

    def no_dequant(*a, **k):
        raise AssertionError("the forward dequantised a projection")
    monkeypatch.setattr(mx4, "dequant_mx4_packed", no_dequant)
    g = torch.Generator().manual_seed(5)
    for rows, lens in ((200, [200]), (256, [1] * 256)):
        toks = torch.randint(3, cfg.vocab_size - 1, (rows,), generator=g)
        hs = []
        for eng in (e16, e4):
            slots = list(range(len(lens)))
            for s_ in slots:
                eng.seq_len[s_] = 0
            sl, po = eng.prefill_rows(slots, lens)
            hs.append(eng.forward(eng.embed(toks.to(DEV)), sl, po).clone())
        err, aq = float(rel_err(hs[1], hs[0])), T._act_quant_error(cfg, toks)
        print(f"mxfp4 gemm {rows} rows: rel err {err:.3e}, activation quantisation alone {aq:.3e}")
        assert err < aq + ENGINE_TOL, rows
