"""The MXFP4 (W4A8) weight path on the GPU: the activation quantiser seen through one-hot weights,
exact arithmetic over every built config, Gaussian operands through every epilogue, the dequantise
kernel, and weight_dtype="mxfp4" engines against a bf16 engine holding the same weights."""
import pytest
import torch
import torch.nn.functional as F

import contract_cases as C
import exact_cases as X
import test_footprint_gpu as FP
from llm_sharding_amd.config import tiny
from llm_sharding_amd.ops import mx4, packing
from llm_sharding_amd.runtime.engine import DecodeGraph, StageEngine
from llm_sharding_amd.runtime.engine_int4 import make_stage_engine
from llm_sharding_amd.runtime.engine_mx4 import Mx4StageEngine
from llm_sharding_amd.utils.numerics import rel_err
from test_int4_gpu import ENGINE_TOL, EPS, _CpuGen, hip

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _launch(h, x, q, e, M, epi, ep, norm=False, cfg=None):
    N, K = q.shape
    mx4.gemv_mx4(x, mx4.pack_b_mx4(q).to(DEV), mx4.pack_scales_mx4(e).to(DEV), M, N, K, epi, ep, norm=norm, eps=EPS, cfg=cfg)
    torch.cuda.synchronize()


def _store(h, x, q, e, cfg=None):
    """y = x @ W^T through the STORE epilogue into a canary-padded buffer: the bf16 result."""
    M = x.shape[0]
    obuf, out = C.guarded(M, q.shape[0], device=DEV)
    _launch(h, x.to(DEV), q, e, M, h.EPI_STORE, h.make_epi(out=out, ldo=out.stride(0)), cfg=cfg)
    C.assert_footprint(obuf, out, what=f"mx4 store {tuple(x.shape)} x {tuple(q.shape)} cfg {cfg}")
    return out.cpu()


# ------------------------------------------------------------------------------ 1. activation quantiser
@pytest.mark.parametrize("M", [7, 33])
@pytest.mark.parametrize("K", [128, 384])
def test_activation_quantiser_through_one_hot_weights(M, K):
    """W = identity (code 1.0, scale 1): y[m, n] is bf16(dequantised a[m, n]), bit for bit."""
    g = X.gen(M + K)
    x = torch.randn(M, K, generator=g) * torch.logspace(-2, 2, M)[:, None]
    x[0, :32] = torch.arange(32) * 8 / 128 + 4 / 128         # maximum last; x * 128 = 4, 12, ..: e4m3 ties in [64, 128)
    x[1, :32] = torch.arange(32, 0, -1) * 8 / 128 - 4 / 128  # the same, maximum first
    x[2, 32:64] = 0                                           # an all-zero block
    x[3, 64:96] = torch.arange(32) * 2.0 ** -133              # a block of bf16 subnormals
    x = x.to(torch.bfloat16)
    q = torch.eye(K, dtype=torch.uint8) * 2
    e = torch.full((K, K // 32), 127, dtype=torch.uint8)
    want = mx4.dequantize_act_mx8(*mx4.quantize_act_mx8(x)).float().to(torch.bfloat16)
    X.assert_bits_equal(_store(hip(), x, q, e), want, f"mx4 one-hot M={M} K={K}")


# ------------------------------------------------------------------------------ 2. exact arithmetic
def _exact_case(M, N, K, seed):
    """All 16 codes, block exponents in [-3, 3], integer activations up to 15 (four significant
    bits: lossless as e4m3 at the block's scale). Every product is a multiple of 2^-4, so a sum of
    magnitudes below 2^20 keeps every fp32 partial sum exact."""
    g = X.gen(seed)
    q = torch.randint(0, 16, (N, K), generator=g).to(torch.uint8)
    e = torch.randint(124, 131, (N, K // 32), generator=g).to(torch.uint8)
    x = torch.randint(-15, 16, (M, K), generator=g).to(torch.bfloat16)
    codes, ea = mx4.quantize_act_mx8(x)
    assert torch.equal(mx4.dequantize_act_mx8(codes, ea), x.double())
    w = mx4.dequantize_mx4(q, e).double()
    assert float((x.double().abs() @ w.abs().t()).max()) < 2 ** 20
    ref = mx4.linear_reference(x, q, e)
    return x, q, e, ref


@pytest.mark.parametrize("N", [48, 112])  # 3 tiles; 7 tiles: no wave count divides it
@pytest.mark.parametrize("K", [128, 384, 640])
def test_exact_arithmetic_and_fragment_layout(K, N):
    h = hip()
    ties = 0
    for M in (1, 7, 16, 17, 33, 128):
        x, q, e, ref = _exact_case(M, N, K, M + N + K)
        ties += int(X.is_tie(ref).sum())
        X.assert_bits_equal(_store(h, x, q, e), X.bf16_rne(ref), f"mx4 exact M={M} N={N} K={K}")
    assert ties > 0  # outputs that sit exactly between two bf16 values are among them


@pytest.mark.parametrize("sk", mx4.MX4_SPLITS)
@pytest.mark.parametrize("cfg", mx4.MX4_CONFIGS)
def test_exact_every_config(cfg, sk):
    """Every built (mb, tnw, nw) at every K split, at the smallest K the split allows plus one
    K-step (a short last scale group)."""
    mb, tnw, nw = cfg
    M, K = {1: 7, 2: 17, 4: 33, 8: 128}[mb], 512 * sk + 128
    x, q, e, ref = _exact_case(M, 112, K, 1000 + 8 * mb + sk)
    X.assert_bits_equal(_store(hip(), x, q, e, cfg=(tnw, nw, sk)), X.bf16_rne(ref), f"mx4 exact cfg {cfg} sk {sk}")


# ------------------------------------------------------------------------------ 3. Gaussian operands
def _gauss(M, N, K, seed, scale=0.02):
    g = X.gen(seed)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    q, e = mx4.quantize_mx4(torch.randn(N, K, generator=g) * scale)
    rstd = torch.rsqrt(x.double().pow(2).mean(-1, keepdim=True) + EPS)
    return g, x, q, e, mx4.linear_reference(x, q, e), rstd


@pytest.mark.parametrize("M", [7, 33])
@pytest.mark.parametrize("kind", ["store_norm", "resid", "swiglu_norm"])
def test_gaussian_epilogues(kind, M):
    """linear_reference holds the quantisation of both operands, so only the bf16 output rounding
    and the fp32 summation order are left: the tolerances of tests/test_footprint_gpu.py."""
    h = hip()
    N, K = (416, 256) if kind.startswith("swiglu") else (208, 384)
    g, x, q, e, y, rstd = _gauss(M, N, K, M + len(kind), 0.05 if kind.startswith("swiglu") else 0.02)
    obuf, out = C.guarded(M, N // 2 if kind.startswith("swiglu") else N, device=DEV)
    if kind == "store_norm":
        ref, tol = y * rstd, 8e-3
        _launch(h, x.to(DEV), q, e, M, h.EPI_STORE, h.make_epi(out=out, ldo=out.stride(0)), norm=True)
    elif kind == "resid":
        resid = torch.randn(M, N, generator=g).to(torch.bfloat16).to(DEV)
        ref, tol = resid.cpu().double() + y, 8e-3
        _launch(h, x.to(DEV), q, e, M, h.EPI_RESID, h.make_epi(out=out, resid=resid, ldo=out.stride(0), ldr=N))
    else:
        gu = (y * rstd).view(M, N // 32, 2, 16)
        ref, tol = (F.silu(gu[:, :, 0]) * gu[:, :, 1]).reshape(M, N // 2), 1e-2
        _launch(h, x.to(DEV), q, e, M, h.EPI_SWIGLU, h.make_epi(out=out, ldo=out.stride(0)), norm=True)
    C.assert_footprint(obuf, out, what=f"mx4 {kind} M={M}")
    err = rel_err(out.cpu(), ref.float())
    print(f"mx4 {kind} M={M}: rel err {float(err):.3e}")
    assert err < tol


@pytest.mark.parametrize("M", [7, 33])
def test_gaussian_qkv_rope(M):
    h = hip()
    NH, NKV, HD, K, SLOTS, T_MAX = FP.NH, FP.NKV, FP.HD, FP.H_IN, FP.SLOTS, FP.T_MAX
    g = X.gen(M)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    wq, wk, wv = (torch.randn(n * HD, K, generator=g) * 0.05 for n in (NH, NKV, NKV))
    q4, e4 = mx4.quantize_mx4(packing.fuse_qkv(wq, wk, wv, NH, NKV, HD))
    y = mx4.linear_reference(x, q4, e4)  # packed column order: un-permute q and k
    inv_q, inv_k = torch.argsort(packing.rope_rows_perm(NH, HD)), torch.argsort(packing.rope_rows_perm(NKV, HD))
    zq, zk, zv = y[:, :NH * HD][:, inv_q], y[:, NH * HD:(NH + NKV) * HD][:, inv_k], y[:, (NH + NKV) * HD:]
    cells = torch.randperm(SLOTS * T_MAX, generator=g)[:M]
    slot, pos = (cells // T_MAX).to(torch.int32).to(DEV), (cells % T_MAX).to(torch.int32).to(DEV)
    cos, sin = FP._rope_tables()
    qbuf, qo = C.guarded(M, NH * HD, device=DEV)
    kflat, kc = C.guarded_cache(SLOTS, NKV, T_MAX, HD, DEV)
    vflat, vc = C.guarded_cache(SLOTS, NKV, T_MAX, HD, DEV)
    ep = h.make_epi(out=qo, k_cache=kc, v_cache=vc, slot=slot, pos=pos, cos=cos, sin=sin, ldo=qo.stride(0), n_heads=NH,
                    n_kv=NKV, head_dim=HD, t_max=T_MAX)
    _launch(h, x.to(DEV), q4, e4, M, h.EPI_QKV, ep)
    C.assert_footprint(qbuf, qo, what="mx4 qkv q")
    C.assert_cache_footprint(kflat, kc, slot.long(), pos.long(), what="mx4 qkv k_cache")
    C.assert_cache_footprint(vflat, vc, slot.long(), pos.long(), what="mx4 qkv v_cache")
    pl, c64, s64 = pos.long().cpu(), cos.cpu().double(), sin.cpu().double()
    rq, rk = FP._rope_ref(zq.view(M, NH, HD), pl, c64, s64), FP._rope_ref(zk.view(M, NKV, HD), pl, c64, s64)
    assert rel_err(qo.cpu(), rq.reshape(M, -1).float()) < 1e-2
    assert rel_err(kc[slot.long(), :, pos.long()].cpu(), rk.float()) < 1e-2
    assert rel_err(vc[slot.long(), :, pos.long()].cpu(), zv.view(M, NKV, HD).float()) < 1e-2


def test_graph_replay_matches_eager():
    h = hip()
    M, N, K = 33, 208, 1024
    g, x, q, e, y, rstd = _gauss(M, N, K, 5)
    xd, wq, ws = x.to(DEV), mx4.pack_b_mx4(q).to(DEV), mx4.pack_scales_mx4(e).to(DEV)
    outs = [torch.zeros(M, N, dtype=torch.bfloat16, device=DEV) for _ in range(2)]
    run = lambda o: mx4.gemv_mx4(xd, wq, ws, M, N, K, h.EPI_STORE, h.make_epi(out=o, ldo=N), norm=True, eps=EPS, cfg=(1, 4, 2))
    run(outs[0])
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=st):
            run(outs[1])
    for i in range(3):  # the arrival counters are reset by the kernel: every replay gives the eager bits
        outs[1].zero_()
        gr.replay()
        torch.cuda.synchronize()
        X.assert_bits_equal(outs[1], outs[0], f"mx4 graph replay {i}")
    assert rel_err(outs[0].cpu(), (y * rstd).float()) < 8e-3


# ------------------------------------------------------------------------------ 4. dequantise kernel
@pytest.mark.parametrize("shape", [(48, 384), (4096, 128)])
def test_dequant_kernel(shape):
    hip()
    N, K = shape
    g = X.gen(N)
    q = torch.randint(0, 16, (N, K), generator=g).to(torch.uint8)
    e = torch.randint(2, 253, (N, K // 32), generator=g).to(torch.uint8)
    obuf, out = C.guarded_flat(N * K, torch.bfloat16, DEV, guard=4096)
    wp = mx4.dequant_mx4_packed(mx4.pack_b_mx4(q).to(DEV), mx4.pack_scales_mx4(e).to(DEV), out, N, K)
    torch.cuda.synchronize()
    C.assert_footprint(obuf, out, what=f"dequant_mx4 {shape}")
    X.assert_bits_equal(wp.cpu(), packing.pack_b(mx4.dequantize_mx4(q, e)), f"dequant_mx4 {shape}")


# ------------------------------------------------------------------------------ 5. engine
def _engines(n=1, **over):
    cfg = tiny(layers=2, hidden=256, heads=4, kv_heads=2, head_dim=64, inter=384, vocab=512)
    kw = dict(has_embed=True, has_head=True, source=_CpuGen(cfg, 7), max_slots=128, max_seq=128, max_prefill_rows=128)
    kw.update(over)
    e16 = StageEngine(cfg, 0, 2, DEV, torch.bfloat16, **kw)
    return cfg, e16, [make_stage_engine(cfg, 0, 2, DEV, torch.bfloat16, weight_dtype="mxfp4", **kw) for _ in range(n)]


def _act_quant_error(cfg, toks):
    """The hidden-state rel_err that MXFP8 activations alone cause for this config and seed, on
    the CPU: models/reference.py's layers on the dequantised mxfp4 weights, with every projection
    as written against every projection's input passed through quantize_act_mx8."""
    from llm_sharding_amd.models import reference as R
    src = _CpuGen(cfg, 7)
    layers = [{k: (mx4.dequantize_mx4(*mx4.quantize_mx4(v)) if k.endswith("proj.weight") else v)
               for k, v in src.layer(i, "cpu", torch.bfloat16).items()} for i in range(2)]
    lin = F.linear

    def run(linear):
        m = R.ReferenceLlama(cfg, src.embedding("cpu", torch.bfloat16), layers, src.final_norm("cpu", torch.bfloat16),
                             src.lm_head("cpu", torch.bfloat16))
        R.F.linear = linear
        try:
            return m.forward_hidden(m.embed[toks][:, None])[:, 0]
        finally:
            R.F.linear = lin
    a8 = lambda x: mx4.dequantize_act_mx8(*mx4.quantize_act_mx8(x.to(torch.bfloat16).reshape(-1, x.shape[-1]))).float().view(x.shape)
    return float(rel_err(run(lambda x, w, b=None: lin(a8(x), w, b)), run(lin)))


def test_engine_matches_bf16_engine_on_the_same_weights():
    """The engine holds exactly quantize_mx4 of the folded matrices. Against the bf16 engine loaded
    with the dequantised weights: a 160-row prefill (dequantise + the bf16 kernels on both sides, W4A16)
    within ENGINE_TOL; 5 / 64 / 128 decode rows (W4A8) within ENGINE_TOL plus what activation
    quantisation alone causes (_act_quant_error: 5.3e-3, 5.3e-3, 5.5e-3 for these rows and seeds)."""
    cfg, e16, (e4,) = _engines(max_seq=256, max_prefill_rows=160)
    assert type(e4) is Mx4StageEngine and e4.mx4 and e4.lm_head_s is None and torch.equal(e4.lm_head, e16.lm_head)
    for l16, l4 in zip(e16.layers, e4.layers):
        for name, (N, K) in zip(("qkv", "o", "gate_up", "down"), StageEngine.proj_shapes(cfg)):
            wp = getattr(l16, name)
            q, e = mx4.quantize_mx4(packing.unpack_b(wp))
            assert torch.equal(getattr(l4, name), mx4.pack_b_mx4(q)) and torch.equal(getattr(l4, name + "_s"), mx4.pack_scales_mx4(e))
            wp.copy_(packing.pack_b(mx4.dequantize_mx4(q, e)))
    for rows in (160, 5, 64, 128):
        toks = torch.randint(3, cfg.vocab_size - 1, (rows,), generator=torch.Generator().manual_seed(rows))
        hs = []
        for eng in (e16, e4):
            slots, lens = (list(range(rows)), [1] * rows) if rows <= 128 else ([0], [rows])  # decode batch / one prompt
            for s_ in range(128):
                eng.seq_len[s_] = 0
            sl, po = eng.prefill_rows(slots, lens)
            hs.append(eng.forward(eng.embed(toks.to(DEV)), sl, po).clone())
        err, aq = float(rel_err(hs[1], hs[0])), (_act_quant_error(cfg, toks) if rows <= mx4.MX4_MAX_ROWS else 0.0)
        print(f"mxfp4 {rows} rows: rel err {err:.3e}, activation quantisation alone {aq:.3e}")
        assert err < aq + ENGINE_TOL, rows


@pytest.mark.parametrize("rows", [5, 64, 128])
def test_decode_graph_replays_the_eager_tokens(rows):
    cfg, _, (e1, e2) = _engines(n=2)
    first = torch.randint(3, cfg.vocab_size - 1, (rows,), generator=torch.Generator().manual_seed(rows))
    toks, eager = first, []
    for _ in range(3):
        sl, po = e1.prefill_rows(list(range(rows)), [1] * rows)
        hh = e1.forward(e1.embed(toks.to(DEV)), sl, po)
        e1.advance(list(range(rows)), [1] * rows)
        toks = e1.head(hh).cpu()
        eager.append(toks.tolist())
    dg = DecodeGraph(e2, rows, "full", history_len=3)
    dg.tokens.copy_(first.to(torch.int32))
    dg.capture()
    for _ in range(3):
        dg.replay()
    torch.cuda.synchronize()
    assert dg.history.cpu().tolist() == eager
