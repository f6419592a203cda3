"""The int4 (W4A16) GEMM for prefill chunks and decode batches above 128 rows
(csrc/quant/gemm_int4.hip) on the GPU: the exact suite of tests/int4_cases.py over every built
config and every K split it admits, the fused-RMSNorm fields, the same bits as the cooperative GEMV,
the one-hot code case, replay in a captured graph, the refusals, and int4 engines at a 200-row
prefill and 256 decode rows (LSA_INT4_GEMM=1) with a dequantise kernel that raises."""
from collections import Counter

import pytest
import torch

import contract_cases as C
import exact_cases as X
import int4_cases as I4
import test_int4_coop_gpu as TC
import test_int4_gpu as T
from llm_sharding_amd.ops import int4, packing
from llm_sharding_amd.utils.numerics import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROWS = (1, 128, 129, 257)     # a lone row, a full tile, one valid row in the second row tile, a third tile
KS = (128, 384, 1024)         # one group (shorter than the ring); an odd group count against 2 splits; 8 groups against 2 / 4 / 8


def l_gemm(cfg=None, ws=None):
    def f(x, w, M, N, K, epi, ep, ar, norm, eps=T.EPS):
        int4.gemm_int4(x, w.wq, w.sc, M, N, K, epi, ep, ws=ws, cfg=cfg)
    return f


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("cfg", int4.INT4_GEMM_CONFIGS)
def test_exact_every_config(cfg, M, monkeypatch):
    h = T.hip()
    bn, N = cfg[0], 2 * cfg[0]
    ran = Counter()
    for K in KS:
        sks = [s for b, s in int4.int4_gemm_candidates(M, N, K) if b == bn]
        assert sks == [s for s in int4.INT4_GEMM_SPLITS if s <= K // 128]
        for sk in sks:
            launch, what = l_gemm((bn, sk)), f"gemm int4 {cfg} sk {sk}"
            lin = I4.case("linear", M, N, K, device=DEV)
            ran["linear"] += T._linear(h, launch, lin, ("store", "store_bias", "resid", "resid_bias"), what)
            if K >= I4.K_ROUND_MIN:
                ran["round_once"] += T._linear(h, launch, I4.case("round_once", M, N, K, device=DEV),
                                               ("store", "resid", "resid_bias"), what)
            ran["swiglu"] += T._swiglu(h, launch, I4.case("swiglu", M, N // 2, K, device=DEV), what)
            ran["qkv_rope"] += T._qkv(h, launch, TC.qkv_case(N // 16, M, K, True, monkeypatch), what)
            ran["qkv_bias"] += T._qkv(h, launch, TC.qkv_case(N // 16, M, K, False, monkeypatch), what)
            ran["gelu"] += T._gelu(h, launch, I4.case("gelu", M, N, K, device=DEV), what)
    assert all(ran[k] > 0 for k in ("linear", "round_once", "swiglu", "gelu", "qkv_rope", "qkv_bias")), dict(ran)


@pytest.mark.parametrize("sk", [1, 2])
def test_fused_norm_fields(sk):
    """ss_out: the bits of hip.row_ss on the kernel's own output. ss_in: SwiGLU of the RMS-normed
    rows against float64, at the tolerance tests/test_gemm_sk_gpu.py applies to that epilogue."""
    h = T.hip()
    c = I4.case("linear", 129, 256, 384, device=DEV)
    out = torch.zeros(c.M, c.N, dtype=torch.bfloat16, device=DEV)
    sbuf, ss = C.guarded(c.M, c.N // 64, dtype=torch.float32, device=DEV, guard_cols=0)
    int4.gemm_int4(c.a, c.W.wq, c.W.sc, c.M, c.N, c.K, h.EPI_RESID,
                   h.make_epi(out=out, resid=c.resid, ldo=c.N, ldr=c.N, bias=c.bias, ss_out=ss), cfg=(128, sk))
    torch.cuda.synchronize()
    C.assert_footprint(sbuf, ss, what="ss_out")
    X.assert_bits_equal(out, c.exp["resid_bias"], "resid + ss_out")
    want = torch.zeros_like(ss)
    h.row_ss(out, c.M, want)
    assert torch.equal(C.bits(ss), C.bits(want))
    M, I, K, eps = 200, 128, 256, 1e-5
    g = X.gen(11)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16).to(DEV)
    q, sc = int4.quantize_int4_groups(torch.randn(2 * I, K, generator=g) * 0.05)
    xs = torch.zeros(M, K // 64, dtype=torch.float32, device=DEV)
    h.row_ss(x, M, xs)
    obuf, o = C.guarded(M, I, device=DEV)
    int4.gemm_int4(x, int4.pack_b_int4(q).to(DEV), int4.pack_scales_int4(sc).to(DEV), M, 2 * I, K, h.EPI_SWIGLU,
                   h.make_epi(out=o, ldo=o.stride(0), ss_in=xs, ss_eps=eps), cfg=(128, sk))
    torch.cuda.synchronize()
    C.assert_footprint(obuf, o, what="swiglu ss_in")
    xd = x.double().cpu()
    xn = xd * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + eps)
    gu = (xn @ int4.dequantize_int4_groups(q, sc).double().T).view(M, I // 16, 2, 16)
    ref = torch.nn.functional.silu(gu[:, :, 0]) * gu[:, :, 1]
    assert rel_err(o.cpu(), ref.reshape(M, I)) < 1e-2


def test_same_bits_as_the_cooperative_kernel_and_one_hot():
    h = T.hip()
    c = I4.case("linear", 128, 256, 384, device=DEV)
    for form in ("store", "resid"):
        outs = []
        for fn in (int4.gemv_coop_int4, int4.gemm_int4):
            out = torch.zeros(c.M, c.N, dtype=torch.bfloat16, device=DEV)
            fn(c.a, c.W.wq, c.W.sc, c.M, c.N, c.K, h.EPI_STORE if form == "store" else h.EPI_RESID,
               h.make_epi(out=out, resid=None if form == "store" else c.resid, ldo=c.N, ldr=c.N))
            outs.append(out)
        X.assert_bits_equal(outs[1], outs[0], f"gemm vs coop int4 {form}")
    c = I4.case("one_hot", device=DEV)                           # every code value in every nibble position
    wq, sc, N = c.W.wq.repeat(8), c.W.sc.repeat(8, 1, 1), 8 * c.N
    obuf, out = C.guarded(c.M, N, device=DEV)
    int4.gemm_int4(c.a, wq, sc, c.M, N, c.K, h.EPI_STORE, h.make_epi(out=out, ldo=out.stride(0)), cfg=(128, 1))
    torch.cuda.synchronize()
    C.assert_footprint(obuf, out, what="gemm one-hot")
    X.assert_bits_equal(out, c.exp.repeat(1, 8), f"gemm {c.tag}")


def test_replay_in_a_captured_graph():
    h = T.hip()
    c = I4.case("linear", 257, 256, 1024, device=DEV)
    ws = h.CoopWorkspace(DEV, slab_floats=int4.int4_gemm_slab_floats(257, 256, 4), groups=6)
    out = torch.zeros(c.M, c.N, dtype=torch.bfloat16, device=DEV)
    ep = h.make_epi(out=out, resid=c.resid, ldo=c.N, ldr=c.N, bias=c.bias)

    def run():
        int4.gemm_int4(c.a, c.W.wq, c.W.sc, c.M, c.N, c.K, h.EPI_RESID, ep, ws=ws, cfg=(128, 4))
    run()
    torch.cuda.synchronize()
    X.assert_bits_equal(out, c.exp["resid_bias"], "gemm int4 eager")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    for i in range(3):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        X.assert_bits_equal(out, c.exp["resid_bias"], f"gemm int4 replay {i}")
        assert int(ws.counters.abs().sum()) == 0


def test_refusals_and_declined_dispatch(monkeypatch):
    h = T.hip()
    c = I4.case("linear", 129, 256, 384, device=DEV)
    obuf, out = C.guarded(129, 256, device=DEV)
    ep = h.make_epi(out=out, ldo=out.stride(0))
    args = (129, 256, 384, h.EPI_STORE, ep)
    odd = torch.zeros(130, 392, dtype=torch.bfloat16, device=DEV)
    small = h.CoopWorkspace(DEV, slab_floats=1024, groups=64)
    for bad in (lambda: int4.gemm_int4(c.a, c.W.wq[:64 * 384 // 2], c.W.sc[:4], 129, 64, 384, h.EPI_STORE, ep),  # N % BN
                lambda: int4.gemm_int4(c.a, c.W.wq, c.W.sc, 129, 256, 320, h.EPI_STORE, ep),                     # K % 128
                lambda: int4.gemm_int4(odd.view(-1)[4:4 + 129 * 392].view(129, 392), c.W.wq, c.W.sc, *args),       # misaligned A
                lambda: int4.gemm_int4(c.a, c.W.wq, c.W.sc, 129, 256, 384, h.EPI_ARGMAX,
                                       h.make_epi(keys=torch.zeros(129, dtype=torch.int64, device=DEV))),
                lambda: int4.gemm_int4(c.a, c.W.wq, c.W.sc, 129, 256, 384, h.EPI_PARTIAL, ep),
                lambda: int4.gemm_int4(c.a, c.W.wq, c.W.sc, *args, cfg=(128, 2), ws=small),                       # workspace
                lambda: int4.gemm_int4(c.a, c.W.wq, c.W.sc, *args, cfg=(128, 4)),                                 # 3 groups, 4 splits
                lambda: int4.gemm_int4(c.a, c.W.wq, c.W.sc, *args, cfg=(256, 1))):                                # not built
        with pytest.raises(ValueError):
            bad()
    monkeypatch.setenv("LSA_INT4_GEMM", "1")
    c = I4.case("linear", 129, 192, 384, device=DEV)             # 192 columns: no built tile divides them
    assert int4.proj_gemm_int4(c.a, c.W.wq, c.W.sc, 129, 192, 384, h.EPI_STORE, ep) is False
    torch.cuda.synchronize()
    assert bool(C.is_sentinel(obuf).all())                       # refused or declined: nothing launched


@pytest.mark.parametrize("kind", ["llama", "gpt2"])
def test_engine_runs_prefill_and_256_decode_rows_without_dequantising(kind, monkeypatch):
    """The int4 engine against the bf16 engine on the same effective weights at a 200-row prefill
    and 256 decode rows, with a dequantise kernel that raises: every projection ran on int4."""
    monkeypatch.setenv("LSA_INT4_GEMM", "1")
    cfg, e16, (e4,) = T._engines(kind, max_slots=256, max_seq=256, max_prefill_rows=256)
    T._same_effective_weights(cfg, e16, e4)
    assert e4.part_k is None

    def no_dequant(*a, **k):
        raise AssertionError("the forward dequantised a projection")
    monkeypatch.setattr(int4, "dequant_int4_packed", no_dequant)
    g = torch.Generator().manual_seed(5)
    for rows, lens in ((200, [200]), (256, [1] * 256)):
        toks = torch.randint(3, cfg.vocab_size - 1, (rows,), generator=g)
        hs = []
        for e in (e16, e4):
            slots = list(range(len(lens)))
            for s_ in slots:
                e.seq_len[s_] = 0
            sl, po = e.prefill_rows(slots, lens)
            hs.append(e.forward(e.embed(toks.to(DEV)), sl, po).clone())
        err = rel_err(hs[1], hs[0])
        print(f"{kind} int4 {rows} rows: rel err {float(err):.3e}")
        assert err < T.ENGINE_TOL, rows
