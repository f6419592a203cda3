"""The int4 (W4A16) weight path on the GPU: every code value in every nibble position, the exact
suite over every built config (tests/int4_cases.py), write footprints, the dequantise kernel,
and weight_dtype="int4" engines (Llama and GPT-2) against bf16 engines holding the same
effective weights."""
from collections import Counter

import numpy as np
import pytest
import torch

import contract_cases as C
import exact_cases as X
import int4_cases as I4
import test_footprint_gpu as FP
import ulp_cases as U
from llm_sharding_amd.config import tiny, tiny_gpt2
from llm_sharding_amd.ops import int4, packing
from llm_sharding_amd.ops import sampling as S
from llm_sharding_amd.runtime.engine import DecodeGraph, RandomSource, StageEngine
from llm_sharding_amd.runtime.engine_int4 import Int4StageEngine, make_stage_engine
from llm_sharding_amd.runtime.sampling import Sampler, SamplingParams
from llm_sharding_amd.utils.numerics import rel_err
from sampling_cases import GAP_MIN

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-5
ENGINE_TOL = 3e-2  # tests/test_engine_gpu.py: two kernel paths of the same depth, numerics.rel_err


def hip():
    from llm_sharding_amd.ops import hip as h
    h.lib()
    return h


def l_int4(h, cfg=None):
    def f(x, w, M, N, K, epi, ep, ar, norm, eps=EPS):
        int4.gemv_int4(x, w.wq, w.sc, M, N, K, epi, ep, norm=norm, eps=eps, a_rows=ar, cfg=cfg)
    return f


# ------------------------------------------------------------------------------ 1. every code, every position
def test_every_code_value_in_every_position():
    """A one-hot activation row picks one weight: the output is q[n, k] * s[n] exactly, for all 15
    code values in each of the 32 nibble positions of the 16-byte word (and every lane)."""
    h = hip()
    c = I4.case("one_hot", device=DEV)
    ran = 0
    for cfg, r0, M in (((1, 4, 1), 0, 64), ((1, 8, 1), 64, 64), ((1, 4, 1), 0, 1), ((1, 4, 2), 77, 1), ((1, 8, 2), 5, 16), ((1, 8, 1), 100, 17)):
        obuf, out = C.guarded(M, c.N, device=DEV)
        a = c.a[r0:r0 + M].contiguous()
        l_int4(h, cfg)(a, c.W, M, c.N, c.K, h.EPI_STORE, h.make_epi(out=out, ldo=out.stride(0)), None, False)
        torch.cuda.synchronize()
        C.assert_footprint(obuf, out, what=f"one-hot rows {r0}..{r0 + M}")
        X.assert_bits_equal(out, c.exp[r0:r0 + M], f"{c.tag} rows {r0}..{r0 + M} cfg {cfg}")
        ran += 1
    assert ran == 6


# ------------------------------------------------------------------------------ 2. exact suite
def _linear(h, launch, c, forms, what, ar=None, a=None):
    n = 0
    for form in forms:
        obuf, out = C.guarded(c.M, c.N, device=DEV)
        bias = c.bias if form.endswith("bias") else None
        if form.startswith("store"):
            ep, epi = h.make_epi(out=out, ldo=out.stride(0), bias=bias), h.EPI_STORE
        else:
            ep, epi = h.make_epi(out=out, resid=c.resid, ldo=out.stride(0), ldr=c.resid.stride(0), bias=bias), h.EPI_RESID
        launch(c.a if a is None else a, c.W, c.M, c.N, c.K, epi, ep, ar, False)
        torch.cuda.synchronize()
        tag = f"{what} {c.tag} {form}"
        C.assert_footprint(obuf, out, what=tag)
        X.assert_bits_equal(out, c.exp[form], tag, unit=c.unit)
        n += 1
    return n


def _swiglu(h, launch, c, what):
    obuf, out = C.guarded(c.M, c.I, device=DEV)
    launch(c.a, c.W, c.M, c.N, c.K, h.EPI_SWIGLU, h.make_epi(out=out, ldo=out.stride(0)), None, False)
    torch.cuda.synchronize()
    C.assert_footprint(obuf, out, what=f"{what} {c.tag}")
    X.assert_bits_equal(out, c.exp, f"{what} {c.tag}")
    return 1


def _qkv(h, launch, c, what):
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


def _gelu(h, launch, c, what):
    """STORE + bias + GELU at the half-ulp bound of tests/ulp_cases.py (SLACK_ACT): the
    pre-activation is exact, so the activation's own fp32 operations are all that may err."""
    obuf, out = C.guarded(c.M, c.N, device=DEV)
    launch(c.a, c.W, c.M, c.N, c.K, h.EPI_STORE, h.make_epi(out=out, ldo=out.stride(0), bias=c.bias, act=h.ACT_GELU), None, False)
    torch.cuda.synchronize()
    C.assert_footprint(obuf, out, what=f"{what} {c.tag}")
    U.assert_half_ulp(out, c.exact, U.SLACK_ACT, f"{what} {c.tag}", inp=c.inp)
    return 1


def _a_rows(h, launch, c, what):
    """The activations scattered over a larger NaN-filled buffer and gathered through a_rows."""
    R = c.M + 9
    x = torch.full((R, c.K), float("nan"), dtype=torch.bfloat16, device=DEV)
    idx = torch.randperm(R, generator=X.gen(c.M + c.K))[:c.M].to(DEV)
    x[idx] = c.a
    ar = torch.cat([idx, torch.full((4,), R - 1, device=DEV)]).to(torch.int32)
    return _linear(h, launch, c, ("store", "resid_bias"), what + " a_rows", ar=ar, a=x)


def _norm(h, launch, c, what):
    """norm=True with mean(x^2) = 4 and eps = 12: the factor is exactly 1/4. Bitwise wherever the
    result is not next to a bf16 rounding boundary, within one ulp everywhere."""
    obuf, out = C.guarded(c.M, c.N, device=DEV)
    launch(c.a, c.W, c.M, c.N, c.K, h.EPI_STORE, h.make_epi(out=out, ldo=out.stride(0)), None, True, eps=c.eps)
    torch.cuda.synchronize()
    C.assert_footprint(obuf, out, what=f"{what} {c.tag}")
    X.assert_within_one_ulp(out, c.exp, f"{what} {c.tag}")
    X.assert_bits_equal(torch.where(c.safe, out, c.exp), c.exp, f"{what} {c.tag}")
    return 1


@pytest.mark.parametrize("cfg", int4.INT4_CONFIGS)
def test_exact_every_config(cfg):
    h = hip()
    tn, mb, nw, ug = cfg
    N = I4.n_for(tn)
    launch = l_int4(h, (tn, nw, ug))
    ran = Counter()
    for M in (m for m in I4.ROWS if packing.row_blocks(m) == mb):
        for K in I4.KS:
            what = f"int4 {cfg}"
            lin = I4.case("linear", M, N, K, device=DEV)
            ran["linear"] += _linear(h, launch, lin, ("store", "store_bias", "resid", "resid_bias"), what)
            if K >= I4.K_ROUND_MIN:
                ran["round_once"] += _linear(h, launch, I4.case("round_once", M, N, K, device=DEV),
                                             ("store", "resid", "resid_bias"), what)
            if tn % 2 == 0:
                ran["swiglu"] += _swiglu(h, launch, I4.case("swiglu", M, N // 2, K, device=DEV), what)
            ran["qkv_rope"] += _qkv(h, launch, I4.case("qkv", M, K, True, device=DEV), what)
            ran["qkv_bias"] += _qkv(h, launch, I4.case("qkv", M, K, False, device=DEV), what)
            ran["gelu"] += _gelu(h, launch, I4.case("gelu", M, N, K, device=DEV), what)
            ran["a_rows"] += _a_rows(h, launch, lin, what)
            ran["norm"] += _norm(h, launch, I4.case("norm", M, N, K, device=DEV), what)
    kinds = ["linear", "round_once", "qkv_rope", "qkv_bias", "gelu", "a_rows", "norm"] + (["swiglu"] if tn % 2 == 0 else [])
    assert all(ran[k] > 0 for k in kinds), (cfg, dict(ran))


def test_dispatch_and_argument_checks():
    """hip.gemv_int4's own choice of config, and the shapes it refuses before any launch."""
    h = hip()
    for M in (1, 33):
        _linear(h, l_int4(h), I4.case("linear", M, 96, 384, device=DEV), ("store", "resid"), "int4 dispatch")
    c = I4.case("linear", 1, 48, 128, device=DEV)
    out = torch.empty(65, 48, dtype=torch.bfloat16, device=DEV)
    ep = h.make_epi(out=out, ldo=48)
    x65 = torch.zeros(65, 128, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError):
        int4.gemv_int4(x65, c.W.wq, c.W.sc, 65, 48, 128, h.EPI_STORE, ep)          # rows
    with pytest.raises(ValueError):
        int4.gemv_int4(c.a, c.W.wq[:-16], c.W.sc, 1, 48, 128, h.EPI_STORE, ep)     # weight bytes
    with pytest.raises(ValueError):
        int4.gemv_int4(c.a, c.W.wq, c.W.sc.view(-1)[:-1], 1, 48, 128, h.EPI_STORE, ep)  # scales
    with pytest.raises(ValueError):
        int4.gemv_int4(c.a, c.W.wq, c.W.sc, 1, 48, 128, h.EPI_STORE, ep, cfg=(2, 4, 1))  # 3 tiles, tn = 2
    with pytest.raises(ValueError):
        int4.gemv_int4(c.a, c.W.wq, c.W.sc, 1, 48, 128, h.EPI_ARGMAX, h.make_epi(keys=torch.zeros(1, dtype=torch.int64, device=DEV)))
    with pytest.raises(ValueError):
        int4.gemv_int4(c.a, c.W.wq, c.W.sc, 1, 48, 128, h.EPI_STORE, ep, cfg=(3, 4, 1))  # not built


# ------------------------------------------------------------------------------ 3. footprint
class _W4:
    """test_footprint_gpu.W for int4: the reference is exactly what the kernel multiplies by."""

    def __init__(self, w, fp8=False):
        q, sc = int4.quantize_int4_groups(w)
        self.ref = int4.dequantize_int4_groups(q, sc)
        self.wq, self.sc, self.wp = int4.pack_b_int4(q), int4.pack_scales_int4(sc), None


@pytest.mark.parametrize("kind", ["store", "resid", "swiglu", "qkv_rope", "qkv_bias"])
def test_footprint(kind, monkeypatch):
    """The guard-band harness of tests/test_footprint_gpu.py with the int4 launcher: Gaussian
    operands in NaN-padded buffers, nothing outside out[:M] and the KV cells named by slot / pos
    written, numerics at that file's tolerances."""
    h = hip()
    monkeypatch.setattr(FP, "W", _W4)
    L = l_int4(h)
    if kind == "store":
        FP.run_epi(h, L, "store", 7, 208, 384, seed=1, fp8=True, a_rows=True, norm=True, bias=True, what="int4")
    elif kind == "resid":
        FP.run_epi(h, L, "resid", 50, 208, 384, seed=2, fp8=True, a_rows=True, norm=False, bias=True, what="int4")
    elif kind == "swiglu":
        FP.run_epi(h, L, "swiglu", 17, 416, 256, seed=3, fp8=True, a_rows=False, norm=True, what="int4")
    elif kind == "qkv_rope":
        FP.run_qkv(h, L, 7, seed=4, rope=True, fp8=True, what="int4")
        FP.run_qkv(h, L, 50, seed=5, rope=True, fp8=True, bad_pos=True, what="int4")
    else:
        FP.run_qkv(h, L, 33, seed=6, rope=False, bias=True, fp8=True, what="int4")


# ------------------------------------------------------------------------------ 4. dequantise kernel
@pytest.mark.parametrize("shape", [(48, 384), (4096, 128)])
def test_dequant_kernel(shape):
    h = hip()
    N, K = shape
    g = X.gen(N)
    q = X.randint(-7, 7, (N, K), g, DEV).to(torch.int8)
    sc = (torch.rand(N, K // 128, generator=g) * 0.01 + 1e-4).to(DEV)
    obuf, out = C.guarded_flat(N * K, torch.bfloat16, DEV, guard=4096)
    wp = int4.dequant_int4_packed(int4.pack_b_int4(q), int4.pack_scales_int4(sc), out, N, K)
    torch.cuda.synchronize()
    C.assert_footprint(obuf, out, what=f"dequant_int4 {shape}")
    want = packing.pack_b(int4.dequantize_int4_groups(q, sc).to(torch.bfloat16))
    X.assert_bits_equal(wp, want, f"dequant_int4 {shape}")
    with pytest.raises(ValueError):
        int4.dequant_int4_packed(int4.pack_b_int4(q), int4.pack_scales_int4(sc), out[:-8], N, K)


# ------------------------------------------------------------------------------ 5. engine
class _CpuGen(RandomSource):
    """Random weights drawn on the CPU in bf16, then moved: every engine sees the same values."""

    def layer(self, i, device, dtype):
        return {k: v.to(device, dtype) for k, v in super().layer(i, "cpu", torch.bfloat16).items()}

    def embedding(self, device, dtype):
        return super().embedding("cpu", torch.bfloat16).to(device, dtype)

    def final_norm(self, device, dtype):
        return super().final_norm("cpu", torch.bfloat16).to(device, dtype)

    def lm_head(self, device, dtype):
        return super().lm_head("cpu", torch.bfloat16).to(device, dtype)

    def pos_embedding(self, device, dtype):
        t = super().pos_embedding("cpu", torch.bfloat16)
        return None if t is None else t.to(device, dtype)

    def final_norm_bias(self, device, dtype):
        t = super().final_norm_bias("cpu", torch.bfloat16)
        return None if t is None else t.to(device, dtype)


def _cfg(kind):
    if kind == "llama":
        return tiny(layers=2, hidden=256, heads=4, kv_heads=2, head_dim=64, inter=384, vocab=512)
    return tiny_gpt2(layers=2, hidden=384, heads=6, vocab=500)


def _engines(kind, n=1, **over):
    cfg = _cfg(kind)
    kw = dict(has_embed=True, has_head=True, source=_CpuGen(cfg, 7), max_slots=80, max_seq=128, max_prefill_rows=128)
    kw.update(over)
    e16 = StageEngine(cfg, 0, 2, DEV, torch.bfloat16, **kw)
    e4 = [make_stage_engine(cfg, 0, 2, DEV, torch.bfloat16, weight_dtype="int4", **kw) for _ in range(n)]
    return cfg, e16, e4


def _same_effective_weights(cfg, e16, e4):
    """Overwrite the bf16 engine's packed projections with bf16(dequantise(quantise(folded))) and
    check that the int4 engine holds exactly quantise(folded), at 4.25 bits per weight."""
    for l16, l4 in zip(e16.layers, e4.layers):
        for name, (N, K) in zip(("qkv", "o", "gate_up", "down"), StageEngine.proj_shapes(cfg)):
            wp, w4, s4 = getattr(l16, name), getattr(l4, name), getattr(l4, name + "_s")
            q, sc = int4.quantize_int4_groups(packing.unpack_b(wp))
            assert w4.dtype == torch.uint8 and w4.numel() == N * K // 2, name
            assert s4.dtype == torch.float32 and s4.numel() == N * K // 128, name
            assert torch.equal(w4, int4.pack_b_int4(q)) and torch.equal(s4, int4.pack_scales_int4(sc)), name
            wp.copy_(packing.pack_b(int4.dequantize_int4_groups(q, sc).to(torch.bfloat16)))


@pytest.mark.parametrize("kind", ["llama", "gpt2"])
def test_engine_matches_bf16_engine_on_the_same_weights(kind):
    cfg, e16, (e4,) = _engines(kind)
    assert type(e4) is Int4StageEngine and e4.int4 and e4.lm_head_s is None and e4.w_scratch is not None
    assert torch.equal(e4.lm_head, e16.lm_head)                # the head stays bf16
    _same_effective_weights(cfg, e16, e4)
    proj16 = sum(n * k * 2 for n, k in StageEngine.proj_shapes(cfg)) * 2
    assert e16.memory_bytes() - e4.memory_bytes() == proj16 - 2 * sum(int4.int4_bytes(n, k) for n, k in StageEngine.proj_shapes(cfg))
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(3, cfg.vocab_size - 1, (100,), generator=g)
    outs = []
    for e in (e16, e4):                                         # prefill, 100 rows: scratch + GEMM
        sl, po = e.prefill_rows([0], [100])
        outs.append(e.forward(e.embed(ids.to(DEV)), sl, po).clone())
        e.advance([0], [100])
    err = rel_err(outs[1], outs[0])
    print(f"{kind} int4 prefill 100 rows: rel err {float(err):.3e}")
    assert err < ENGINE_TOL
    for rows in (5, 64, 80):                                    # native; native, 4 row blocks; scratch + coop
        toks = torch.randint(3, cfg.vocab_size - 1, (rows,), generator=g)
        hs = []
        for e in (e16, e4):
            slots = list(range(rows))
            for s_ in slots[1:]:
                e.seq_len[s_] = 0
            sl, po = e.prefill_rows(slots, [1] * rows)
            hs.append(e.forward(e.embed(toks.to(DEV)), sl, po).clone())
            e.advance(slots, [1] * rows)
        err = rel_err(hs[1], hs[0])
        print(f"{kind} int4 decode {rows} rows: rel err {float(err):.3e}")
        assert err < ENGINE_TOL, rows


def test_engine_refuses_k_not_multiple_of_128():
    cfg = tiny(layers=1, hidden=256, heads=4, kv_heads=2, head_dim=64, inter=320, vocab=512)
    with pytest.raises(ValueError, match="down"):
        make_stage_engine(cfg, 0, 1, DEV, torch.bfloat16, source=RandomSource(cfg, 0), weight_dtype="int4", load=False)


def test_decode_graph_and_sampler_on_int4_engine():
    cfg, e16, (e1, e2) = _engines("llama", n=2, max_slots=3)
    rows = 3
    prompts = [torch.tensor([1, 9, 8, 7]), torch.tensor([1, 100]), torch.tensor([1, 55, 44, 33, 22, 11])]
    firsts = []
    for e in (e1, e2):
        f = []
        for s, p in enumerate(prompts):
            sl, po = e.prefill_rows([s], [p.numel()])
            hh = e.forward(e.embed(p.to(DEV)), sl, po)
            e.advance([s], [p.numel()])
            f.append(int(e.head(hh, [p.numel() - 1])[0]))
        firsts.append(f)
    assert firsts[0] == firsts[1]
    toks, eager = torch.tensor(firsts[0]), []
    for _ in range(3):
        sl, po = e1.prefill_rows(list(range(rows)), [1] * rows)
        hh = e1.forward(e1.embed(toks.to(DEV)), sl, po)
        e1.advance(list(range(rows)), [1] * rows)
        toks = e1.head(hh).cpu()
        eager.append(toks.tolist())
    dg = DecodeGraph(e2, rows, "full", history_len=3)
    dg.tokens.copy_(torch.tensor(firsts[1], dtype=torch.int32))
    dg.capture()
    for _ in range(3):
        dg.replay()
    torch.cuda.synchronize()
    assert dg.history.cpu().tolist() == eager
    assert bool(((dg.history >= 0) & (dg.history < cfg.vocab_size)).all())
    # the bf16 head path is untouched: logits as the bf16 engine's, sampled tokens as the reference's
    h = torch.randn((6, cfg.hidden_size), generator=torch.Generator().manual_seed(2)).to(torch.bfloat16).to(DEV)
    smp = Sampler(e1)
    lg = smp.logits(h, list(range(6)))
    assert torch.equal(lg, Sampler(e16).logits(h, list(range(6))))
    params = [SamplingParams(0.7, top_p=0.9, seed=11), SamplingParams(1.0, top_k=50, seed=12), SamplingParams(0.0),
              SamplingParams(1.3, top_k=100, top_p=0.95, seed=14), SamplingParams(2.0, seed=15), SamplingParams(0.5, seed=16)]
    ctr = [4, 5, 6, 7, 8, 9]
    tok = smp.sample(h, list(range(6)), params, ctr).cpu().numpy()
    ref, kept, gap, _ = S.sample_reference(lg.cpu(), cfg.vocab_size, [p.temperature for p in params], [p.top_k for p in params],
                                           [p.top_p for p in params], [p.seed for p in params], ctr)
    must = (gap >= GAP_MIN) | np.array([p.greedy for p in params])
    assert kept[np.arange(6), tok].all() and must.sum() >= 4 and (tok[must] == ref[must]).all()
