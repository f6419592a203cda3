"""CPU side of the int4 (W4A16) weight path: the quantiser against the sharder's, the packed
layout's round trip, the conditions of the exact-case builders at every shape the GPU file uses
(tests/int4_cases.py), and the engine option on a CPU engine."""
import pytest
import torch

import contract_cases as C
import exact_cases as X
import int4_cases as I4
from llm_sharding_amd.config import tiny
from llm_sharding_amd.ops import int4, packing
from llm_sharding_amd.utils import model_sharder as MS


def _gauss(N, K, seed, scale=0.02):
    return torch.randn(N, K, generator=X.gen(seed)) * scale


@pytest.mark.parametrize("shape", [(16, 128), (48, 384), (64, 1024)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_quantiser_equals_sharder(shape, dtype):
    w = _gauss(*shape, seed=shape[1]).to(dtype)
    w[3] = 0                                                  # an all-zero group row: the clamp on the scale
    q, s = int4.quantize_int4_groups(w)
    packed, s_ref = MS.quantize_int4(w)
    lo, hi = (packed & 0xF).to(torch.int8), (packed >> 4).to(torch.int8)
    q_ref = torch.stack((lo, hi), dim=2).reshape(shape[0], -1)
    q_ref = torch.where(q_ref > 7, q_ref - 16, q_ref)
    assert q.dtype == torch.int8 and s.dtype == torch.float32 and s.shape == (shape[0], shape[1] // 128)
    assert torch.equal(q, q_ref) and torch.equal(C.bits(s), C.bits(s_ref.float()))
    assert int(q.abs().max()) <= 7
    assert torch.equal(int4.dequantize_int4_groups(q, s), MS.dequantize_int4(packed, s_ref))


def test_dequantise_inverts_quantise_on_the_grid():
    g = X.gen(3)
    q = X.randint(-7, 7, (32, 256), g, "cpu").to(torch.int8)
    q[:, 0], q[:, 128] = 7, -7                               # every group holds its extreme: amax / 7 = scale
    s = I4.group_scales(32, 256, g, "cpu") * 0.375           # not only powers of two
    w = int4.dequantize_int4_groups(q, s)
    assert torch.equal(w, (q.float().view(32, 2, 128) * s[:, :, None]).reshape(32, 256))
    q2, s2 = int4.quantize_int4_groups(w)
    assert torch.equal(q2, q) and torch.allclose(s2, s, rtol=2 ** -22, atol=0)


def test_quantisation_error_of_a_gaussian():
    """Mean relative error mean|w - dq(q(w))| / mean|w| of a 256 x 1024 Gaussian: 0.114 (the
    expected value for a step of amax / 7 over 128 Gaussians, amax about 2.8 sigma: uniform
    rounding noise of 0.4 sigma / sqrt(12) against mean|w| = 0.8 sigma). The cap of 0.2 is a
    sanity bound, not a tolerance."""
    w = _gauss(256, 1024, seed=11)
    q, s = int4.quantize_int4_groups(w)
    err = float((w - int4.dequantize_int4_groups(q, s)).abs().mean() / w.abs().mean())
    print(f"int4 group-128 mean relative error {err:.4f}")
    assert 0.05 < err < 0.2


@pytest.mark.parametrize("N", [16, 48])
@pytest.mark.parametrize("K", [128, 384])
def test_pack_round_trip(N, K):
    for q in (I4.all_codes(N, K), X.randint(-7, 7, (N, K), X.gen(N + K), "cpu").to(torch.int8)):
        p = int4.pack_b_int4(q)
        assert p.dtype == torch.uint8 and p.shape == (N * K // 2,)
        assert torch.equal(int4.unpack_b_int4(p, N, K), q)
    sc = I4.group_scales(N, K, X.gen(1), "cpu")
    ps = int4.pack_scales_int4(sc)
    assert ps.shape == (N // 16, K // 128, 16) and torch.equal(int4.unpack_scales_int4(ps), sc)


def test_packed_layout_is_the_documented_one():
    """Wq4[nt][g][lane][dword h] holds fragment 4g + h of pack_b; inside the dword (rotated right
    by 3) element 2p sits at nibble p and element 2p + 1 at nibble p + 4, offset by 8."""
    N, K = 32, 256
    q = X.randint(-7, 7, (N, K), X.gen(5), "cpu").to(torch.int8)
    frag = packing.pack_b(q)                                   # [nt, kt, lane, 8]
    by = int4.pack_b_int4(q).view(N // 16, K // 128, 64, 4, 4).long()
    d = by[..., 0] | (by[..., 1] << 8) | (by[..., 2] << 16) | (by[..., 3] << 24)
    d = ((d >> 3) | (d << 29)) & 0xFFFFFFFF
    for nt, g, lane, h in ((0, 0, 0, 0), (1, 1, 37, 3), (0, 1, 63, 2), (1, 0, 16, 1)):
        el = frag[nt, 4 * g + h, lane].long() + 8
        want = sum(int(el[2 * p]) << (4 * p) | int(el[2 * p + 1]) << (4 * p + 16) for p in range(4))
        assert int(d[nt, g, lane, h]) == want


def test_bad_shapes_raise():
    with pytest.raises(ValueError):
        int4.quantize_int4_groups(torch.zeros(16, 192))
    with pytest.raises(ValueError):
        int4.quantize_int4_groups(torch.zeros(16, 64))     # no gcd fallback
    with pytest.raises(ValueError):
        int4.pack_b_int4(torch.zeros(16, 160, dtype=torch.int8))
    with pytest.raises(ValueError):
        int4.pack_b_int4(torch.zeros(8, 128, dtype=torch.int8))
    with pytest.raises(ValueError):
        int4.pack_b_int4(torch.full((16, 128), -8, dtype=torch.int8))
    with pytest.raises(ValueError):
        int4.unpack_b_int4(torch.zeros(100, dtype=torch.uint8), 16, 128)


def test_configs():
    assert len(set(int4.INT4_CONFIGS)) == len(int4.INT4_CONFIGS)
    assert {b for _, b, _, _ in int4.INT4_CONFIGS} == {1, 2, 4}
    # every Llama-2-7B projection at 1, 16 and 64 rows: a built config, >= 256 workgroups
    for n, k, even in ((12288, 4096, False), (4096, 4096, False), (22016, 4096, True), (4096, 11008, False)):
        for rows in (1, 16, 17, 64):
            tn, nw, ug = int4.int4_config(n // 16, rows, even, k)
            assert (tn, packing.row_blocks(rows), nw, ug) in int4.INT4_CONFIGS
            assert n // 16 // tn >= 256 and (not even or tn % 2 == 0)
    assert int4.int4_gemv_candidates(48, 384, 65) == []
    assert int4.int4_bytes(4096, 4096) * 8 == 4096 * 4096 * 4.25
    # every built config has a shape in the GPU file's sweep
    for tn, mb, nw, ug in int4.INT4_CONFIGS:
        assert any((tn, nw, ug) in int4.int4_gemv_candidates(I4.n_for(tn) // 16, K, M, tn % 2 == 0)
                   for M in I4.ROWS for K in I4.KS if packing.row_blocks(M) == mb)


@pytest.mark.parametrize("K", I4.KS)
@pytest.mark.parametrize("M", I4.ROWS)
def test_exact_builders(M, K):
    """The conditions of every case of tests/test_int4_gpu.py hold (partial sums below 2^24,
    the gate window, the tie and double-rounding shares), and the references are self-consistent."""
    for tn in (1, 2, 4):
        N = I4.n_for(tn)
        c = I4.case("linear", M, N, K)
        assert c.W.ref.shape == (N, K) and int(c.W.q.min()) == -7 and int(c.W.q.max()) == 7
        assert torch.equal(int4.unpack_b_int4(c.W.wq, N, K), c.W.q)
        assert set(c.W.scale.unique().tolist()) <= set(I4.INT4_SCALES)
        # group by group in fp32, as the kernel accumulates: the same value
        acc = torch.zeros(M, N)
        for g in range(K // 128):
            sl = slice(128 * g, 128 * (g + 1))
            acc = acc + c.W.scale[:, g][None, :] * (c.a[:, sl].float() @ c.W.q[:, sl].float().T)
        assert torch.equal(acc.double(), c.y)
    if K >= I4.K_ROUND_MIN:
        for tn in (1, 2):
            I4.case("round_once", M, I4.n_for(tn), K)
        r = I4.case("round_once", M, I4.n_for(4), K)
        print(f"{r.tag}: ties {r.stats['tie_share']:.2%}, double rounding {r.stats['double_rounding_share']:.2%}")
    s = I4.case("swiglu", M, I4.n_for(2) // 2, K)
    assert s.exp.shape == (M, I4.n_for(2) // 2)
    for rope in (True, False):
        qc = I4.case("qkv", M, K, rope)
        assert qc.N == 192 and qc.exp_q.shape == (M, 128)
    n = I4.case("norm", M, I4.n_for(1), K)
    assert bool((n.a.float().pow(2).mean(-1) == 4).all())


def test_one_hot_and_gelu_builders():
    c = I4.case("one_hot")
    assert c.exp.shape == (128, 16) and torch.equal(c.exp.double(), c.W.ref.T)
    assert sorted(c.W.q.unique().tolist()) == list(range(-7, 8))
    for M in I4.ROWS:
        for K in I4.KS:
            for tn in (1, 2, 4):
                g = I4.case("gelu", M, I4.n_for(tn), K)
                assert g.exact.shape == (M, I4.n_for(tn))


def test_checker_sees_one_wrong_nibble():
    c = I4.case("linear", 7, 48, 384)
    q = c.W.q.clone()
    q[5, 200] = q[5, 200] - 1 if q[5, 200] > -7 else q[5, 200] + 1
    y = X.matmul(c.a, int4.dequantize_int4_groups(q, c.W.scale))
    with pytest.raises(AssertionError):
        X.assert_bits_equal(y.float(), c.y.float(), "one nibble off")


def test_engine_option_on_cpu():
    from llm_sharding_amd.runtime.engine import RandomSource, StageEngine
    from llm_sharding_amd.runtime.engine_int4 import Int4StageEngine, make_stage_engine
    cfg = tiny()
    kw = dict(has_embed=True, has_head=True, source=RandomSource(cfg, 0), max_slots=2, max_seq=32)
    with pytest.raises(ValueError):
        StageEngine(cfg, 0, cfg.num_hidden_layers, "cpu", torch.float32, weight_dtype="int5", **kw)
    e16 = StageEngine(cfg, 0, cfg.num_hidden_layers, "cpu", torch.float32, **kw)
    with pytest.raises(ValueError):
        make_stage_engine(cfg, 0, cfg.num_hidden_layers, "cpu", torch.float32, weight_dtype="int5", **kw)
    e4 = make_stage_engine(cfg, 0, cfg.num_hidden_layers, "cpu", torch.float32, weight_dtype="int4", **kw)
    assert type(e4) is Int4StageEngine and type(make_stage_engine(cfg, 0, 1, "cpu", torch.float32, load=False)) is StageEngine
    assert not e4.int4 and e4.lm_head_s is None and e4.memory_bytes() == e16.memory_bytes()
    ids = torch.arange(1, 9)
    outs = []
    for e in (e16, e4):
        slot, pos = e.prefill_rows([0], [ids.numel()])
        outs.append(e.forward(e.embed(ids), slot, pos))
    assert torch.equal(outs[0], outs[1])


def test_int4_forward_is_the_base_forward_with_int4_weight_closures():
    """Int4StageEngine._forward_hip / _forward_hip_gpt2 are StageEngine's bodies; only the lines
    that choose a kernel by the weight kind differ (the base's fp8 lines against int4 ones), so
    every other route (fused RMSNorm sums, split-K partials, attention) is the base engine's, and
    a change of the base forward fails here until it is carried over."""
    import difflib
    import inspect
    from llm_sharding_amd.runtime.engine import StageEngine
    from llm_sharding_amd.runtime.engine_int4 import Int4StageEngine
    for name in ("_forward_hip", "_forward_hip_gpt2"):
        a = inspect.getsource(getattr(StageEngine, name)).splitlines()
        b = inspect.getsource(getattr(Int4StageEngine, name)).splitlines()
        changed = [ln for ln in difflib.unified_diff(a, b, lineterm="", n=0) if not ln.startswith(("---", "+++", "@@"))]
        assert 0 < len(changed) <= 16, (name, changed)
        for ln in changed:
            body = ln[1:].strip()
            if ln[0] == "-":
                assert not body or "fp8" in body, (name, ln)
            else:
                assert "int4" in body or "_weights_bf16" in body, (name, ln)


def test_stage_memory_counts_int4():
    from llm_sharding_amd.config import get_preset
    from llm_sharding_amd.parallel.scheduler import stage_memory
    cfg = get_preset("llama2-7b")
    kw = dict(slots=1, max_seq=128, prefill_rows=0)
    m16, m4 = stage_memory(cfg, 32, **kw), stage_memory(cfg, 32, weight_dtype="int4", **kw)
    proj = 32 * sum(n * k for n, k in ((12288, 4096), (4096, 4096), (22016, 4096), (4096, 11008)))
    assert m16["weights"] - m4["weights"] == proj * (16 - 4.25) / 8
    assert abs(m4["weights"] - 3.44e9) < 0.02e9                      # the issue's 3.44 GB of layer weights
    assert m4["scratch"] - m16["scratch"] == 2 * 22016 * 4096
    assert stage_memory(cfg, 32, weight_dtype="fp8", **kw) == m16        # fp8 is not modelled (as before)
