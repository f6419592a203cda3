"""CPU side of the fp8 KV cache (kv_dtype="fp8"): the format's torch references (ops/kv8.py), the
preconditions of the GPU tests (tests/kv8_cases.py), the engine option on a CPU engine, the pin of
Fp8KVStageEngine's forward body to the base engine's, and the scheduler's memory model."""
import math

import pytest
import torch

import contract_cases as C
import kv8_cases as K8
from llm_sharding_amd.config import get_preset, tiny
from llm_sharding_amd.ops import kv8


def _f8(codes):
    return codes.view(torch.float8_e4m3fn).float()


def _bound_ok(x, codes, s):
    """|dequant - x| <= max(|x| * 2^-4, s * 2^-10): half an ulp of a 3-bit mantissa, or half the
    smallest e4m3 step (2^-9) at the vector's scale."""
    xf = x.float()
    err = (kv8.dequantize_reference(codes, s).float() - xf).abs()
    return bool((err <= torch.maximum(xf.abs() * 2.0 ** -4, s[..., None] * 2.0 ** -10)).all())


def test_scales_are_powers_of_two_and_codes_fill_the_top_octave():
    g = torch.Generator().manual_seed(0)
    for hd in (64, 128):
        x = (torch.randn(2048, hd, generator=g) * torch.rand(2048, 1, generator=g) * 3).to(torch.bfloat16)
        codes, s = kv8.quantize_reference(x)
        assert codes.dtype == torch.uint8 and s.dtype == torch.float32 and s.shape == (2048,)
        m, e = torch.frexp(s)
        assert bool((m == 0.5).all())                                # powers of two
        top = _f8(codes).abs().amax(-1)
        assert float(top.min()) >= 128 and float(top.max()) <= 256
        assert not bool(((codes & 0x7F) == K8.NAN_CODE).any())       # the NaN code never appears
        assert _bound_ok(x, codes, s)


def test_zero_vector():
    codes, s = kv8.quantize_reference(torch.zeros(3, 64, dtype=torch.bfloat16))
    assert bool((s == 1).all()) and bool((codes == 0).all())
    assert bool((kv8.dequantize_reference(codes, s) == 0).all())


def test_error_bound_over_forty_octaves():
    g = torch.Generator().manual_seed(1)
    mag = 2.0 ** (torch.rand(4096, 128, generator=g) * 40 - 20)      # magnitudes 2^-20 .. 2^20 inside one vector
    x = (mag * torch.where(torch.rand(4096, 128, generator=g) < 0.5, -1.0, 1.0)).to(torch.bfloat16)
    codes, s = kv8.quantize_reference(x)
    assert _bound_ok(x, codes, s)
    top = _f8(codes).abs().amax(-1)
    assert float(top.min()) >= 128 and float(top.max()) <= 256


def test_every_finite_bf16_pattern():
    """The GPU append test's inputs: all 65280 patterns are there, the reference holds its bound on
    them, and the scale clamp keeps s and 1 / s normal down to the bf16 denormals."""
    for hd in (64, 128):
        pool, n_pat = K8.vector_pool(hd)
        pat = pool[:n_pat].reshape(-1).view(torch.int16).to(torch.int32) & 0xFFFF
        assert torch.equal(torch.bincount(pat, minlength=1 << 16)[(torch.arange(1 << 16) & 0x7F80) != 0x7F80],
                           torch.full((65280,), 2))
        codes, s = kv8.quantize_reference(pool)
        assert float(s.min()) == 2.0 ** -126 and bool(torch.isfinite(1 / s).all())
        assert not bool(((codes & 0x7F) == K8.NAN_CODE).any())
        big = pool.float().abs().amax(-1) >= 2.0 ** -119              # above the clamp: the top octave is used
        assert float(_f8(codes[big]).abs().amax(-1).min()) >= 128
        # the bound is the format's wherever dequantisation is exact: every non-zero code * s, the
        # smallest being 2^-9 * s, is a bf16 normal, and below the one overflow: a code of 256 at the
        # largest scale, 2^120, is 2^128 (the round-robin vectors all sit at that scale)
        norm = (s >= 2.0 ** -117) & (s < 2.0 ** 120)
        assert int(norm.sum()) > 0.4 * s.numel() and _bound_ok(pool[norm], codes[norm], s[norm])
        top = pool[s == 2.0 ** 120].float().abs()
        assert bool(torch.isinf(kv8.dequantize_reference(*kv8.quantize_reference(pool[s == 2.0 ** 120])).float()
                                [top >= 248 * 2.0 ** 120]).all())


def test_non_finite_and_wrong_dtype_are_refused():
    x = torch.zeros(2, 64, dtype=torch.bfloat16)
    x[1, 3] = float("inf")
    with pytest.raises(ValueError):
        kv8.quantize_reference(x)
    with pytest.raises(ValueError):
        kv8.quantize_reference(torch.zeros(2, 64))


@pytest.mark.parametrize("hd", [64, 128])
def test_membership_caches_round_trip_bit_exactly(hd):
    """The precondition of the GPU membership tests: the exact-membership K / V patterns are
    representable, so the kernel under test sees exactly the values check_membership decodes."""
    case = C.build_membership_case(8, 2, hd, C.membership_lengths(hd))
    k8, v8, ks, vs = K8.quantize_cache(case.K, case.V)
    for r, T in enumerate(case.lens):
        s = int(case.slot[r])
        for t, c8, sc in ((case.K, k8, ks), (case.V, v8, vs)):
            back = kv8.dequantize_reference(c8[s, :, :T], sc[s, :, :T])
            assert torch.equal(C.bits(back), C.bits(t[s, :, :T])), (hd, r)
            assert bool((c8[s, :, T:] == K8.NAN_CODE).all()) and bool(torch.isnan(sc[s, :, T:]).all())


def test_attn_reference_equals_the_bf16_reference_on_an_exact_cache():
    case = C.build_membership_case(8, 2, 64, [1, 17, 300])
    k8, v8, ks, vs = K8.quantize_cache(case.K, case.V)
    q = torch.randn(3, 8 * 64, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16)
    ref = kv8.attn_decode_reference(q, k8, v8, ks, vs, case.slot, case.lens, 8)
    assert torch.equal(ref, C.attention_reference(q, case))


def test_engine_option_on_cpu():
    from llm_sharding_amd.runtime.engine import RandomSource, StageEngine
    from llm_sharding_amd.runtime.engine_int4 import make_stage_engine
    cfg = tiny()
    kw = dict(has_embed=True, has_head=True, source=RandomSource(cfg, 0), max_slots=2, max_seq=32)
    e16 = make_stage_engine(cfg, 0, cfg.num_hidden_layers, "cpu", torch.float32, **kw)
    e8 = make_stage_engine(cfg, 0, cfg.num_hidden_layers, "cpu", torch.float32, kv_dtype="fp8", **kw)
    assert type(e16) is StageEngine and isinstance(e8, StageEngine) and e8.memory_bytes() == e16.memory_bytes()
    ids = torch.arange(1, 9)
    outs = []
    for e in (e16, e8):
        slot, pos = e.prefill_rows([0], [ids.numel()])
        outs.append(e.forward(e.embed(ids), slot, pos))
    assert torch.equal(outs[0], outs[1])
    for bad in ("fp16", "int8", "", None):
        with pytest.raises(ValueError):
            make_stage_engine(cfg, 0, cfg.num_hidden_layers, "cpu", torch.float32, kv_dtype=bad, **kw)
    with pytest.raises(ValueError):
        make_stage_engine(cfg, 0, cfg.num_hidden_layers, "cpu", torch.float32, kv_dtype="fp8", weight_dtype="int4", **kw)


def test_server_refuses_a_prefix_pool_on_fp8_kv():
    from llm_sharding_amd.parallel.server import PipelineServer
    from llm_sharding_amd.runtime.engine import RandomSource
    cfg = tiny(layers=1)
    with pytest.raises(ValueError, match="prefix_slots"):
        PipelineServer(cfg, RandomSource(cfg, 0), device="cpu", batch=1, max_seq=32, prefix_slots=1, kv_dtype="fp8")
    with pytest.raises(ValueError, match="kv_dtype"):
        PipelineServer(cfg, RandomSource(cfg, 0), device="cpu", batch=1, max_seq=32, kv_dtype="fp4")


def test_kv8_forward_is_the_base_forward_with_the_kv8_calls():
    """Fp8KVStageEngine._forward_hip is StageEngine's body: only the lines that name the kv8 calls
    (prefix restore, append, decode attention) and the attn_oproj switch differ, so every projection
    route is the base engine's, and a change of the base forward fails here until it is carried over."""
    import difflib
    import inspect
    from llm_sharding_amd.runtime.engine import StageEngine
    from llm_sharding_amd.runtime.engine_kv8 import Fp8KVStageEngine
    a = inspect.getsource(StageEngine._forward_hip).splitlines()
    b = inspect.getsource(Fp8KVStageEngine._forward_hip).splitlines()
    changed = [ln for ln in difflib.unified_diff(a, b, lineterm="", n=0) if not ln.startswith(("---", "+++", "@@"))]
    assert 0 < len(changed) <= 12, changed
    removed = [ln[1:].strip() for ln in changed if ln[0] == "-"]
    added = [ln[1:].strip() for ln in changed if ln[0] == "+"]
    assert len(removed) == 3, removed                         # the two-line ao switch, the hip.attn line
    for body in removed:
        assert "ATTN_OPROJ" in body or "ao_sync is not None" in body or "hip.attn(" in body, body
    for body in added:
        assert "kv8" in body, body
    assert sum("kv8.attn(" in x for x in added) == 1 and sum("kv8.kv8_append(" in x for x in added) == 1
    assert sum("kv8.kv8_dequant(" in x for x in added) == 1 and "ao = False  # kv8: attn_oproj reads a bf16 cache" in added


def test_scheduler_counts_the_fp8_cache():
    from llm_sharding_amd.parallel.scheduler import kv_slots_for_memory, kv_token_bytes, stage_memory
    cfg = get_preset("llama2-7b")
    assert kv_token_bytes(cfg) == 16384 and kv_token_bytes(cfg, kv_dtype="fp8") == 8448 == kv8.kv8_token_bytes(32, 128)
    kw = dict(slots=512, max_seq=2048, prefill_rows=2048)
    m16, m8 = stage_memory(cfg, 32, **kw), stage_memory(cfg, 32, kv_dtype="fp8", **kw)
    assert m16 == stage_memory(cfg, 32, kv_dtype="bf16", **kw)
    assert m16["kv"] == 32 * 16384 * 512 * 2048 and m8["kv"] == 32 * 8448 * 512 * 2048
    assert m8["scratch"] - m16["scratch"] == 16384 * 512 * 2048      # one bf16 staging layer
    assert m8["weights"] == m16["weights"] and m8["io"] == m16["io"]
    assert m8["total"] == m8["weights"] + m8["kv"] + m8["scratch"] + m8["io"]
    with pytest.raises(ValueError):
        stage_memory(cfg, 32, kv_dtype="int8", **kw)
    # slots: the default call is today's formula; fp8 charges the staging layer to the slots it serves
    mem, w, T = 288e9, 13.5e9, 2048
    args = dict(reserve_bytes=8e9, max_per_microbatch=10 ** 6)
    free = mem - 8e9 - w
    assert kv_slots_for_memory(cfg, 32, T, mem, w, **args) == int(free // (16384.0 * 32 * T))
    n8 = kv_slots_for_memory(cfg, 32, T, mem, w, kv_dtype="fp8", **args)
    assert n8 == int(free // ((8448.0 * 32 + 16384.0) * T))
    assert n8 > 1.8 * kv_slots_for_memory(cfg, 32, T, mem, w, **args)
    assert math.isclose(stage_memory(cfg, 32, slots=1, max_seq=2048, prefill_rows=0)["kv"], 1.07e9, rel_tol=5e-3)


@pytest.mark.parametrize("max_seq", [2048, 4096])
def test_server_sizing_hands_out_the_slots_fp8_frees(max_seq):
    """serve.py's sizing (scheduler.size_kv_slots: slots from HBM, then a plan priced by the same
    cache format, to a fixed point) for llama2-7b on one 288 GB device with two micro-batches of at
    most 128 slots: the fp8 plan exists, holds more slots than the bf16 one, and fits the device."""
    from llm_sharding_amd.parallel import scheduler as S
    cfg = get_preset("llama2-7b")
    mem, M = 288e9, 2
    reserve = 8e9 + S.scratch_bytes(cfg, 2048, sets=1)
    got = {}
    for kvd in ("bf16", "fp8"):
        batch, plan = S.size_kv_slots(cfg, 1, max_seq, mem, reserve, M, 0, kvd)
        st = plan.stages[0]
        assert plan.ranges() == [(0, 32)] and st.kv_bytes == 32 * S.kv_token_bytes(cfg, 2, kvd) * max_seq * batch * M
        staging = 16384 * max_seq * batch * M if kvd == "fp8" else 0
        assert st.weight_bytes + st.kv_bytes + staging <= mem - 8e9
        got[kvd] = batch
    assert got["bf16"] == {2048: 123, 4096: 61}[max_seq]            # what the bf16 sizing gave before
    assert got["fp8"] > got["bf16"] and (got["fp8"] == 128 or got["fp8"] > 1.8 * got["bf16"])
    # the default call prices bf16: an fp8 slot count that bf16 cannot hold is refused without the format
    if got["fp8"] * 16384 * 32 * max_seq * M + 13.5e9 > mem - 8e9:
        with pytest.raises(ValueError, match="does not fit"):
            S.plan_stages(cfg, 1, kv_tokens=max_seq * got["fp8"] * M)
    # a prefix pool's slots come out of the same budget
    b_pool, _ = S.size_kv_slots(cfg, 1, max_seq, mem, reserve, M, 4, "bf16")
    assert b_pool == (got["bf16"] * M - 4) // M
