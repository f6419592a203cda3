"""The MXFP4 weight format on the CPU (ops/mx4.py): quantiser, exact dequantisation, packers, the
activation quantiser's contract, and the engine option's wiring."""
import pytest
import torch

from llm_sharding_amd.config import get_preset, tiny, tiny_gpt2
from llm_sharding_amd.ops import kv8, mx4


@pytest.mark.parametrize("eb", [-140, -125, -3, 0, 5, 125])
def test_quantize_every_code_and_exponent(eb):
    """A block holding all 16 code values at scale 2^eb comes back as those codes and that
    exponent (clamped to the bf16-normal range), and dequantises to itself through bf16."""
    vals = torch.tensor(mx4.E2M1 + tuple(-v for v in mx4.E2M1), dtype=torch.float64).repeat(2) * 2.0 ** max(eb, -126)
    w = vals.float().view(1, 32)
    q, e = mx4.quantize_mx4(w)
    ec = min(max(eb, mx4.MX_EB_MIN), mx4.MX_EB_MAX)
    assert int(e[0, 0]) == ec + 127
    d = mx4.dequantize_mx4(q, e)
    assert d.dtype == torch.bfloat16 and bool(torch.isfinite(d).all())
    assert torch.equal(d.double().float().to(torch.bfloat16), d)
    if ec == eb:
        assert torch.equal(q[0, :16], torch.tensor([0, 1, 2, 3, 4, 5, 6, 7, 0, 9, 10, 11, 12, 13, 14, 15], dtype=torch.uint8))
        assert torch.equal(d.double().view(-1), vals)
    nz = d.float().abs()[d != 0]
    assert nz.numel() == 0 or float(nz.min()) >= 2.0 ** -126  # bf16 normals only


def test_quantize_rounding_saturation_and_zero_block():
    w = torch.zeros(2, 32)
    w[0, :9] = torch.tensor([4.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, -0.25, 0.3])  # amax 4: eb = 0; ties to the even code
    w[1, 32 - 1] = 0.0
    q, e = mx4.quantize_mx4(w)
    assert q[0, :9].tolist() == [6, 0, 2, 2, 4, 4, 6, 8, 1] and e.tolist() == [[127], [127]]
    assert not bool(q[1].any())
    q, e = mx4.quantize_mx4(torch.tensor([[7.9] + [5.1] * 31]))  # amax 7.9: eb = 0, 7.9 saturates at 6, 5.1 -> 6
    assert int(e) == 127 and q.tolist() == [[7] * 32]


@pytest.mark.parametrize("steps", [1, 3, 5])
def test_pack_unpack_inverses(steps):
    N, K = 48, 128 * steps
    g = torch.Generator().manual_seed(steps)
    q = torch.randint(0, 16, (N, K), generator=g).to(torch.uint8)
    e = torch.randint(2, 253, (N, K // 32), generator=g).to(torch.uint8)
    p, s = mx4.pack_b_mx4(q), mx4.pack_scales_mx4(e)
    assert p.numel() == N * K // 2 and s.numel() == N * mx4.scale_groups(K) * 16
    assert torch.equal(mx4.unpack_b_mx4(p, N, K), q) and torch.equal(mx4.unpack_scales_mx4(s, N, K), e)
    # lane 16 * block + column of tile 2, K-step steps - 1: byte 5 holds elements 10 and 11
    lane = p.view(N // 16, steps, 64, 16)[2, steps - 1, 16 * 3 + 7]
    k0 = 128 * (steps - 1) + 32 * 3
    assert int(lane[5]) == int(q[39, k0 + 10]) | (int(q[39, k0 + 11]) << 4)
    assert int(s.view(N // 16, -1, 64, 4)[2, (steps - 1) // 4, 16 * 3 + 7, (steps - 1) % 4]) == int(e[39, 4 * (steps - 1) + 3])
    assert mx4.mx4_bytes(N, K) * 8 == 4.25 * N * K


def test_quantize_act_is_the_kv8_convention():
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(6, 96, generator=g) * torch.logspace(-3, 3, 6)[:, None]).to(torch.bfloat16)
    x[1, 32:64] = 0
    x[2, :32] = 2.0 ** -130
    codes, e = mx4.quantize_act_mx8(x)
    for b in range(3):
        c, s = kv8.quantize_reference(x[:, 32 * b:32 * b + 32])
        assert torch.equal(codes[:, 32 * b:32 * b + 32], c)
        assert torch.equal((e[:, b].to(torch.int32) << 23).view(torch.float32), s)
    assert int(e.max()) < 255 and not bool(((codes & 0x7F) == 0x7F).any())
    q, eb = mx4.quantize_mx4(torch.randn(16, 96, generator=g))
    want = mx4.dequantize_act_mx8(codes, e) @ mx4.dequantize_mx4(q, eb).double().t()
    assert torch.equal(mx4.linear_reference(x, q, eb), want)


def test_forward_is_the_base_forward_with_mx4_weight_closures():
    """Mx4StageEngine._forward_hip is StageEngine's body; only the lines that choose a kernel by the
    weight kind differ, so a change of the base forward fails here until it is carried over."""
    import difflib
    import inspect
    from llm_sharding_amd.runtime.engine import StageEngine
    from llm_sharding_amd.runtime.engine_mx4 import Mx4StageEngine
    a = inspect.getsource(StageEngine._forward_hip).splitlines()
    b = inspect.getsource(Mx4StageEngine._forward_hip).splitlines()
    changed = [ln for ln in difflib.unified_diff(a, b, lineterm="", n=0) if not ln.startswith(("---", "+++", "@@"))]
    assert 0 < len(changed) <= 14, changed
    for ln in changed:
        body = ln[1:].strip()
        if ln[0] == "-":
            assert not body or "fp8" in body, ln
        else:
            assert "mx4" in body or "mxfp4" in body or "_weights_bf16" in body, ln


def test_engine_option_and_refusals():
    from llm_sharding_amd.runtime.engine import RandomSource, StageEngine
    from llm_sharding_amd.runtime.engine_int4 import make_stage_engine
    from llm_sharding_amd.runtime.engine_mx4 import Mx4StageEngine
    cfg = tiny()
    kw = dict(has_embed=True, has_head=True, source=RandomSource(cfg, 0), max_slots=2, max_seq=32)
    e16 = StageEngine(cfg, 0, cfg.num_hidden_layers, "cpu", torch.float32, **kw)
    e4 = make_stage_engine(cfg, 0, cfg.num_hidden_layers, "cpu", torch.float32, weight_dtype="mxfp4", **kw)
    assert type(e4) is Mx4StageEngine and not e4.mx4 and e4.memory_bytes() == e16.memory_bytes()  # ignored on the CPU
    ids = torch.arange(1, 9)
    outs = []
    for e in (e16, e4):
        slot, pos = e.prefill_rows([0], [ids.numel()])
        outs.append(e.forward(e.embed(ids), slot, pos))
    assert torch.equal(outs[0], outs[1])
    for bad in (dict(kv_dtype="fp8"), dict(kv_layout="paged", kv_pages=4)):
        with pytest.raises(ValueError, match="mxfp4"):
            make_stage_engine(cfg, 0, 1, "cpu", torch.float32, weight_dtype="mxfp4", load=False, **bad)
    g2 = tiny_gpt2()
    with pytest.raises(NotImplementedError):
        Mx4StageEngine(g2, 0, 1, "cuda", torch.bfloat16, source=RandomSource(g2, 0), load=False)
    odd = tiny(layers=1, hidden=256, heads=4, kv_heads=2, head_dim=64, inter=320, vocab=512)
    with pytest.raises(ValueError, match="down"):
        Mx4StageEngine(odd, 0, 1, "cuda", torch.bfloat16, source=RandomSource(odd, 0), load=False)


def test_stage_memory_counts_mxfp4():
    from llm_sharding_amd.parallel.scheduler import stage_memory
    cfg = get_preset("llama2-7b")
    kw = dict(slots=1, max_seq=128, prefill_rows=0)
    m16, m4 = stage_memory(cfg, 32, **kw), stage_memory(cfg, 32, weight_dtype="mxfp4", **kw)
    proj = 32 * sum(n * k for n, k in ((12288, 4096), (4096, 4096), (22016, 4096), (4096, 11008)))
    assert m16["weights"] - m4["weights"] == proj * (16 - 4.25) / 8
    assert m4["scratch"] - m16["scratch"] == 2 * 22016 * 4096
