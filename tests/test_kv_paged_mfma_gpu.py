"""lsa_attn_decode_mfma_paged (csrc/cache/kv_paged.hip) against lsa_attn_decode_mfma on the static cache the
pages were cut from, on raw bits (NaN wherever a row must not read); then the routing and the paged engine."""
import pytest
import torch

import kv_paged_cases as K
from llm_sharding_amd.config import tiny
from llm_sharding_amd.ops import hip
from llm_sharding_amd.ops import kv_paged as KP
from llm_sharding_amd.utils.numerics import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
_CASES = {}


def _case(hd, g):
    if (hd, g) not in _CASES:
        _CASES[(hd, g)] = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in K.attn_case(hd, g).items()}
    return _CASES[(hd, g)]


def _i32(x):
    return torch.tensor(list(x), dtype=torch.int32, device=DEV)


def _lens(lens, form):
    return (_i32([n - 1 for n in lens]), None) if form == "pos" else (_i32([0] * len(lens)), _i32(lens))


def _out(rows, c, extra=0):
    return torch.full((rows + extra, c["n_heads"] * c["hd"]), 7.0, dtype=torch.bfloat16, device=DEV)


def _static(c, slot, lens, form, nw):
    rows, (pos, kvl), out = len(slot), _lens(lens, form), _out(len(slot), c)
    rc = hip.lib().lsa_attn_decode_mfma(hip._p(c["q"]), c["q"].stride(0), hip._p(c["k"]), hip._p(c["v"]), hip._p(_i32(slot)),
                                        hip._p(pos), hip._p(kvl), rows, c["n_heads"], c["n_kv"], c["hd"], K.ATTN_MAX_SEQ,
                                        float(c["hd"] ** -0.5), hip._p(out), out.stride(0), nw, hip._stream())
    assert rc == 0
    return out


def _paged(c, slot, lens, form, nw):
    rows, (pos, kvl), out = len(slot), _lens(lens, form), _out(len(slot), c)
    KP.attn_paged_mfma(c["q"], c["kp"], c["vp"], c["table"], _i32(slot), pos, rows, c["n_heads"], c["n_kv"], c["hd"], out,
                       kv_len=kvl, nw=nw)
    return out


@pytest.mark.parametrize("rows", [1, 7, 129])
@pytest.mark.parametrize("nw", [1, 2, 4])
@pytest.mark.parametrize("g", [2, 3, 4, 8])
@pytest.mark.parametrize("hd", [64, 128])
def test_equals_the_static_mfma_kernel_bit_for_bit(hd, g, nw, rows):
    """Contexts 1 / 63 / 64 / 65 / 130 / 1100 and shorter prefixes mixed across the rows. The static result is
    finite although everything beyond a context is NaN: equal bits also prove that only the row's keys were read."""
    c, cpu = _case(hd, g), K.attn_case(hd, g)
    launches = [K.attn_rows(1, first=s) for s in range(len(K.CONTEXTS))] if rows == 1 else [K.attn_rows(rows)]
    for slot, lens in launches:
        assert K.live_pages_assigned(cpu["table"], slot, lens, cpu["n_pages"])
        for form in ("pos", "kv_len"):
            static, paged = _static(c, slot, lens, form, nw), _paged(c, slot, lens, form, nw)
            assert bool(torch.isfinite(static.float()).all()), (form, slot, lens)
            assert torch.equal(K.bits(paged), K.bits(static)), (form, slot, lens[:6])


def test_is_the_reference_attention():
    c, cpu, (slot, lens) = _case(128, 4), K.attn_case(128, 4), K.attn_rows(7)   # (test_attn_gqa_gpu.py's bound)
    ref = K.attn_reference(cpu["q"], torch.nan_to_num(cpu["kp"]), torch.nan_to_num(cpu["vp"]), cpu["table"], slot, lens,
                           cpu["n_heads"])
    err = rel_err(_paged(c, slot, lens, "pos", 0).cpu(), ref.float())
    assert err < 1e-2, err


def _routed(c, slot, lens, paged, mfma=True):
    rows, nh, nkv, hd = len(slot), c["n_heads"], c["n_kv"], c["hd"]
    po, pl = torch.zeros(rows * nh * 4 * hd, device=DEV), torch.zeros(rows * nh * 4, device=DEV)
    cnt, out, (pos, _) = torch.zeros(rows * nkv, dtype=torch.int32, device=DEV), _out(rows, c), _lens(lens, "pos")
    prev, hip.ATTN_MFMA = hip.ATTN_MFMA, mfma
    try:
        if paged:
            KP.attn_paged(c["q"], c["kp"], c["vp"], c["table"], _i32(slot), pos, rows, nh, nkv, hd, 4, po, pl, out, counters=cnt)
        else:
            hip.attn(c["q"], c["k"], c["v"], _i32(slot), pos, rows, nh, nkv, hd, 4, po, pl, out, counters=cnt)
    finally:
        hip.ATTN_MFMA = prev
    return out


def test_attn_paged_takes_hip_attns_route():
    (slot, lens), c4, c1 = K.attn_rows(129), _case(128, 4), _case(128, 1)
    split4, split1 = _routed(c4, slot, lens, True), _routed(c1, slot, lens, True)         # 258 items < 512: split-KV
    prev, hip.ATTN_MFMA_MIN_ITEMS = hip.ATTN_MFMA_MIN_ITEMS, 129 * c4["n_kv"]
    try:
        mfma = _routed(c4, slot, lens, True)
        assert torch.equal(mfma, _routed(c4, slot, lens, False)) and torch.equal(mfma, _static(c4, slot, lens, "pos", 0))
        assert not torch.equal(mfma, split4)                                              # (another summation order)
        assert torch.equal(_routed(c4, slot, lens, True, mfma=False), split4)             # the switch
        assert torch.equal(_routed(c1, slot, lens, True), split1)                         # group 1: never MFMA
    finally:
        hip.ATTN_MFMA_MIN_ITEMS = prev


def test_three_launches_and_five_graph_replays_are_bitwise_equal():
    c, (slot, lens) = _case(128, 4), K.attn_rows(129)
    eager = [_paged(c, slot, lens, "pos", 2) for _ in range(3)]
    assert torch.equal(eager[0], eager[1]) and torch.equal(eager[0], eager[2])
    sl, (pos, _), out = _i32(slot), _lens(lens, "pos"), _out(129, c, extra=3)
    s, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=s):
        KP.attn_paged_mfma(c["q"], c["kp"], c["vp"], c["table"], sl, pos, 129, c["n_heads"], c["n_kv"], c["hd"], out, nw=2)
    for i in range(5):
        out.fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[:129], eager[0]) and bool((out[129:] == 7.0).all()), i


def test_refusals_launch_nothing():
    c, sl, pos = _case(64, 2), _i32([1, 2]), _i32([10, 20])
    nkv, out = c["n_kv"], _out(3, c)
    good = dict(table=hip._p(c["table"]), n_pages=c["n_pages"], nh=c["n_heads"], hd=64, t_max=K.ATTN_MAX_SEQ, out=hip._p(out))
    bad = [dict(table=None), dict(t_max=K.ATTN_MAX_SEQ - 1), dict(n_pages=1), dict(nh=nkv), dict(nh=5 * nkv + 1),
           dict(nh=17 * nkv), dict(hd=32), dict(out=out.data_ptr() + 2)]
    for kw in bad:
        a = dict(good, **kw)
        rc = KP._lib().lsa_attn_decode_mfma_paged(hip._p(c["q"]), c["q"].stride(0), hip._p(c["kp"]), hip._p(c["vp"]), a["table"],
                                                  a["n_pages"], hip._p(sl), hip._p(pos), None, 2, a["nh"], nkv, a["hd"],
                                                  a["t_max"], 0.125, a["out"], out.stride(0), 0, hip._stream())
        assert rc != 0, kw
    assert bool((out == 7.0).all())


def test_engine_equals_the_bf16_engine_on_the_mfma_route():
    """tiny() (4 / 2 heads, hd 64): two slots x a 64-token chunk, 8 steps past the page edge, shuffled NaN pool."""
    from llm_sharding_amd.runtime.engine import RandomSource
    from llm_sharding_amd.runtime.engine_int4 import make_stage_engine
    cfg = tiny(layers=2)
    kw = dict(has_embed=True, has_head=True, max_slots=2, max_seq=128, max_prefill_rows=256)
    e16 = make_stage_engine(cfg, 0, 2, DEV, torch.bfloat16, source=RandomSource(cfg, 5), **kw)
    ep = make_stage_engine(cfg, 0, 2, DEV, torch.bfloat16, source=RandomSource(cfg, 5), kv_layout="paged", kv_pages=7, **kw)
    ep.pool._free = [ep.pool._free[i] for i in torch.randperm(ep.kv_free_pages, generator=torch.Generator().manual_seed(0)).tolist()]
    for kp, vp, _ in ep.kvp:
        kp[1:].fill_(float("nan"))
        vp[1:].fill_(float("nan"))
    ids = torch.randint(3, cfg.vocab_size, (128,), generator=torch.Generator().manual_seed(3)).to(DEV)
    prev, hip.ATTN_MFMA_MIN_ITEMS = hip.ATTN_MFMA_MIN_ITEMS, 2
    try:
        hs = []
        for e in (e16, ep):
            slot, pos = e.prefill_rows([0, 1], [64, 64])
            h = [e.forward(e.embed(ids), slot, pos).clone()]
            e.advance([0, 1], [64, 64])
            tok = e.head(h[0], [63, 127]).to(torch.int32)
            for _ in range(8):
                slot, pos = e.prefill_rows([0, 1], [1, 1])
                h.append(e.forward(e.embed(tok), slot, pos).clone())
                e.advance([0, 1], [1, 1])
                tok = e.head(h[-1]).to(torch.int32)
            hs.append(h)
    finally:
        hip.ATTN_MFMA_MIN_ITEMS = prev
    assert ep.seq_len[:2] == [72, 72] and bool(torch.isfinite(hs[1][-1].float()).all())
    for i, (x, y) in enumerate(zip(*hs)):
        assert torch.equal(K.bits(y), K.bits(x)), f"hidden after forward {i}"
