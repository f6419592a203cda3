"""lsa_attn_decode_mfma_kv8 (csrc/cache/kv8_mfma.hip): fp64 numerics, key membership under NaN poison, determinism and
graph capture, the route of kv8.attn, and the fp8 engine on that route."""
import functools

import pytest
import torch

import contract_cases as C
import kv8_cases as K8
from llm_sharding_amd.config import tiny
from llm_sharding_amd.ops import hip, kv8
from llm_sharding_amd.utils.numerics import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
T_MAX = 320
LENS = [1, 31, 32, 33, 64, 65, 129, 257, T_MAX, T_MAX + 80]    # sub-block / wave hand-over / buffer re-use edges, the clamp
SLOTS = [3, 7, 1, 10, 5, 2, 9, 4, 8, 6]          # one slot per row; slots 0 and 11 belong to nobody
SHAPES = [(24, 8, 128), (64, 8, 128), (16, 2, 64), (12, 2, 64), (32, 16, 128), (8, 2, 128), (32, 2, 64)]  # G 3 8 8 6 2 4 16


def _i32(x):
    return torch.tensor(list(x), dtype=torch.int32, device=DEV)


@functools.lru_cache(maxsize=None)
def _case(nh, nkv, hd, t_max=T_MAX):
    """Gaussian bf16 cache quantised by the reference, q, the fp64 reference, and the poisoned twin of the cache."""
    g = torch.Generator().manual_seed(nh * 1000 + hd)
    kc, vc = (torch.randn(12, nkv, t_max, hd, generator=g).to(torch.bfloat16) for _ in range(2))
    (k8, ks), (v8, vs) = kv8.quantize_reference(kc), kv8.quantize_reference(vc)
    q = torch.randn(len(LENS), nh * hd, generator=g).to(torch.bfloat16)
    lens = [min(n, t_max) for n in LENS]
    ref = kv8.attn_decode_reference(q, k8, v8, ks, vs, SLOTS, lens, nh)
    dead = torch.ones(12, t_max, dtype=torch.bool)
    for s, n in zip(SLOTS, lens):
        dead[s, :n] = False
    dead = dead[:, None, :].expand(-1, nkv, -1)
    poison = [t.clone() for t in (k8, v8, ks, vs)]
    for codes, sc in ((poison[0], poison[2]), (poison[1], poison[3])):
        codes[dead] = K8.NAN_CODE
        sc[dead] = float("nan")
    deq = (kv8.dequantize_reference(k8, ks), kv8.dequantize_reference(v8, vs))
    dev = lambda ts: tuple(t.to(DEV) for t in ts)
    return dict(q=q.to(DEV), cache=dev((k8, v8, ks, vs)), poison=dev(poison), deq=dev(deq), ref=ref, nh=nh, nkv=nkv, hd=hd)


def _forms(form):                                                # (pos is a decoy once kv_len is given)
    return (_i32(n - 1 for n in LENS), None) if form == "pos" else (_i32([0] * len(LENS)), _i32(LENS))


def _raw(c, cache, form, nw):
    """The entry point itself, into a sentinel-guarded output: (return code, output window)."""
    (pos, kvl), (buf, out), p = _forms(form), C.guarded(len(LENS), c["nh"] * c["hd"], torch.bfloat16, DEV), hip._p
    rc = kv8._lib().lsa_attn_decode_mfma_kv8(p(c["q"]), c["q"].stride(0), *(p(t) for t in cache), p(_i32(SLOTS)), p(pos),
                                             p(kvl), len(LENS), c["nh"], c["nkv"], c["hd"], T_MAX, c["hd"] ** -0.5, p(out),
                                             out.stride(0), nw, hip._stream())
    torch.cuda.synchronize()
    C.assert_footprint(buf, out, what="lsa_attn_decode_mfma_kv8 out")
    return rc, out


@pytest.mark.parametrize("form", ["pos", "kv_len"])
@pytest.mark.parametrize("nw", [1, 2, 4])
@pytest.mark.parametrize("nh,nkv,hd", SHAPES)
def test_numerics_and_membership(nh, nkv, hd, nw, form):
    """rel_err < 1e-2 against fp64 (the MFMA and the kv8 kernel's bound), and at most 1.5 times the error of the bf16 MFMA
    kernel on the dequantised cache (same roundings of P and output, another summation order). The poisoned cache - NaN
    codes and NaN scales in every cell no row owns - must give finite, identical bits: every row is compared."""
    c = _case(nh, nkv, hd)
    rc, out = _raw(c, c["cache"], form, nw)
    assert rc == 0
    (pos, kvl), base = _forms(form), torch.zeros_like(out)
    rc = hip.lib().lsa_attn_decode_mfma(hip._p(c["q"]), c["q"].stride(0), hip._p(c["deq"][0]), hip._p(c["deq"][1]),
                                        hip._p(_i32(SLOTS)), hip._p(pos), hip._p(kvl), len(LENS), nh, nkv, hd, T_MAX,
                                        hd ** -0.5, hip._p(base), base.stride(0), nw, hip._stream())
    assert rc == 0
    e, e16 = float(rel_err(out.cpu(), c["ref"])), float(rel_err(base.cpu(), c["ref"]))
    print(f"kv8 mfma ({nh},{nkv},{hd}) nw {nw} {form}: rel_err {e:.3e}, bf16 mfma on the dequantised cache {e16:.3e}, "
          f"ratio {e / e16:.3f}")
    assert e < 1e-2 and e <= 1.5 * e16
    rc, got = _raw(c, c["poison"], form, nw)
    assert rc == 0 and bool(torch.isfinite(got.float()).all())
    assert torch.equal(C.bits(got), C.bits(out))


ROWS, NH, NKV, HD = 129, 8, 2, 128


@functools.lru_cache(maxsize=None)
def _batch():
    g = torch.Generator().manual_seed(7)
    kc, vc = (torch.randn(ROWS, NKV, T_MAX, HD, generator=g).to(torch.bfloat16) for _ in range(2))
    (k8, ks), (v8, vs) = kv8.quantize_reference(kc), kv8.quantize_reference(vc)
    q = torch.randn(ROWS, NH * HD, generator=g).to(torch.bfloat16).to(DEV)
    return tuple(t.to(DEV) for t in (k8, v8, ks, vs)), q, _i32((7 * r + 3) % ROWS for r in range(ROWS)), \
        _i32((37 * r + 5) % T_MAX for r in range(ROWS))


def _mfma(rows=ROWS, r0=0, nw=2):
    cache, q, slot, pos = _batch()
    out = torch.zeros(rows, NH * HD, dtype=torch.bfloat16, device=DEV)
    kv8.attn_kv8_mfma(q[r0:r0 + rows], *cache, slot[r0:r0 + rows].clone(), pos[r0:r0 + rows].clone(), rows, NH, NKV, HD, out,
                      nw=nw)
    return out


def _routed(nh=NH, mfma=True):
    cache, q, slot, pos = _batch()
    po, pl = torch.zeros(ROWS * nh * 4 * HD, device=DEV), torch.zeros(ROWS * nh * 4, device=DEV)
    cnt, out = torch.zeros(ROWS * NKV, dtype=torch.int32, device=DEV), torch.zeros(ROWS, nh * HD, dtype=torch.bfloat16, device=DEV)
    (kv8.attn if mfma is not None else kv8.attn_kv8)(q, *cache, slot, pos, ROWS, nh, NKV, HD, 4, po, pl, out, counters=cnt)
    return out


def test_launches_a_lone_row_and_graph_replays_are_bitwise_equal():
    full = _mfma()
    assert torch.equal(full, _mfma()) and torch.equal(full, _mfma())
    assert torch.equal(_mfma(rows=1, r0=5)[0], full[5])
    cache, q, slot, pos = _batch()
    out, s, g = torch.zeros_like(full), torch.cuda.Stream(), torch.cuda.CUDAGraph()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=s):
        kv8.attn_kv8_mfma(q, *cache, slot, pos, ROWS, NH, NKV, HD, out, nw=2)
    for i in range(3):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, full), i


def test_attn_takes_hip_attns_route_and_the_binding_refuses():
    split, split1 = _routed(mfma=None), _routed(nh=NKV, mfma=None)      # attn_kv8 itself, G = 4 and G = 1
    prev, prev_nw = (hip.ATTN_MFMA_MIN_ITEMS, hip.ATTN_MFMA), hip.ATTN_GQA_NW
    try:
        hip.ATTN_MFMA_MIN_ITEMS, hip.ATTN_MFMA, hip.ATTN_GQA_NW = ROWS * NKV, True, 2
        assert torch.equal(_routed(), _mfma(nw=2)) and not torch.equal(_routed(), split)
        assert torch.equal(_routed(nh=NKV), split1)                     # group 1: never MFMA
        hip.ATTN_MFMA = False
        assert torch.equal(_routed(), split)                            # the switch
        hip.ATTN_MFMA_MIN_ITEMS, hip.ATTN_MFMA = ROWS * NKV + 1, True
        assert torch.equal(_routed(), split)                            # one item fewer than the threshold
    finally:
        (hip.ATTN_MFMA_MIN_ITEMS, hip.ATTN_MFMA), hip.ATTN_GQA_NW = prev, prev_nw
    (cache, _, slot, pos), q = _batch(), torch.zeros(ROWS, 17 * NKV * HD, dtype=torch.bfloat16, device=DEV)
    out, p = torch.full_like(q, 7.0), hip._p
    bad = ((NKV, HD, T_MAX, 2), (17 * NKV, HD, T_MAX, 2), (NH, 32, T_MAX, 2), (NH + 1, HD, T_MAX, 1), (NH, HD, 318, 1))
    for nh, hd, t, code in bad:    # G 1, G 17, hd 32, nh % nkv, max_seq % 4 (the documented refusal: 16-byte scale loads)
        cut = tuple((t_[..., :hd] if t_.dim() == 4 else t_)[:, :, :t].contiguous() for t_ in cache)
        with pytest.raises(ValueError):
            kv8.attn_kv8_mfma(q, *cut, slot, pos, ROWS, nh, NKV, hd, out)
        assert kv8._lib().lsa_attn_decode_mfma_kv8(p(q), q.stride(0), *(p(t_) for t_ in cache), p(slot), p(pos), None, ROWS, nh,
                                                   NKV, hd, t, 0.1, p(out), out.stride(0), 0, hip._stream()) == code
    assert bool((out == 7.0).all())


def test_engine_on_the_mfma_route():
    """tiny() (G = 2): 60-token prefills, 6 decode steps across key 64, route on (2 items suffice) and off; a captured step."""
    from llm_sharding_amd.models import weights as W
    from llm_sharding_amd.runtime.engine import DecodeGraph, RandomSource
    from llm_sharding_amd.runtime.engine_int4 import make_stage_engine
    cfg = tiny(layers=2)
    ids = torch.randint(3, cfg.vocab_size, (120,), generator=torch.Generator().manual_seed(3)).to(DEV)
    head = W.random_lm_head(cfg, torch.bfloat16, "cpu", 5).float().t()
    logits = lambda h: torch.nn.functional.rms_norm(h.cpu().float(), (h.shape[1],), eps=cfg.rms_norm_eps) @ head
    prev = hip.ATTN_MFMA_MIN_ITEMS
    try:
        hs = []
        for items in (2, 1 << 30):
            hip.ATTN_MFMA_MIN_ITEMS = items
            e = make_stage_engine(cfg, 0, 2, DEV, torch.bfloat16, source=RandomSource(cfg, 5), kv_dtype="fp8", has_embed=True,
                                  has_head=True, max_slots=2, max_seq=128, max_prefill_rows=256)
            slot, pos = e.prefill_rows([0, 1], [60, 60])
            e.forward(e.embed(ids), slot, pos)
            e.advance([0, 1], [60, 60])
            tok, steps = ids[:2].to(torch.int32), []
            for _ in range(6):
                slot, pos = e.prefill_rows([0, 1], [1, 1])
                steps.append(e.forward(e.embed(tok), slot, pos).clone())
                e.advance([0, 1], [1, 1])
            hs.append(torch.cat(steps))
            if items == 2:                                              # sequence lengths 66: the next step, captured
                slot, pos = e.prefill_rows([0, 1], [1, 1])
                eager = e.forward(e.embed(tok), slot, pos).clone()
                dg = DecodeGraph(e, 2, "full", slots=[0, 1])
                dg.tokens.copy_(tok)
                dg.capture().replay()
                torch.cuda.synchronize()
                assert torch.equal(dg.out_hidden, eager)
    finally:
        hip.ATTN_MFMA_MIN_ITEMS = prev
    assert not torch.equal(hs[0], hs[1])                                # (another kernel ran: another summation order)
    err = rel_err(logits(hs[0]), logits(hs[1]))
    print(f"fp8 engine, MFMA route against split route, logits rel_err {float(err):.3e}")
    assert err < 1e-2
