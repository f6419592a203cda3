"""GPU side of the fp8 KV cache (csrc/cache/kv8.hip, ops/kv8.py, runtime/engine_kv8.py): append and
dequant bit for bit against the torch references inside guarded buffers, the decode attention's
exact key membership and its numerics against the fp64 reference over the dequantised cache,
determinism, and the engine against the bf16 engine on the same weights."""
import functools

import pytest
import torch

import contract_cases as C
import kv8_cases as K8
from llm_sharding_amd.config import tiny, tiny_gpt2
from llm_sharding_amd.ops import kv8
from llm_sharding_amd.utils.numerics import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _i32(x):
    return torch.tensor(list(x), dtype=torch.int32, device=DEV)


def _same_bits(a, b, what):
    a, b = a.cpu(), b.cpu()
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    bad = a != b
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} element(s) differ, first at {bad.nonzero()[:4].tolist()}"


# ------------------------------------------------------------------------------ append
def _run_append(case, slot, pos, rows):
    got = {k: v.clone().to(DEV) for k, v in _blank(case).items()}
    views = _views(case, got)
    kv8.kv8_append(case["kst"].to(DEV), case["vst"].to(DEV), views["k8"], views["v8"], views["ks"], views["vs"],
                   _i32(slot), _i32(pos), rows)
    torch.cuda.synchronize()
    return got


def _blank(case):
    """The four guarded allocations, all sentinel."""
    shape = case["shape"]
    return {"k8": K8.guarded_u8(shape)[0], "v8": K8.guarded_u8(shape)[0],
            "ks": K8.guarded_f32(shape[:3])[0], "vs": K8.guarded_f32(shape[:3])[0]}


def _views(case, flats):
    shape = case["shape"]
    n8, ns = shape[0] * shape[1] * shape[2] * shape[3], shape[0] * shape[1] * shape[2]
    g8, gs = K8.GUARD_KEYS * shape[3], K8.GUARD_KEYS
    return {"k8": flats["k8"][g8:g8 + n8].view(*shape), "v8": flats["v8"][g8:g8 + n8].view(*shape),
            "ks": flats["ks"][gs:gs + ns].view(*shape[:3]), "vs": flats["vs"][gs:gs + ns].view(*shape[:3])}


@pytest.mark.parametrize("hd,n_kv,rows", [(128, 2, 1), (64, 8, 1), (128, 8, 7), (64, 2, 7), (128, 8, 129), (64, 2, 129),
                                          (128, 2, 600), (64, 8, 600)])
def test_append_equals_the_reference_and_writes_only_the_named_cells(hd, n_kv, rows):
    """Codes and scales bitwise, and the whole guarded allocations compared: every byte outside the
    named cells is still the sentinel. (128, 8, 129), (128, 2, 600) and (64, 8, 600) carry all 65280
    finite bf16 patterns in both groupings (kv8_cases.vector_pool), the others a prefix of them."""
    case = K8.append_case(hd, n_kv, rows)
    assert case["covers_all_patterns"] == ((hd, n_kv, rows) in ((128, 8, 129), (128, 2, 600), (64, 8, 600)))
    got = _run_append(case, case["slot"], case["pos"], rows)
    for name in ("k8", "v8", "ks", "vs"):
        _same_bits(got[name], case["exp"][name], f"append {name} hd={hd} n_kv={n_kv} rows={rows}")


def test_append_skips_rows_outside_the_cache():
    case = K8.append_case(128, 2, 7)
    t_max = case["shape"][2]
    slot = list(case["slot"]) + [1, 2, 3]
    pos = list(case["pos"]) + [-1, t_max, t_max + 5]
    got = _run_append(case, slot, pos, len(slot))
    for name in ("k8", "v8", "ks", "vs"):
        _same_bits(got[name], case["exp"][name], f"append with skipped rows: {name}")
    only = _run_append(case, [1, 2, 3], [-1, t_max, -7], 3)
    for name, blank in _blank(case).items():
        _same_bits(only[name], blank, f"append of skipped rows only: {name}")


def test_append_validates():
    case = K8.append_case(64, 2, 7)
    t = {k: v.to(DEV) for k, v in _views(case, _blank(case)).items()}
    kst, vst = case["kst"].to(DEV), case["vst"].to(DEV)
    slot, pos = _i32(case["slot"]), _i32(case["pos"])
    with pytest.raises(ValueError):
        kv8.kv8_append(kst, vst, t["k8"], t["v8"], t["ks"], t["vs"], slot, pos, 8)            # more rows than slot holds
    with pytest.raises(ValueError):
        kv8.kv8_append(kst[:, :, :-1], vst, t["k8"], t["v8"], t["ks"], t["vs"], slot, pos, 7)  # staging shape
    with pytest.raises(ValueError):
        kv8.kv8_append(kst, vst, t["k8"], t["v8"], t["ks"].double(), t["vs"], slot, pos, 7)    # scale dtype
    with pytest.raises(ValueError):
        kv8.kv8_append(kst, vst, t["k8"], t["v8"], t["ks"], t["vs"], slot.long(), pos, 7)      # int64 slot


# ------------------------------------------------------------------------------ dequant
@pytest.mark.parametrize("hd,n_kv", [(128, 2), (64, 3)])
def test_dequant_equals_the_reference_and_writes_only_the_prefixes(hd, n_kv):
    slots, t_max = 7, 133
    g = torch.Generator().manual_seed(hd)
    x = (torch.randn(slots, n_kv, t_max, hd, generator=g) *
         2.0 ** torch.randint(-12, 13, (slots, n_kv, t_max, 1), generator=g)).to(torch.bfloat16)
    x[2, 0, 5] = 0                                                   # a zero vector: s = 1
    codes, sc = kv8.quantize_reference(x)
    v_codes, v_sc = kv8.quantize_reference(x.flip(2))
    jobs = [(5, t_max), (1, 1), (3, 0), (6, 77), (2, 32)]           # slots 0 and 4 are never named
    kflat, kst = C.guarded_cache(slots, n_kv, t_max, hd, DEV)
    vflat, vst = C.guarded_cache(slots, n_kv, t_max, hd, DEV)
    ek, ev = kflat.cpu().clone(), vflat.cpu().clone()
    gk = 512 * hd
    ekv, evv = ek[gk:gk + x.numel()].view(x.shape), ev[gk:gk + x.numel()].view(x.shape)
    for s, n in jobs:
        ekv[s, :, :n] = kv8.dequantize_reference(codes[s, :, :n], sc[s, :, :n])
        evv[s, :, :n] = kv8.dequantize_reference(v_codes[s, :, :n], v_sc[s, :, :n])
    kv8.kv8_dequant(codes.to(DEV), v_codes.to(DEV), sc.to(DEV), v_sc.to(DEV), kst, vst, jobs)
    torch.cuda.synchronize()
    _same_bits(C.bits(kflat), C.bits(ek), "dequant K")
    _same_bits(C.bits(vflat), C.bits(ev), "dequant V")
    with pytest.raises(ValueError):
        kv8.kv8_dequant(codes.to(DEV), v_codes.to(DEV), sc.to(DEV), v_sc.to(DEV), kst, vst, [(7, 1)])
    with pytest.raises(ValueError):
        kv8.kv8_dequant(codes.to(DEV), v_codes.to(DEV), sc.to(DEV), v_sc.to(DEV), kst, vst, [(1, t_max + 1)])


# ------------------------------------------------------------------------------ attention: membership
NH, NKV = 8, 2


@functools.lru_cache(maxsize=None)
def _membership(hd):
    """The exact-membership cache as fp8 tensors on the device; lengths 1, t_max, the base set and
    c - 1, c, c + 1 around the chunk edges of THIS kernel (its keys per iteration, from the binding)."""
    extra = K8.kv8_edge_lengths(hd, kv8.attn_kv8_kpi(hd))
    lens = C.pad_lengths(C.membership_lengths(hd, extra), 65)
    case = C.build_membership_case(NH, NKV, hd, lens)
    dev = tuple(t.to(DEV) for t in K8.quantize_cache(case.K, case.V))
    assert bool((dev[0][0] == K8.NAN_CODE).all()) and bool(torch.isnan(dev[2][0]).all())  # an unused slot
    return case, dev


def _attend(case, dev, q, r0, r1, nsplit, form):
    """Rows [r0, r1) of ``case`` through attn_kv8 with a NaN-guarded q and a sentinel-guarded out."""
    rows = r1 - r0
    nh, nkv, hd = case.nh, case.nkv, case.hd
    qbuf, qw = C.guarded_q(q[r0:r1].to(DEV))
    obuf, ow = C.guarded(rows, nh * hd, torch.bfloat16, DEV)
    po = torch.zeros(rows * nh * nsplit * hd, device=DEV)
    pl = torch.zeros(rows * nh * nsplit, device=DEV)
    cnt = torch.zeros(rows * nkv, dtype=torch.int32, device=DEV)
    slot = case.slot[r0:r1].to(DEV)
    if form == "pos":
        pos, kvl = case.pos[r0:r1].to(DEV), None
    else:
        pos, kvl = case.pos_decoy[r0:r1].to(DEV), case.kv_len[r0:r1].to(DEV)
    kv8.attn_kv8(qw, *dev, slot, pos, rows, nh, nkv, hd, nsplit, po, pl, ow, kv_len=kvl, counters=cnt)
    torch.cuda.synchronize()
    C.assert_footprint(obuf, ow, what=f"attn_kv8 out rows {r0}:{r1} nsplit {nsplit}")
    assert not bool(cnt.any()), "arrival counters left non-zero"
    return ow


@pytest.mark.parametrize("form", ["pos", "kv_len"])
@pytest.mark.parametrize("nsplit", [1, 4, 16])
@pytest.mark.parametrize("hd", [64, 128])
def test_membership(hd, nsplit, form):
    case, dev = _membership(hd)
    q = torch.zeros(case.rows, case.nh * hd, dtype=torch.bfloat16)
    out = _attend(case, dev, q, 0, case.rows, nsplit, form)
    C.check_membership(out, case, what=f"kv8 hd={hd} nsplit={nsplit} {form}")


@pytest.mark.parametrize("hd", [64, 128])
def test_membership_in_small_batches(hd):
    """Few work items per launch (the grids a batch-1 .. 32 decode makes), one split and four."""
    case, dev = _membership(hd)
    q = torch.zeros(case.rows, case.nh * hd, dtype=torch.bfloat16)
    for b, nsplit in ((32, 1), (1, 4)):
        for r0, r1 in C.batches(case.rows, b)[:40]:
            out = _attend(case, dev, q, r0, r1, nsplit, "pos")
            C.check_membership(out, case, r0, r1, what=f"kv8 hd={hd} rows {r0}:{r1} nsplit={nsplit}")


# ------------------------------------------------------------------------------ attention: numerics
@functools.lru_cache(maxsize=None)
def _gauss_cache(nkv, hd, slots=3, T=1100):
    g = torch.Generator().manual_seed(nkv * 1000 + hd)
    kc = torch.randn(slots, nkv, T, hd, generator=g).to(torch.bfloat16)
    vc = torch.randn(slots, nkv, T, hd, generator=g).to(torch.bfloat16)
    (k8, ks), (v8, vs) = kv8.quantize_reference(kc), kv8.quantize_reference(vc)
    return k8, v8, ks, vs


@pytest.mark.parametrize("nh,nkv,hd", [(32, 32, 128), (64, 8, 128), (24, 8, 128), (8, 2, 64)])
@pytest.mark.parametrize("nsplit", [1, 4, 16])
def test_attention_numerics(nh, nkv, hd, nsplit):
    """test_attention_split's shapes and positions against the fp64 reference over the
    DEQUANTISED cache: the kernel's roundings are fp32 accumulation and the bf16 store, so the
    bf16 kernel's tolerance applies."""
    cache = _gauss_cache(nkv, hd)
    rows = 6
    q = torch.randn(rows, nh * hd, generator=torch.Generator().manual_seed(nh)).to(torch.bfloat16)
    slot, pos = [0, 1, 2, 0, 1, 2], [0, 1, 37, 255, 511, 1099]
    ref = kv8.attn_decode_reference(q, *cache, slot, [p + 1 for p in pos], nh)
    dev = tuple(t.to(DEV) for t in cache)
    po = torch.zeros(rows * nh * nsplit * hd, device=DEV)
    pl = torch.zeros(rows * nh * nsplit, device=DEV)
    out = torch.zeros(rows, nh * hd, dtype=torch.bfloat16, device=DEV)
    kv8.attn_kv8(q.to(DEV), *dev, _i32(slot), _i32(pos), rows, nh, nkv, hd, nsplit, po, pl, out)
    e = rel_err(out.cpu(), ref)
    print(f"attn_kv8 ({nh},{nkv},{hd}) nsplit {nsplit}: rel_err {e:.3e}")
    assert e < 1e-2


@pytest.mark.parametrize("rising", [True, False])
@pytest.mark.parametrize("hd", [64, 128])
def test_attention_score_range(hd, rising):
    """Scores spanning 80 in the exp2 domain, the running maximum moving in every block (rising) or
    never (falling), with one split and four, in the pos and the kv_len form."""
    lens = C.pad_lengths([1, 2, 17, 64, 129, 300, 513, C.t_max_for(hd)], 66)
    case, q = C.build_score_case(NH, NKV, hd, lens, rising=rising)
    cache = K8.quantize_cache(case.K, case.V)
    ref = kv8.attn_decode_reference(q, *cache, case.slot, case.lens, NH)
    dev = tuple(t.to(DEV) for t in cache)
    for nsplit in (1, 4):
        out = _attend(case, dev, q, 0, case.rows, nsplit, "pos")
        assert bool(torch.isfinite(out.float()).all())
        e = rel_err(out.cpu(), ref)
        print(f"score case hd {hd} rising {rising} nsplit {nsplit}: rel_err {e:.3e}")
        assert e < 1e-2
    out = _attend(case, dev, q, 0, 32, 1, "kv_len")
    assert rel_err(out.cpu(), ref[:32]) < 1e-2


def test_attention_refuses_unbuilt_shapes():
    k8 = torch.zeros(1, 1, 16, 128, dtype=torch.uint8, device=DEV)
    ks = torch.zeros(1, 1, 16, device=DEV)
    q = torch.zeros(1, 5 * 128, dtype=torch.bfloat16, device=DEV)
    out = torch.zeros_like(q)
    z = _i32([0])
    with pytest.raises(ValueError):
        kv8.attn_kv8(q, k8, k8, ks, ks, z, z, 1, 5, 1, 128, 1, None, None, out)               # G = 5
    with pytest.raises(ValueError):
        kv8.attn_kv8(q, k8, k8, ks, ks, z, z, 1, 1, 1, 128, 17, None, None, out)              # nsplit > 16
    with pytest.raises(ValueError):
        kv8.attn_kv8(q, k8, k8, ks, ks, z, z, 1, 1, 1, 128, 2, None, None, out)               # no workspace
    k32 = torch.zeros(1, 1, 16, 32, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        kv8.attn_kv8(q, k32, k32, ks, ks, z, z, 1, 1, 1, 32, 1, None, None, out)              # hd 32
    L = kv8._lib()
    p = kv8.hip._p
    assert L.lsa_attn_decode_kv8(p(q), 640, p(k8), p(k8), p(ks), p(ks), p(z), p(z), None, 1, 5, 1, 128, 16, 1.0, 1, 64,
                                 None, None, p(out), 640, None, None) == 2                     # LSA_UNSUPPORTED
    assert L.lsa_attn_decode_kv8(p(q), 640, p(k8), p(k8), p(ks), p(ks), p(z), p(z), None, 1, 5, 2, 128, 16, 1.0, 1, 64,
                                 None, None, p(out), 640, None, None) == 1                     # LSA_BAD_SHAPE
    assert L.lsa_attn_decode_kv8(p(q), 640, p(k32), p(k32), p(ks), p(ks), p(z), p(z), None, 1, 1, 1, 32, 16, 1.0, 1, 64,
                                 None, None, p(out), 640, None, None) == 2


# ------------------------------------------------------------------------------ determinism
def _det_setup(rows=129, nh=8, nkv=2, hd=128, T=600):
    g = torch.Generator().manual_seed(7)
    kc = torch.randn(rows, nkv, T, hd, generator=g).to(torch.bfloat16)
    vc = torch.randn(rows, nkv, T, hd, generator=g).to(torch.bfloat16)
    dev = tuple(t.to(DEV) for pair in (kv8.quantize_reference(kc), kv8.quantize_reference(vc)) for t in pair)
    dev = (dev[0], dev[2], dev[1], dev[3])
    q = torch.randn(rows, nh * hd, generator=g).to(torch.bfloat16).to(DEV)
    slot = _i32((7 * r + 3) % rows for r in range(rows))
    pos = _i32((37 * r + 5) % T for r in range(rows))
    return dev, q, slot, pos


def _det_run(dev, q, slot, pos, rows, nsplit, nh=8, nkv=2, hd=128):
    po = torch.zeros(rows * nh * nsplit * hd, device=DEV)
    pl = torch.zeros(rows * nh * nsplit, device=DEV)
    cnt = torch.zeros(rows * nkv, dtype=torch.int32, device=DEV)
    out = torch.zeros(rows, nh * hd, dtype=torch.bfloat16, device=DEV)
    kv8.attn_kv8(q, *dev, slot, pos, rows, nh, nkv, hd, nsplit, po, pl, out, counters=cnt)
    torch.cuda.synchronize()
    assert not bool(cnt.any())
    return out


@pytest.mark.parametrize("nsplit", [1, 4, 16])
def test_three_launches_are_bitwise_equal(nsplit):
    dev, q, slot, pos = _det_setup()
    outs = [_det_run(dev, q, slot, pos, 129, nsplit) for _ in range(3)]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_a_row_alone_equals_the_row_inside_129_rows():
    """One kernel serves every grid, and a row's chunks depend on its own length only."""
    dev, q, slot, pos = _det_setup()
    for nsplit in (1, 4):
        full = _det_run(dev, q, slot, pos, 129, nsplit)
        for r in (0, 64, 128):
            alone = _det_run(dev, q[r:r + 1], slot[r:r + 1].clone(), pos[r:r + 1].clone(), 1, nsplit)
            assert torch.equal(alone[0], full[r]), (nsplit, r)


def test_graph_replays_are_bitwise_equal_and_leave_the_counters_zero():
    dev, q, slot, pos = _det_setup()
    rows, nh, nkv, hd, nsplit = 129, 8, 2, 128, 4
    eager = _det_run(dev, q, slot, pos, rows, nsplit)
    po = torch.zeros(rows * nh * nsplit * hd, device=DEV)
    pl = torch.zeros(rows * nh * nsplit, device=DEV)
    cnt = torch.zeros(rows * nkv, dtype=torch.int32, device=DEV)
    out = torch.zeros(rows, nh * hd, dtype=torch.bfloat16, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        kv8.attn_kv8(q, *dev, slot, pos, rows, nh, nkv, hd, nsplit, po, pl, out, counters=cnt)
    for i in range(3):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager), i
        assert not bool(cnt.any()), i


# ------------------------------------------------------------------------------ engine
# Global rel_err of the final logits, fp8-KV engine against the bf16 engine, on this file's tiny case
# (2 layers, hd 64), measured on an MI355X (profiles/kv8.md): 1.726e-3 on the two decode rows (67 and
# 115 tokens of context) and 4.983e-3 on the 160-row step (158 of its rows attend one key). Each is
# asserted at twice the measured value: the margin covers input seeds, not another algorithm.
LOGITS_REL_ERR_MEASURED = (1.726e-3, 4.983e-3)


def _engines(max_slots=160, max_seq=128):
    from llm_sharding_amd.runtime.engine import RandomSource
    from llm_sharding_amd.runtime.engine_int4 import make_stage_engine
    cfg = tiny(layers=2)
    kw = dict(has_embed=True, has_head=True, max_slots=max_slots, max_seq=max_seq, max_prefill_rows=256)
    e16 = make_stage_engine(cfg, 0, 2, DEV, torch.bfloat16, source=RandomSource(cfg, 5), **kw)
    e8 = make_stage_engine(cfg, 0, 2, DEV, torch.bfloat16, source=RandomSource(cfg, 5), kv_dtype="fp8", **kw)
    return cfg, e16, e8


def _logits(cfg, h, seed=5):
    from llm_sharding_amd.models import weights as W
    from llm_sharding_amd.models.reference import rmsnorm
    x = rmsnorm(h.cpu().float(), W.random_final_norm(cfg, torch.bfloat16, "cpu", seed).float(), cfg.rms_norm_eps)
    return x @ W.random_lm_head(cfg, torch.bfloat16, "cpu", seed).float().t()


def test_engine_against_the_bf16_engine():
    """A 40-token prefill (decode-attention route), its 24-token continuation batched with another
    sequence's 112 tokens (136 rows: the flash-prefill route, a tile at p0 = 40 > 0 whose prefix is
    restored from the codes), three decode steps, and one 160-row decode step through the GEMMs."""
    from llm_sharding_amd.runtime.engine_kv8 import Fp8KVStageEngine
    cfg, e16, e8 = _engines()
    assert type(e8) is Fp8KVStageEngine and e8.kv8 and len(e8.kv8_cache) == 2
    assert e8.k_cache[0] is e8.k_cache[1] and e8.v_cache[0] is e8.v_cache[1]       # one staging layer
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(3, cfg.vocab_size, (1024,), generator=g).to(DEV)
    written = torch.zeros(160, 128, dtype=torch.bool)
    outs = {}
    for name, e in (("bf16", e16), ("fp8", e8)):
        at = 0

        def step(slots, lens, direct=False):
            nonlocal at
            slot, pos = e.prefill_rows(slots, lens)
            n = len(slot)
            h = e.embed(ids[at:at + n])
            at += n
            if direct:  # a > 128-row DECODE step (what a 160-row decode graph runs): no tile table
                h = e._forward_hip(h, e._i32(slot), e._i32(pos), None, n, nsplit=e.decode_nsplit(n)).clone()
            else:
                h = e.forward(h, slot, pos).clone()
            e.advance(slots, lens)
            written[torch.tensor(slot), torch.tensor(pos)] = True
            return h
        step([0], [40])
        step([0, 1], [24, 112])
        for _ in range(3):
            h = step([0, 1], [1, 1])
        outs[name] = (h, step(list(range(160)), [1] * 160, direct=True))
    torch.cuda.synchronize()
    # layer 0's K / V do not depend on attention: the fp8 engine's layer-0 tensors are the reference
    # quantisation of the bf16 engine's layer-0 cache at every written cell, and untouched elsewhere
    k8, v8, ks, vs = (t.cpu() for t in e8.kv8_cache[0])
    for c8, sc, bf in ((k8, ks, e16.k_cache[0]), (v8, vs, e16.v_cache[0])):
        codes, s = kv8.quantize_reference(bf.cpu())
        w = written[:, None, :].expand(-1, cfg.num_key_value_heads, -1)
        _same_bits(c8[w], codes[w], "layer-0 codes")
        _same_bits(sc[w], s[w], "layer-0 scales")
        assert not bool(c8[~w].any()) and not bool(sc[~w].any()), "cells never appended were written"
    for c in e8.kv8_cache[1]:
        w = written[:, None, :].expand(-1, cfg.num_key_value_heads, -1)
        assert not bool(c.cpu()[~w].any())
    errs = [rel_err(_logits(cfg, outs["fp8"][i]), _logits(cfg, outs["bf16"][i])) for i in (0, 1)]
    print(f"fp8-KV against bf16 engine, final logits rel_err: decode rows {errs[0]:.4e}, 160-row step {errs[1]:.4e}")
    for e, measured in zip(errs, LOGITS_REL_ERR_MEASURED):
        assert 0 < float(e) <= 2 * measured, (errs, LOGITS_REL_ERR_MEASURED)


def test_engine_memory_is_the_models_plus_the_staging_layer():
    from llm_sharding_amd.parallel.scheduler import stage_memory
    cfg, e16, e8 = _engines(max_slots=6, max_seq=64)
    m = stage_memory(cfg, 2, slots=6, max_seq=64, prefill_rows=0, has_embed=True, head_rows=cfg.head_rows, kv_dtype="fp8")
    staging = cfg.kv_bytes_per_token_per_layer(2) * 6 * 64
    assert m["kv"] == 2 * cfg.num_key_value_heads * (2 * cfg.head_dim + 8) * 6 * 64
    assert e8.memory_bytes() == m["weights"] + m["kv"] + staging
    m16 = stage_memory(cfg, 2, slots=6, max_seq=64, prefill_rows=0, has_embed=True, head_rows=cfg.head_rows)
    assert e16.memory_bytes() == m16["weights"] + m16["kv"]
    assert m["scratch"] - m16["scratch"] == staging


def test_decode_graph_equals_the_eager_step():
    from llm_sharding_amd.runtime.engine import DecodeGraph
    cfg, _, e8 = _engines(max_slots=4, max_seq=128)
    g = torch.Generator().manual_seed(4)
    ids = torch.randint(3, cfg.vocab_size, (64,), generator=g).to(DEV)
    slot, pos = e8.prefill_rows([0, 1], [30, 17])
    e8.forward(e8.embed(ids[:47]), slot, pos)
    e8.advance([0, 1], [30, 17])
    tok = ids[47:49].to(torch.int32)
    slot, pos = e8.prefill_rows([0, 1], [1, 1])
    h = e8.forward(e8.embed(tok), slot, pos).clone()
    nxt = e8.head(h).to(torch.int32)
    cells = [tuple(t[[0, 1], :, [30, 17]].clone() for t in c) for c in e8.kv8_cache]
    for c in e8.kv8_cache:                                              # the graph must write them again
        for t in c:
            t[[0, 1], :, [30, 17]] = 0
    dg = DecodeGraph(e8, 2, "full", slots=[0, 1])
    dg.tokens.copy_(tok)
    dg.capture()
    dg.replay()
    torch.cuda.synchronize()
    assert torch.equal(dg.out_hidden, h) and torch.equal(dg.tokens, nxt)
    assert dg.pos.tolist() == [31, 18]
    for c, want in zip(e8.kv8_cache, cells):
        for t, w in zip(c, want):
            assert torch.equal(t[[0, 1], :, [30, 17]], w)
    assert not bool(e8.attn_cnt.any())


def test_engine_refusals():
    from llm_sharding_amd.ops.kvcache import fork_slots
    from llm_sharding_amd.runtime.engine import RandomSource
    from llm_sharding_amd.runtime.engine_int4 import make_stage_engine
    cfg = tiny(layers=1)
    kw = dict(has_embed=True, has_head=True, source=RandomSource(cfg, 0), max_slots=3, max_seq=32)
    with pytest.raises(ValueError, match="int4"):
        make_stage_engine(cfg, 0, 1, DEV, torch.bfloat16, kv_dtype="fp8", weight_dtype="int4", **kw)
    with pytest.raises(ValueError, match="kv_dtype"):
        make_stage_engine(cfg, 0, 1, DEV, torch.bfloat16, kv_dtype="e5m2", **kw)
    g2 = tiny_gpt2(layers=1)
    with pytest.raises(NotImplementedError, match="GPT-2"):
        make_stage_engine(g2, 0, 1, DEV, torch.bfloat16, kv_dtype="fp8", has_embed=True, has_head=True,
                          source=RandomSource(g2, 0), max_slots=2, max_seq=32)
    e8 = make_stage_engine(cfg, 0, 1, DEV, torch.bfloat16, kv_dtype="fp8", **kw)
    with pytest.raises(NotImplementedError, match="fork"):
        fork_slots(e8, 0, [1, 2], 4)
    with pytest.raises(NotImplementedError, match="fork"):
        e8.fork_slots(0, [1], 4)
    e8w = make_stage_engine(cfg, 0, 1, DEV, torch.bfloat16, kv_dtype="fp8", weight_dtype="fp8", **kw)
    assert e8w.fp8 and e8w.kv8                                          # fp8 weights + fp8 KV: the base body serves both
    slot, pos = e8w.prefill_rows([0], [5])
    assert bool(torch.isfinite(e8w.forward(e8w.embed(torch.arange(3, 8, device=DEV)), slot, pos).float()).all())


def test_speculative_graph_through_the_fp8_engine():
    """SpecDecodeGraph on the subclass, unchanged: the k + 1 rows of a step name distinct cells of
    one slot (appended, then attended in the same layer). Run B drafts run A's own output, so every
    draft is accepted: the same tokens, greedy and sampled, in fewer steps - a cell left by a
    rejected draft of run A, or a row that attended a neighbour's cell, would change a token."""
    from llm_sharding_amd.runtime.sampling import SamplingParams
    from llm_sharding_amd.runtime.speculative import generate_speculative
    cfg, _, e8 = _engines(max_slots=4, max_seq=128)
    g = torch.Generator().manual_seed(9)
    prompts = [torch.randint(3, cfg.vocab_size, (n,), generator=g).tolist() for n in (20, 33, 9)]
    params = [None, SamplingParams(0.8, top_p=0.9, seed=3), None]
    new, k = 24, 3
    a, sa = generate_speculative(e8, prompts, new, k=k, sampling=params)
    assert all(len(t) == new for t in a) and all(sum(acc) == new for acc in sa["accepted"])
    b, sb = generate_speculative(e8, prompts, new, k=k, sampling=params, script=[p + t for p, t in zip(prompts, a)])
    assert b == a, (a, b)
    assert all(acc == [k + 1] * (new // (k + 1)) for acc in sb["accepted"]) and sb["steps"] <= sa["steps"]


def test_sampling_graph_through_the_fp8_engine():
    """SamplingDecodeGraph on the subclass, unchanged: a seeded run repeats token for token from
    the same cache state (the second run appends the same cells again), ids stay in the vocabulary."""
    from llm_sharding_amd.runtime.sampling import SamplingDecodeGraph, SamplingParams
    cfg, _, e8 = _engines(max_slots=4, max_seq=128)
    g = torch.Generator().manual_seed(6)
    ids = torch.randint(3, cfg.vocab_size, (49,), generator=g).to(DEV)
    slot, pos = e8.prefill_rows([0, 1], [30, 17])
    e8.forward(e8.embed(ids[:47]), slot, pos)
    e8.advance([0, 1], [30, 17])
    hist = []
    for _ in range(2):
        sg = SamplingDecodeGraph(e8, 2, "full", slots=[0, 1], history_len=8)
        sg.set_params(1, SamplingParams(0.7, top_k=20, seed=5))
        sg.tokens.copy_(ids[47:49].to(torch.int32))
        sg.capture()
        for _ in range(8):
            sg.replay()
        torch.cuda.synchronize()
        assert sg.pos.tolist() == [38, 25]
        hist.append(sg.history.clone())
    assert torch.equal(hist[0], hist[1])
    assert int(hist[0].min()) >= 0 and int(hist[0].max()) < cfg.vocab_size
    assert len(set(hist[0][:, 1].tolist())) > 1                     # the sampled row moves
