"""Per-element contract of every attention kernel (tests/attn_exact_cases.py): case A, a q / K
pattern whose selected keys differ for every head of a GQA group and whose scores are exact, so
``round(out n_r)`` must be the integer vector of exactly head r's selected keys; case B, Gaussian,
peaked and ramped scores against the float64 result, every element inside the rounding interval
``bf16(ref - c A) .. bf16(ref + c A)`` with the derived slack c of the kernel's class; and ties
(exact quotients half way between two bf16 values) that must round to even. Buffers are guarded
as in test_attn_membership_gpu.py. Every test prints its worst needed slack in units of A
(profiles/attn_numerics.md)."""
import functools

import pytest
import torch

import attn_exact_cases as E
import contract_cases as C
import kv8_cases as K8
import test_attn_membership_gpu as M
from llm_sharding_amd.ops import kv8, packing

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES, GQA_SHAPES, OPROJ_SHAPES = M.SHAPES, M.GQA_SHAPES, M.OPROJ_SHAPES
KV8_A_SHAPES = [(8, 2, 64), (8, 2, 128)]                                # test_kv8_gpu.py's membership shapes
KV8_B_SHAPES = [(32, 32, 128), (64, 8, 128), (24, 8, 128), (8, 2, 64)]  # ... and its numerics shapes
hip = M.hip


def _b_lens(hd, rows):
    return tuple(C.pad_lengths(E.B_LENS + [C.t_max_for(hd)], rows))


@functools.lru_cache(maxsize=1)
def _acase(nh, nkv, hd, lens):
    case, q = E.build_select_case(nh, nkv, hd, list(lens), DEV)
    return case, q, E.select_expected(case, case.slot, case.lens_t)


@functools.lru_cache(maxsize=1)
def _bcase(variant, nh, nkv, hd, lens):
    return E.build_b_case(variant, nh, nkv, hd, list(lens), DEV)


@functools.lru_cache(maxsize=1)
def _bref(variant, nh, nkv, hd, lens):
    case, q = _bcase(variant, nh, nkv, hd, lens)
    return case, q, E.interval_reference(q, case)


@functools.lru_cache(maxsize=1)
def _tcase(nh, nkv, hd):
    return E.build_tie_case(nh, nkv, hd, DEV)


def _report(kernel, what, worst, bound):
    print(f"attn-exact B | {kernel} | {what} | worst needed {worst:.3e} A | allowed up to {bound:.3e} A")


def _check_b(out, ref, A, S, T, nh, hd, cls, kernel, what):
    c = E.slack_c(S, T, hd, cls)
    worst = E.check_interval(out, ref, A, c, nh, hd, f"{kernel} {what}", T)
    _report(kernel, what, worst, float(c.max()))
    return worst


def _decode_all(h, case, q, B, nsplit, forms=(False, True)):
    """Every row of ``case`` through hip.attn in launches of B rows: {use_kvlen: bf16 [rows, nh * hd]}."""
    outs = {}
    for use_kvlen in forms:
        out = torch.empty(case.rows, case.nh * case.hd, dtype=torch.bfloat16, device=DEV)
        for r0, r1 in C.batches(case.rows, B):
            qbuf, qw = C.guarded_q(q[r0:r1])
            out[r0:r1] = M._decode(h, case, qw, r0, r1, nsplit, use_kvlen)
        outs[use_kvlen] = out
    return outs


# ------------------------------------------------------------------------------ split / small-grid
def _decode_a(h, shape, lens, B, nsplit, kernel):
    nh, nkv, hd = shape
    case, q, (exp, cnt) = _acase(nh, nkv, hd, tuple(lens))
    worst = 0.0
    for use_kvlen, out in _decode_all(h, case, q, B, nsplit).items():
        worst = max(worst, E.check_select(out, exp, cnt, case.lens_t, f"{kernel} {shape} kv_len {use_kvlen}"))
    print(f"attn-exact A | {kernel} | {shape} | {case.rows} rows | worst decode residual {worst:.3f}")


def _decode_b(h, shape, variant, B, nsplit, kernel, use_kvlen):
    nh, nkv, hd = shape
    case, q, (ref, A, S, T) = _bref(variant, nh, nkv, hd, _b_lens(hd, B))
    out = _decode_all(h, case, q, B, nsplit, forms=(use_kvlen,))[use_kvlen]
    _check_b(out, ref, A, S, T, nh, hd, E.FP32_P, kernel, f"{shape} {variant}")


def _decode_ties(h, shape, B, nsplit, kernel):
    case, q, exp = _tcase(*shape)
    idx = torch.arange(B, device=DEV) % case.rows                        # B rows: the case's rows repeated
    qbuf, qw = C.guarded_q(q[idx])
    big = C.AttnCase(case.nh, case.nkv, case.hd, case.t_max, [case.lens[i % case.rows] for i in range(B)], case.kflat,
                     case.vflat, case.K, case.V, case.slot[idx], case.pos[idx], case.kv_len[idx], case.pos_decoy[idx])
    E.check_ties(M._decode(h, big, qw, 0, B, nsplit, False), exp[idx], f"{kernel} {shape}")


@pytest.mark.parametrize("nsplit", [1, 4, 16])
@pytest.mark.parametrize("nh,nkv,hd", SHAPES)
def test_split_selected_keys(nh, nkv, hd, nsplit):
    h = hip()
    B = M._split_rows(h, nh, nkv)
    lens = C.pad_lengths(C.membership_lengths(hd, C.split_edge_lengths(hd, nsplit)), B)
    _decode_a(h, (nh, nkv, hd), lens, B, nsplit, f"attn_split nsplit {nsplit}")
    _decode_ties(h, (nh, nkv, hd), B, nsplit, f"attn_split nsplit {nsplit}")


@pytest.mark.parametrize("nsplit", [1, 4, 16])
@pytest.mark.parametrize("variant", E.B_VARIANTS)
@pytest.mark.parametrize("nh,nkv,hd", SHAPES)
def test_split_interval(nh, nkv, hd, variant, nsplit):
    h = hip()
    _decode_b(h, (nh, nkv, hd), variant, M._split_rows(h, nh, nkv), nsplit, f"attn_split nsplit {nsplit}", nsplit == 4)


@pytest.mark.parametrize("nh,nkv,hd", SHAPES)
def test_small_grid_selected_keys(nh, nkv, hd):
    h = hip()
    B = M._small_rows(nh, nkv)
    _decode_a(h, (nh, nkv, hd), C.pad_lengths(C.membership_lengths(hd), B), B, 1, "attn_small")
    _decode_ties(h, (nh, nkv, hd), B, 1, "attn_small")


@pytest.mark.parametrize("variant", E.B_VARIANTS)
@pytest.mark.parametrize("nh,nkv,hd", SHAPES)
def test_small_grid_interval(nh, nkv, hd, variant):
    h = hip()
    _decode_b(h, (nh, nkv, hd), variant, M._small_rows(nh, nkv), 1, "attn_small", True)


# ------------------------------------------------------------------------------ gqa_decode_kernel
@pytest.mark.parametrize("nw", [1, 2, 4])
@pytest.mark.parametrize("nh,nkv,hd", GQA_SHAPES)
def test_mfma_decode_selected_keys(nh, nkv, hd, nw):
    """The group's heads are MFMA columns: each must decode to its own selected keys (a padding
    column read as a head, or two columns swapped, decodes to another head's)."""
    h = hip()
    case, q, (exp, cnt) = _acase(nh, nkv, hd, tuple(C.membership_lengths(hd)))
    qbuf, qw = C.guarded_q(q)
    worst = 0.0
    for use_kvlen in (False, True):
        out = M._mfma(h, case, qw, nw, use_kvlen)
        worst = max(worst, E.check_select(out, exp, cnt, case.lens_t, f"gqa_decode nw {nw} kv_len {use_kvlen}"))
    print(f"attn-exact A | gqa_decode nw {nw} | {(nh, nkv, hd)} | {case.rows} rows | worst decode residual {worst:.3f}")
    tcase, tq, texp = _tcase(nh, nkv, hd)
    tbuf, tqw = C.guarded_q(tq)
    E.check_ties(M._mfma(h, tcase, tqw, nw, False), texp, f"gqa_decode nw {nw}")


@pytest.mark.parametrize("nw", [1, 2, 4])
@pytest.mark.parametrize("variant", E.B_VARIANTS)
@pytest.mark.parametrize("nh,nkv,hd", GQA_SHAPES)
def test_mfma_decode_interval(nh, nkv, hd, variant, nw):
    h = hip()
    case, q, (ref, A, S, T) = _bref(variant, nh, nkv, hd, _b_lens(hd, 12))
    qbuf, qw = C.guarded_q(q)
    out = M._mfma(h, case, qw, nw, use_kvlen=nw == 2)
    _check_b(out, ref, A, S, T, nh, hd, E.BF16_P, f"gqa_decode nw {nw}", f"{(nh, nkv, hd)} {variant}")


# ------------------------------------------------------------------------------ flash_prefill_kernel
def _prefill(h, case, segs, q, causal, tile_rows):
    """M._prefill with the tile height chosen: (out window, slot per row, keys per row)."""
    nh, nkv, hd = case.nh, case.nkv, case.hd
    slot = sum([[int(case.slot[j])] * n for j, (p0, n) in enumerate(segs)], [])
    pos = sum([list(range(p0, p0 + n)) for p0, n in segs], [])
    kvl = None if causal else sum([[p0 + n] * n for p0, n in segs], [])
    rows = len(slot)
    obuf, out = C.guarded(rows, nh * hd, device=DEV)
    tiles = h.build_prefill_tiles(slot, pos, kvl, device=DEV, tile_rows=tile_rows)
    assert int(tiles[:, 1].max()) <= tile_rows
    h.attn_prefill(q[:rows], case.K, case.V, tiles, nh, nkv, hd, out, causal=causal)
    torch.cuda.synchronize()
    C.assert_footprint(obuf, out, what=f"prefill causal {causal} tile rows {tile_rows} out")
    lens = torch.tensor([p + 1 for p in pos] if causal else kvl, device=DEV)
    return out, torch.tensor(slot, device=DEV), lens


def _tile_rows(h, nh, nkv, tiles):
    full = h.prefill_tile_rows(nh, nkv)
    assert full > 16 and h.prefill_tile_rows(nh, nkv, 16) == 16          # what a short prompt gets: halved down to 16
    return full if tiles == "full" else 16


@pytest.mark.parametrize("tiles", ["full", "16-row"])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("nh,nkv,hd", SHAPES)
def test_prefill_selected_keys(nh, nkv, hd, causal, tiles):
    """Row i of a causal run sees keys [0, pos0 + i]: each (row, head) decodes to the head's
    selected keys among them; full tiles and the 16-row tiles of prefill_tile_rows(nh, nkv, rows)."""
    h = hip()
    segs = M._prefill_segments(hd, causal)
    case, _, _ = _acase(nh, nkv, hd, tuple(p0 + n for p0, n in segs))
    rows = sum(n for p0, n in segs)
    qbuf, qw = C.guarded_q(E.select_q(rows, nh, hd, DEV))
    out, slots, lens = _prefill(h, case, segs, qw, causal, _tile_rows(h, nh, nkv, tiles))
    exp, cnt = E.select_expected(case, slots, lens)
    worst = E.check_select(out, exp, cnt, lens, f"prefill causal {causal} {tiles} tiles")
    print(f"attn-exact A | flash_prefill causal {causal} {tiles} | {(nh, nkv, hd)} | {rows} rows | "
          f"worst decode residual {worst:.3f}")
    if causal:
        return
    tcase, tq, texp = _tcase(nh, nkv, hd)                                # kv_len 2 and 4: one row each
    tsegs = [(T - 1, 1) for T in tcase.lens]
    tbuf, tqw = C.guarded_q(tq)
    tout, _, _ = _prefill(h, tcase, tsegs, tqw, False, _tile_rows(h, nh, nkv, tiles))
    E.check_ties(tout, texp, f"prefill {tiles} tiles")


@pytest.mark.parametrize("tiles", ["full", "16-row"])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("variant", E.B_VARIANTS)
@pytest.mark.parametrize("nh,nkv,hd", SHAPES)
def test_prefill_interval(nh, nkv, hd, variant, causal, tiles):
    """A fresh 150-row prompt and 70 rows on cached history up to the end of the cache."""
    h = hip()
    t_max = C.t_max_for(hd)
    segs = [(0, 150), (t_max - 70, 70)]
    case, _ = _bcase(variant, nh, nkv, hd, tuple(p0 + n for p0, n in segs))
    rows = sum(n for p0, n in segs)
    q = E.b_query(variant, rows, nh, hd, DEV)
    qbuf, qw = C.guarded_q(q)
    out, slots, lens = _prefill(h, case, segs, qw, causal, _tile_rows(h, nh, nkv, tiles))
    seg_of = sum([[j] * n for j, (p0, n) in enumerate(segs)], [])
    ref, A, S, T = E.interval_reference(q, case, lens=lens.tolist(), rows=seg_of)
    _check_b(out, ref, A, S, T, nh, hd, E.BF16_P, f"flash_prefill causal {causal} {tiles}", f"{(nh, nkv, hd)} {variant}")


# ------------------------------------------------------------------------------ attn_oproj_kernel
def _oproj_setup(nh, hd, N):
    K = nh * hd
    g = torch.Generator(device=DEV).manual_seed(N + nh)
    wp = packing.pack_b((torch.randn(N, K, device=DEV, generator=g) * K ** -0.5).to(torch.bfloat16))
    rbuf, resid = C.operand(1, N, DEV, gen=g)
    return wp, rbuf, resid


def _oproj_rows(h, case, q, N, rows):
    wp, rbuf, resid = _oproj_setup(case.nh, case.hd, N)
    qbuf, qw = C.guarded_q(q)
    return torch.cat([M._oproj(h, case, qw, r, N, wp, resid, use_kvlen=bool(r % 2)).clone() for r in rows])


@pytest.mark.parametrize("nh,nkv,hd,N", OPROJ_SHAPES)
def test_attn_oproj_selected_keys(nh, nkv, hd, N):
    """attn_out of the fused kernel, one launch per length (M._oproj checks the counters zero)."""
    h = hip()
    case, q, (exp, cnt) = _acase(nh, nkv, hd, tuple(C.membership_lengths(hd)))
    att = _oproj_rows(h, case, q, N, range(case.rows))
    worst = E.check_select(att, exp, cnt, case.lens_t, "attn_oproj")
    print(f"attn-exact A | attn_oproj | {(nh, nkv, hd)} | {case.rows} launches | worst decode residual {worst:.3f}")
    tcase, tq, texp = _tcase(nh, nkv, hd)
    E.check_ties(_oproj_rows(h, tcase, tq, N, range(2)), texp[:2], "attn_oproj")


@pytest.mark.parametrize("variant", E.B_VARIANTS)
@pytest.mark.parametrize("nh,nkv,hd,N", OPROJ_SHAPES)
def test_attn_oproj_interval(nh, nkv, hd, N, variant):
    h = hip()
    case, q, (ref, A, S, T) = _bref(variant, nh, nkv, hd, tuple(E.B_LENS + [C.t_max_for(hd)]))
    att = _oproj_rows(h, case, q, N, range(case.rows))
    _check_b(att, ref, A, S, T, nh, hd, E.FP32_P, "attn_oproj", f"{(nh, nkv, hd)} {variant}")


# ------------------------------------------------------------------------------ attn_kv8
def _kv8_attend(case, dev, q, r0, r1, nsplit, form):
    """test_kv8_gpu.py's launch: NaN-guarded q, sentinel-guarded out, counters checked zero."""
    rows, nh, nkv, hd = r1 - r0, case.nh, case.nkv, case.hd
    qbuf, qw = C.guarded_q(q[r0:r1].to(DEV))
    obuf, ow = C.guarded(rows, nh * hd, torch.bfloat16, DEV)
    po = torch.zeros(rows * nh * nsplit * hd, device=DEV)
    pl = torch.zeros(rows * nh * nsplit, device=DEV)
    cnt = torch.zeros(rows * nkv, dtype=torch.int32, device=DEV)
    slot = case.slot[r0:r1].to(DEV)
    pos, kvl = (case.pos[r0:r1], None) if form == "pos" else (case.pos_decoy[r0:r1], case.kv_len[r0:r1].to(DEV))
    kv8.attn_kv8(qw, *dev, slot, pos.to(DEV), rows, nh, nkv, hd, nsplit, po, pl, ow, kv_len=kvl, counters=cnt)
    torch.cuda.synchronize()
    C.assert_footprint(obuf, ow, what=f"attn_kv8 out rows {r0}:{r1} nsplit {nsplit}")
    assert not bool(cnt.any()), "arrival counters left non-zero"
    return ow


def _quantized(case):
    """The case's cache as fp8 tensors on the device; the case itself then holds the DEQUANTISED
    values (what the fp64 reference has to see)."""
    k8, v8, ks, vs = K8.quantize_cache(case.K, case.V)
    for cache, codes, sc in ((case.K, k8, ks), (case.V, v8, vs)):
        ok = ~torch.isnan(sc)
        deq = kv8.dequantize_reference(codes, torch.where(ok, sc, torch.ones(())))
        cache.copy_(torch.where(ok[..., None].to(cache.device), deq.to(cache.device), cache))
    return tuple(t.to(DEV) for t in (k8, v8, ks, vs))


@functools.lru_cache(maxsize=None)
def _kv8_a(nh, nkv, hd):
    extra = K8.kv8_edge_lengths(hd, kv8.attn_kv8_kpi(hd))
    lens = C.pad_lengths(C.membership_lengths(hd, extra), 65)
    case, q = E.build_select_case(nh, nkv, hd, lens)
    bits = C.bits(case.K).clone(), C.bits(case.V).clone()
    dev = _quantized(case)
    assert torch.equal(C.bits(case.K), bits[0]) and torch.equal(C.bits(case.V), bits[1])  # the patterns are exact in e4m3
    return case, q, dev, E.select_expected(case, case.slot, case.lens_t)


@functools.lru_cache(maxsize=None)
def _kv8_t(nh, nkv, hd):
    case, q, exp = E.build_tie_case(nh, nkv, hd)
    bits = C.bits(case.V).clone()
    dev = _quantized(case)
    assert torch.equal(C.bits(case.V), bits)                                 # 4-bit significands, one binade per vector
    return case, q, exp, dev


@pytest.mark.parametrize("form", ["pos", "kv_len"])
@pytest.mark.parametrize("nsplit", [1, 4, 16])
@pytest.mark.parametrize("nh,nkv,hd", KV8_A_SHAPES)
def test_kv8_selected_keys(nh, nkv, hd, nsplit, form):
    case, q, dev, (exp, cnt) = _kv8_a(nh, nkv, hd)
    out = _kv8_attend(case, dev, q, 0, case.rows, nsplit, form)
    worst = E.check_select(out.cpu(), exp, cnt, case.lens_t, f"attn_kv8 nsplit {nsplit} {form}")
    print(f"attn-exact A | attn_kv8 nsplit {nsplit} {form} | {(nh, nkv, hd)} | {case.rows} rows | "
          f"worst decode residual {worst:.3f}")


@pytest.mark.parametrize("nh,nkv,hd", KV8_A_SHAPES)
def test_kv8_selected_keys_in_small_batches(nh, nkv, hd):
    """Few work items per launch (the grids a batch-1 .. 32 decode makes), one split and four; and the ties."""
    case, q, dev, (exp, cnt) = _kv8_a(nh, nkv, hd)
    for b, nsplit in ((32, 1), (1, 4)):
        for r0, r1 in C.batches(case.rows, b)[:40]:
            out = _kv8_attend(case, dev, q, r0, r1, nsplit, "pos")
            E.check_select(out.cpu(), exp[r0:r1], cnt[r0:r1], case.lens_t[r0:r1], f"attn_kv8 rows {r0}:{r1} nsplit {nsplit}")
    tcase, tq, texp, tdev = _kv8_t(nh, nkv, hd)
    for nsplit in (1, 4):
        E.check_ties(_kv8_attend(tcase, tdev, tq, 0, tcase.rows, nsplit, "pos").cpu(), texp, f"attn_kv8 nsplit {nsplit}")


@functools.lru_cache(maxsize=1)
def _kv8_b(variant, nh, nkv, hd):
    case, q = E.build_b_case(variant, nh, nkv, hd, list(E.B_LENS + [C.t_max_for(hd)]))
    dev = _quantized(case)
    ref, A, S, T = E.interval_reference(q, case)
    other = kv8.attn_decode_reference(q, *(t.cpu() for t in dev), case.slot, case.lens, nh)
    assert float((other - ref).abs().max()) <= 1e-12 * float(A.max())       # one reference, two routes
    return case, q, dev, (ref, A, S, T)


@pytest.mark.parametrize("nsplit", [1, 4, 16])
@pytest.mark.parametrize("variant", E.B_VARIANTS)
@pytest.mark.parametrize("nh,nkv,hd", KV8_B_SHAPES)
def test_kv8_interval(nh, nkv, hd, variant, nsplit):
    """Against the fp64 result over the DEQUANTISED cache: the kernel's own roundings are those of
    the bf16 fp32-P kernels (the per-key scales are powers of two), so their slack applies."""
    case, q, dev, (ref, A, S, T) = _kv8_b(variant, nh, nkv, hd)
    out = _kv8_attend(case, dev, q, 0, case.rows, nsplit, "pos" if nsplit != 4 else "kv_len")
    _check_b(out.cpu(), ref, A, S, T, nh, hd, E.FP32_P, f"attn_kv8 nsplit {nsplit}", f"{(nh, nkv, hd)} {variant}")
    if nsplit == 1:                                                          # small batches: one row per launch
        for r in (0, case.rows - 1):
            alone = _kv8_attend(case, dev, q, r, r + 1, 1, "pos")
            assert torch.equal(alone[0], out[r])
