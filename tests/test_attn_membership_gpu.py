"""Exact key membership of every attention kernel (tests/contract_cases.py): with q = 0 and a
power-of-two V pattern ``round(out * len)`` must be exactly the integer vector of keys [0, len),
so one key dropped (a split-chunk edge, a wave's sub-block, the last partial block, the length
limit itself) or one key too many fails, and every cache cell at key >= len is NaN, so nothing
beyond the length may reach the output. Plus one score-range case per kernel (q = c e_0, K[:, 0]
rising / falling over the context: score * log2(e) spans 80) against an fp64 softmax.

Every output is a window in a sentinel-filled buffer (nothing outside it may change), q has NaN
rows / columns around it, the split workspaces are sentinel beyond what the launch may use and
the arrival counters are zero afterwards."""
import functools

import pytest
import torch

import contract_cases as C
from llm_sharding_amd.ops import packing
from llm_sharding_amd.utils.numerics import rel_err  # global + per-16x16-tile + per-row

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = [(8, 8, 128), (8, 2, 64), (24, 8, 128)]
# lsa_attn_decode_mfma takes GQA groups of 2..16 heads only (no (8, 8, 128))
GQA_SHAPES = [(8, 2, 64), (24, 8, 128), (64, 8, 128)]
# (nh, nkv, hd, N): the shapes attn_oproj.hip is instantiated for (LSA_AO_CONFIGS); N 4096 at
# K 4096 gives the two-tiles-per-workgroup layout its (128, 1, 16, 2) instance is built for
OPROJ_SHAPES = [(8, 8, 64, 512), (8, 4, 64, 512), (32, 32, 128, 4096)]
SCORE_LENS = [1, 2, 33, 257, 513]  # + t_max


def hip():
    from llm_sharding_amd.ops import hip as h
    h.lib()
    return h


@functools.lru_cache(maxsize=1)
def _mcase(nh, nkv, hd, lens):
    return C.build_membership_case(nh, nkv, hd, list(lens), DEV)


@functools.lru_cache(maxsize=1)
def _scase(nh, nkv, hd, lens, rising):
    case, q = C.build_score_case(nh, nkv, hd, list(lens), DEV, rising=rising, seed=nh * 7 + hd + rising)
    return case, q, C.attention_reference(q, case)


def _split_rows(h, nh, nkv):
    """Rows per launch that reach attn_split_kernel: more than 128 (row, kv-head) items (below it
    nsplit = 1 takes the small-grid kernel) and, for GQA, fewer than hip.attn's MFMA threshold."""
    B = 32 if nkv == 8 else 96
    g = nh // nkv
    assert B * nkv > 128 and not (2 <= g <= 16 and B * nkv >= h.ATTN_MFMA_MIN_ITEMS)
    return B


def _small_rows(nh, nkv):
    B = 128 // nkv
    assert B * nkv <= 128 and nh // nkv <= 4  # attention.hip launch_split: G <= 4, nsplit 1
    return B


def _decode(h, case, q, r0, r1, nsplit, use_kvlen):
    """One hip.attn launch of rows r0 .. r1 with every buffer guarded; returns the output window."""
    B, nh, nkv, hd = r1 - r0, case.nh, case.nkv, case.hd
    obuf, out = C.guarded(B, nh * hd, device=DEV)
    pobuf, po = C.guarded_flat(B * nh * nsplit * hd, torch.float32, DEV)
    plbuf, pl = C.guarded_flat(B * nh * nsplit, torch.float32, DEV)
    cbuf, cnt = C.guarded_flat(B * nkv, torch.int32, DEV)
    cnt.zero_()
    pos = case.pos_decoy[r0:r1] if use_kvlen else case.pos[r0:r1]
    h.attn(q[:B], case.K, case.V, case.slot[r0:r1], pos, B, nh, nkv, hd, nsplit, po, pl, out,
           kv_len=case.kv_len[r0:r1] if use_kvlen else None, counters=cnt)
    torch.cuda.synchronize()
    what = f"rows {r0}:{r1} nsplit {nsplit} kv_len {use_kvlen}"
    C.assert_footprint(obuf, out, what=what + " out")
    C.assert_footprint(pobuf, po, inside="any", what=what + " part_o")
    C.assert_footprint(plbuf, pl, inside="any", what=what + " part_lse")
    C.assert_footprint(cbuf, cnt, what=what + " counters")
    assert int(cnt.abs().sum()) == 0, what + ": arrival counters not reset"
    return out


def _decode_membership(h, case, B, nsplit):
    qbuf, q = C.guarded_q(torch.zeros(B, case.nh * case.hd, dtype=torch.bfloat16, device=DEV))
    tested, worst = 0, 0.0
    for use_kvlen in (False, True):
        for r0, r1 in C.batches(case.rows, B):
            out = _decode(h, case, q, r0, r1, nsplit, use_kvlen)
            worst = max(worst, C.check_membership(out, case, r0, r1, what=f"rows {r0}:{r1} kv_len {use_kvlen}"))
            tested += 1
    assert tested > 0
    return worst


@pytest.mark.parametrize("nsplit", [1, 4, 16])
@pytest.mark.parametrize("nh,nkv,hd", SHAPES)
def test_split_membership(nh, nkv, hd, nsplit):
    """attn_split_kernel: every case length plus c - 1, c, c + 1 around every chunk edge c
    (contract_cases.split_chunk: attn_body.h:54-58), pos and kv_len forms."""
    h = hip()
    B = _split_rows(h, nh, nkv)
    lens = C.pad_lengths(C.membership_lengths(hd, C.split_edge_lengths(hd, nsplit)), B)
    worst = _decode_membership(h, _mcase(nh, nkv, hd, tuple(lens)), B, nsplit)
    print(f"split ({nh},{nkv},{hd}) nsplit {nsplit}: {len(lens)} rows, worst decode residual {worst:.3f}")


@pytest.mark.parametrize("nh,nkv,hd", SHAPES)
def test_small_grid_membership(nh, nkv, hd):
    """attn_small_kernel (rows * n_kv <= 128, one split; 8 waves x 8 key groups)."""
    h = hip()
    B = _small_rows(nh, nkv)
    lens = C.pad_lengths(C.membership_lengths(hd), B)
    worst = _decode_membership(h, _mcase(nh, nkv, hd, tuple(lens)), B, 1)
    print(f"small-grid ({nh},{nkv},{hd}): {len(lens)} rows, worst decode residual {worst:.3f}")


def _mfma(h, case, q, nw, use_kvlen):
    rows, nh, nkv, hd = case.rows, case.nh, case.nkv, case.hd
    obuf, out = C.guarded(rows, nh * hd, device=DEV)
    pos = case.pos_decoy if use_kvlen else case.pos
    rc = h.lib().lsa_attn_decode_mfma(h._p(q), q.stride(0), h._p(case.K), h._p(case.V), h._p(case.slot), h._p(pos),
                                      h._p(case.kv_len if use_kvlen else None), rows, nh, nkv, hd, case.t_max,
                                      float(hd ** -0.5), h._p(out), out.stride(0), nw, h._stream())
    assert rc == 0
    torch.cuda.synchronize()
    C.assert_footprint(obuf, out, what=f"mfma nw {nw} kv_len {use_kvlen} out")
    return out


@pytest.mark.parametrize("nw", [1, 2, 4])
@pytest.mark.parametrize("nh,nkv,hd", GQA_SHAPES)
def test_mfma_decode_membership(nh, nkv, hd, nw):
    """gqa_decode_kernel: waves take the 32-key sub-blocks w, w + nw, ..."""
    h = hip()
    case = _mcase(nh, nkv, hd, tuple(C.membership_lengths(hd)))
    qbuf, q = C.guarded_q(torch.zeros(case.rows, nh * hd, dtype=torch.bfloat16, device=DEV))
    tested, worst = 0, 0.0
    for use_kvlen in (False, True):
        out = _mfma(h, case, q, nw, use_kvlen)
        worst = max(worst, C.check_membership(out, case, what=f"nw {nw} kv_len {use_kvlen}"))
        tested += 1
    assert tested > 0
    print(f"mfma ({nh},{nkv},{hd}) nw {nw}: {case.rows} rows, worst decode residual {worst:.3f}")


def _prefill_segments(hd, causal):
    """(pos0, n) runs, one cache slot each. Causal: every row i decodes to keys [0, pos0 + i], so
    the runs cover lengths 1..150, cached history, the 512 / 1024 marks and the end of the cache,
    with run lengths that are no multiple of any tile height (16..128). Explicit kv_len: one
    run per case length, 1-3 rows each."""
    t_max = C.t_max_for(hd)
    if causal:
        segs = [(0, 150), (37, 70), (0, 1), (200, 61), (500, 30)]
        segs += [(1000, 50), (t_max - 100, 100)] if hd == 128 else [(t_max - 100, 100)]
        return segs
    return [(T - min(T, 1 + i % 3), min(T, 1 + i % 3)) for i, T in enumerate(C.membership_lengths(hd))]


def _prefill(h, case, segs, q, causal):
    nh, nkv, hd = case.nh, case.nkv, case.hd
    slot = sum([[int(case.slot[j])] * n for j, (p0, n) in enumerate(segs)], [])
    pos = sum([list(range(p0, p0 + n)) for p0, n in segs], [])
    kvl = None if causal else sum([[p0 + n] * n for p0, n in segs], [])
    rows = len(slot)
    obuf, out = C.guarded(rows, nh * hd, device=DEV)
    tiles = h.build_prefill_tiles(slot, pos, kvl, device=DEV, tile_rows=h.prefill_tile_rows(nh, nkv))
    h.attn_prefill(q[:rows], case.K, case.V, tiles, nh, nkv, hd, out, causal=causal)
    torch.cuda.synchronize()
    C.assert_footprint(obuf, out, what=f"prefill causal {causal} out")
    lens = torch.tensor([p + 1 for p in pos] if causal else kvl, device=DEV)
    return out, torch.tensor(slot, device=DEV), lens


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("nh,nkv,hd", SHAPES)
def test_prefill_membership(nh, nkv, hd, causal):
    """flash_prefill_kernel: causal rows see exactly keys [0, pos0 + i]; the explicit-kv_len
    (unmasked) form exactly [0, kv_len)."""
    h = hip()
    segs = _prefill_segments(hd, causal)
    assert all(n % 16 for p0, n in segs if n > 3) and any(p0 > 0 for p0, n in segs)
    case = _mcase(nh, nkv, hd, tuple(p0 + n for p0, n in segs))
    assert case.lens[case.slot.tolist().index(case.K.shape[0] - 1)] == case.t_max
    rows = sum(n for p0, n in segs)
    qbuf, q = C.guarded_q(torch.zeros(rows, nh * hd, dtype=torch.bfloat16, device=DEV))
    out, slots, lens = _prefill(h, case, segs, q, causal)
    worst = C.check_membership(out, case, what=f"prefill causal {causal}", lens_t=lens,
                               expected=C.expected_rows(case, slots, lens))
    print(f"prefill ({nh},{nkv},{hd}) causal {causal}: {rows} rows, worst decode residual {worst:.3f}")


def _oproj(h, case, q, r, N, wp, resid, use_kvlen):
    """One attn_oproj launch for row r (batch 1); returns the attn_out window."""
    nh, nkv, hd = case.nh, case.nkv, case.hd
    K = nh * hd
    abuf, att = C.guarded(1, K, device=DEV)
    obuf, out = C.guarded(1, N, device=DEV)
    sync = torch.zeros(4, dtype=torch.int32, device=DEV)
    ep = h.make_epi(out=out, resid=resid, ldo=out.stride(0), ldr=resid.stride(0))
    pos = case.pos_decoy[r:r + 1] if use_kvlen else case.pos[r:r + 1]
    ok = h.attn_oproj(q[r:r + 1], case.K, case.V, case.slot[r:r + 1], pos, nh, nkv, hd, att, wp, N, ep, sync,
                      kv_len=case.kv_len[r:r + 1] if use_kvlen else None)
    assert ok is True
    torch.cuda.synchronize()
    assert sync.tolist() == [0, 0, 0, 0], sync.tolist()
    C.assert_footprint(abuf, att, what=f"attn_oproj row {r} attn_out")
    C.assert_footprint(obuf, out, what=f"attn_oproj row {r} out")
    return att


@pytest.mark.parametrize("nh,nkv,hd,N", OPROJ_SHAPES)
def test_attn_oproj_membership(nh, nkv, hd, N):
    """attn_oproj_kernel's attention part (attn_out only), one launch per case length."""
    h = hip()
    case = _mcase(nh, nkv, hd, tuple(C.membership_lengths(hd)))
    K = nh * hd
    g = torch.Generator(device=DEV).manual_seed(N + nh)
    wp = packing.pack_b((torch.randn(N, K, device=DEV, generator=g) * K ** -0.5).to(torch.bfloat16))
    rbuf, resid = C.operand(1, N, DEV, gen=g)
    qbuf, q = C.guarded_q(torch.zeros(case.rows, K, dtype=torch.bfloat16, device=DEV))
    tested, worst = 0, 0.0
    for r in range(case.rows):
        for use_kvlen in (False, True):
            att = _oproj(h, case, q, r, N, wp, resid, use_kvlen)
            worst = max(worst, C.check_membership(att, case, r, r + 1, what=f"attn_oproj row {r} kv_len {use_kvlen}"))
            tested += 1
    assert tested > 0
    print(f"attn_oproj ({nh},{nkv},{hd}): {tested} launches, worst decode residual {worst:.3f}")


# ------------------------------------------------------------------------------ score range
def _score_lens(hd, rows):
    return tuple(C.pad_lengths(SCORE_LENS + [C.t_max_for(hd)], rows))


def _report(name, shape, rising, err):
    print(f"score-range {name} {shape} {'rising' if rising else 'falling'}: {err!r}")


@pytest.mark.parametrize("rising", [True, False])
@pytest.mark.parametrize("nsplit", [1, 4, 16])
@pytest.mark.parametrize("nh,nkv,hd", SHAPES)
def test_split_score_range(nh, nkv, hd, nsplit, rising):
    h = hip()
    B = _split_rows(h, nh, nkv)
    case, q0, ref = _scase(nh, nkv, hd, _score_lens(hd, B), rising)
    qbuf, q = C.guarded_q(q0)
    out = _decode(h, case, q, 0, B, nsplit, use_kvlen=False)
    err = rel_err(out, ref)
    _report(f"split nsplit {nsplit}", (nh, nkv, hd), rising, err)
    assert err < 1e-2, err


@pytest.mark.parametrize("rising", [True, False])
@pytest.mark.parametrize("nh,nkv,hd", SHAPES)
def test_small_grid_score_range(nh, nkv, hd, rising):
    h = hip()
    B = _small_rows(nh, nkv)
    case, q0, ref = _scase(nh, nkv, hd, _score_lens(hd, B), rising)
    qbuf, q = C.guarded_q(q0)
    out = _decode(h, case, q, 0, B, 1, use_kvlen=True)
    err = rel_err(out, ref)
    _report("small-grid", (nh, nkv, hd), rising, err)
    assert err < 1e-2, err


@pytest.mark.parametrize("rising", [True, False])
@pytest.mark.parametrize("nw", [1, 2, 4])
@pytest.mark.parametrize("nh,nkv,hd", GQA_SHAPES)
def test_mfma_decode_score_range(nh, nkv, hd, nw, rising):
    h = hip()
    case, q0, ref = _scase(nh, nkv, hd, _score_lens(hd, 12), rising)
    qbuf, q = C.guarded_q(q0)
    out = _mfma(h, case, q, nw, use_kvlen=False)
    err = rel_err(out, ref)
    _report(f"mfma nw {nw}", (nh, nkv, hd), rising, err)
    assert err < 1e-2, err


@pytest.mark.parametrize("rising", [True, False])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("nh,nkv,hd", SHAPES)
def test_prefill_score_range(nh, nkv, hd, causal, rising):
    """Two runs (a fresh 150-row prompt and 70 rows on cached history up to the end of the
    cache); every query row is c e_0, the ramp spans each slot's whole context."""
    h = hip()
    t_max = C.t_max_for(hd)
    segs = [(0, 150), (t_max - 70, 70)]
    case, _, _ = _scase(nh, nkv, hd, tuple(p0 + n for p0, n in segs), rising)
    rows = sum(n for p0, n in segs)
    q0 = torch.zeros(rows, nh, hd, dtype=torch.bfloat16, device=DEV)
    q0[:, :, 0] = 80.0 / (8.0 * hd ** -0.5 * 1.4426950408889634)
    qbuf, q = C.guarded_q(q0.view(rows, nh * hd))
    out, slots, lens = _prefill(h, case, segs, q, causal)
    seg_of = sum([[j] * n for j, (p0, n) in enumerate(segs)], [])
    ref = C.attention_reference(q, case, lens=lens.tolist(), rows=seg_of)
    err = rel_err(out, ref)
    _report(f"prefill causal {causal}", (nh, nkv, hd), rising, err)
    assert err < 1e-2, err


@pytest.mark.parametrize("rising", [True, False])
@pytest.mark.parametrize("nh,nkv,hd,N", OPROJ_SHAPES)
def test_attn_oproj_score_range(nh, nkv, hd, N, rising):
    h = hip()
    case, q0, ref = _scase(nh, nkv, hd, _score_lens(hd, 6), rising)
    K = nh * hd
    g = torch.Generator(device=DEV).manual_seed(N + nh)
    wp = packing.pack_b((torch.randn(N, K, device=DEV, generator=g) * K ** -0.5).to(torch.bfloat16))
    rbuf, resid = C.operand(1, N, DEV, gen=g)
    qbuf, q = C.guarded_q(q0)
    att = torch.cat([_oproj(h, case, q, r, N, wp, resid, use_kvlen=bool(r % 2)).clone() for r in range(case.rows)])
    err = rel_err(att, ref)
    _report("attn_oproj", (nh, nkv, hd), rising, err)
    assert err < 1e-2, err
