"""Negative controls for the contract-test checkers (tests/contract_cases.py), on the CPU: the
membership decoder accepts an fp64 -> bf16 reference at every case length and flags a reference
with one key dropped or one key too many; assert_footprint raises for a fake "kernel" that writes a
guard row, a guard column, leaves a window element unwritten or appends K/V one position late;
the builders' NaN poison lies outside [0, len) for every row."""
import pytest
import torch

import contract_cases as C

SHAPES = [(8, 2, 64), (8, 8, 128)]


def _all_lengths(hd):
    extra = []
    for nsplit in (4, 16):
        extra += C.split_edge_lengths(hd, nsplit)
    return C.membership_lengths(hd, extra)


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "x".join(map(str, s)))
def case(request):
    nh, nkv, hd = request.param
    return C.build_membership_case(nh, nkv, hd, _all_lengths(hd))


def test_lengths_cover_the_edges():
    for hd in (64, 128):
        lens = C.membership_lengths(hd)
        t_max = C.t_max_for(hd)
        assert t_max % 32 and t_max <= 12 * hd and t_max in lens and 1 in lens
        assert min(lens) >= 1 and max(lens) == t_max  # length 0 is outside the contract
        for nsplit in (4, 16):
            edges = C.split_edge_lengths(hd, nsplit)
            chunk = C.split_chunk(t_max, nsplit, hd)
            assert chunk % ((64 // (hd // 8)) * 4) == 0 and chunk >= 64
            assert {chunk - 1, chunk, chunk + 1} <= set(edges)
    # attn_body.h:54-58 by hand: T 1100, 16 splits, hd 128 -> ceil = 69 -> 69 -> KPI 16 -> 80
    assert C.split_chunk(1100, 16, 128) == 80
    assert C.split_chunk(750, 4, 64) == 192 and C.split_chunk(100, 4, 64) == 64
    assert C.batches(70, 32) == [(0, 32), (32, 64), (38, 70)] and C.batches(64, 32) == [(0, 32), (32, 64)]


def test_poison_lies_outside_the_valid_keys(case):
    used = set(case.slot.tolist())
    assert len(used) == case.rows
    for r, T in enumerate(case.lens):
        s = int(case.slot[r])
        for cache in (case.K, case.V):
            assert bool(torch.isfinite(cache[s, :, :T].float()).all()), (r, T)
            assert bool(C.is_sentinel(cache[s, :, T:]).all()), (r, T)
    for s in range(case.K.shape[0]):
        if s not in used:
            assert bool(C.is_sentinel(case.K[s]).all()) and bool(C.is_sentinel(case.V[s]).all())
    # one row fills the last slot (and so its last kv head) to the end of the cache
    last = case.slot.tolist().index(case.K.shape[0] - 1)
    assert case.lens[last] == case.t_max
    # guard bands on both sides of the cache view
    for flat, cache in ((case.kflat, case.K), (case.vflat, case.V)):
        off = cache.storage_offset()
        assert off >= 512 * case.hd and flat.numel() - off - cache.numel() >= 512 * case.hd
        assert bool(C.is_sentinel(flat[:off]).all()) and bool(C.is_sentinel(flat[off + cache.numel():]).all())
    # the kv_len form's decoy positions are valid and differ from len - 1
    assert bool(((case.pos_decoy >= 0) & (case.pos_decoy < case.t_max) & (case.pos_decoy != case.pos)).all())
    # every V value is exact in bf16 and every per-dim sum at most 126
    assert int(case.expected.max()) <= 126 and int(case.expected.min()) >= 0
    assert bool((case.expected.sum(-1) > 0).all())


def test_decoder_accepts_the_reference(case):
    ref = C.membership_reference(case)
    assert bool(torch.isfinite(ref.float()).all())
    resid = C.check_membership(ref, case, what="reference")
    # bf16 rounding moves a sum by at most 126 * 2^-8 = 0.492; the case lengths leave a wider margin
    assert resid < 0.45, resid


@pytest.mark.parametrize("fault", ["drop_last", "drop_middle", "add_next"])
@pytest.mark.parametrize("renormalise", [True, False])
def test_decoder_flags_a_wrong_key_set(case, fault, renormalise):
    """Row by row: a reference whose key set is off by one key is flagged (a one-key context
    with its only key dropped has no key left and is not a single-key fault)."""
    kw = dict(drop="last") if fault == "drop_last" else dict(drop="middle") if fault == "drop_middle" else dict(add=True)
    bad = C.membership_reference(case, renormalise=renormalise, **kw)
    good = C.membership_reference(case)
    tested = 0
    for r, T in enumerate(case.lens):
        if T == 1 and fault != "add_next":
            continue
        out = good.clone()
        out[r] = bad[r]
        with pytest.raises(AssertionError):
            C.check_membership(out, case, what=fault)
        tested += 1
    assert tested > 0


def test_decoder_flags_poison_and_a_wrong_slot(case):
    out = C.membership_reference(case)
    out[3, 5] = float("nan")
    with pytest.raises(AssertionError, match="non-finite"):
        C.check_membership(out, case)
    # row 1 reading row 2's slot (another shift) with its own length
    out = C.membership_reference(case)
    i = case.lens.index(17)  # (a multiple of hd keys gives a rotation-invariant sum)
    j = (i + 1) % case.rows
    T = case.lens[i]
    si, sj = int(case.slot[i]), int(case.slot[j])
    wrong = torch.stack([torch.roll(case.expected[i, h], int(case.shift[sj, h] - case.shift[si, h]))
                         for h in range(case.nkv)]).double()
    assert not torch.equal(wrong.long(), case.expected[i])
    out[i] = (wrong / T).repeat_interleave(case.nh // case.nkv, 0).reshape(-1).to(torch.bfloat16)
    with pytest.raises(AssertionError):
        C.check_membership(out, case)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32, torch.int32, torch.int64])
def test_assert_footprint_negative_controls(dtype):
    M, N = 17, 48

    def fresh():
        buf, win = C.guarded(M, N, dtype)
        assert buf.shape == (M + 2 * C.GUARD_ROWS, N + C.GUARD_COLS) and buf.stride(0) % 8 == 0
        assert win.data_ptr() % 16 == 0 and bool(C.is_sentinel(buf).all())
        return buf, win

    val = torch.ones((), dtype=dtype)
    buf, win = fresh()
    win.fill_(1)
    C.assert_footprint(buf, win)                       # a correct kernel passes
    for r, c in ((C.GUARD_ROWS - 1, 0), (C.GUARD_ROWS + M, N - 1), (0, 3)):  # guard rows
        buf, win = fresh()
        win.fill_(1)
        buf[r, c] = val
        with pytest.raises(AssertionError, match="outside"):
            C.assert_footprint(buf, win)
    for r, c in ((C.GUARD_ROWS, N), (C.GUARD_ROWS + M - 1, N + C.GUARD_COLS - 1)):  # guard columns
        buf, win = fresh()
        win.fill_(1)
        buf[r, c] = val
        with pytest.raises(AssertionError, match="outside"):
            C.assert_footprint(buf, win)
    buf, win = fresh()
    win.fill_(1)
    C.sentinel_fill(win[M - 1, N - 1:N])              # one element left unwritten
    with pytest.raises(AssertionError, match="unwritten"):
        C.assert_footprint(buf, win)
    opt = torch.zeros(M, N, dtype=torch.bool)
    opt[M - 1] = True
    C.assert_footprint(buf, win, optional=opt)         # ... unless that row may be either
    C.assert_footprint(buf, win, inside="any")
    # a written NaN / a written 0 are not the sentinel
    if dtype.is_floating_point:
        buf, win = fresh()
        win.fill_(float("nan"))
        C.assert_footprint(buf, win)
    b1, w1 = C.guarded_flat(100, dtype)
    w1.zero_()
    C.assert_footprint(b1, w1)
    b1[3] = val
    with pytest.raises(AssertionError, match="outside"):
        C.assert_footprint(b1, w1)


def test_cache_footprint_negative_controls():
    slots, nkv, T, hd, M = 3, 2, 40, 16, 5
    slot = torch.tensor([0, 2, 1, 2, 0, 1, 1])        # longer than M: the tail points at unused cells
    pos = torch.tensor([0, 39, 7, 8, 20, 30, 31])

    def append(at):
        flat, cache = C.guarded_cache(slots, nkv, T, hd)
        cache[slot[:M], :, at[:M]] = 1.0
        return flat, cache

    flat, cache = append(pos)
    C.assert_cache_footprint(flat, cache, slot[:M], pos[:M])
    flat, cache = append(pos + 1 - (pos == T - 1).long() * 2)  # one position late (early at the end)
    with pytest.raises(AssertionError):
        C.assert_cache_footprint(flat, cache, slot[:M], pos[:M])
    flat, cache = append(pos)
    cache[slot[M], :, pos[M]] = 1.0                   # a row >= M appended through a stale pos[m]
    with pytest.raises(AssertionError, match="outside"):
        C.assert_cache_footprint(flat, cache, slot[:M], pos[:M])
    flat, cache = append(pos)
    C.sentinel_fill(cache[2, 1, 39, 3:4])             # one dim of one head not appended
    with pytest.raises(AssertionError, match="unwritten"):
        C.assert_cache_footprint(flat, cache, slot[:M], pos[:M])
    flat, cache = append(pos)
    flat[cache.storage_offset() + cache.numel()] = 1.0  # first element past the cache
    with pytest.raises(AssertionError, match="outside"):
        C.assert_cache_footprint(flat, cache, slot[:M], pos[:M])


@pytest.mark.parametrize("rising", [True, False])
def test_score_case_reference_is_finite_and_peaked(rising):
    nh, nkv, hd = 8, 2, 64
    lens = [1, 2, 33, 257, C.t_max_for(hd)]
    case, q = C.build_score_case(nh, nkv, hd, lens, rising=rising)
    for r, T in enumerate(case.lens):
        s = int(case.slot[r])
        assert bool(torch.isfinite(case.K[s, :, :T].float()).all()) and bool(C.is_sentinel(case.V[s, :, T:]).all())
    ref = C.attention_reference(q, case)
    assert bool(torch.isfinite(ref).all())
    # score * log2(e) spans about 80 over the longest context, monotonically
    T = lens[-1]
    s = int(case.slot[-1])
    sc = (case.K[s, 0, :T, 0].double() * q[-1, 0].double()) * hd ** -0.5 * 1.4426950408889634
    assert 78 < float(sc.max() - sc.min()) < 82
    d = sc[1:] - sc[:-1]
    assert bool((d >= 0).all() if rising else (d <= 0).all())
    # the operand helper: random inside, NaN outside
    buf, win = C.operand(5, 32)
    assert bool(torch.isfinite(win.float()).all()) and int(C.is_sentinel(buf).sum()) == buf.numel() - win.numel()
