"""GPU side of the paged KV cache (csrc/cache/kv_paged.hip, ops/kv_paged.py,
runtime/engine_paged.py). The kernels do no arithmetic of their own, so every comparison is
torch.equal on raw bits: append and gather against the torch references inside sentinel pools, the
decode attention against lsa_attn_decode on the static cache the pages were cut from (with NaN in
every page a row must not read), and the engine against the bf16 engine on the same weights."""
import pytest
import torch

import kv_paged_cases as K
from llm_sharding_amd.config import tiny, tiny_gpt2
from llm_sharding_amd.ops import hip
from llm_sharding_amd.ops import kv_paged as KP

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAGE = KP.PAGE


def _i32(x):
    return torch.tensor(list(x), dtype=torch.int32, device=DEV)


def _same_bits(a, b, what):
    a, b = K.bits(a), K.bits(b)
    bad = a != b
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} element(s) differ, first at {bad.nonzero()[:4].tolist()}"


# ------------------------------------------------------------------------------ append
def _run_append(case, slot, pos, table=None):
    S, n_kv, T, hd = case["shape"]
    kp, vp = K.sentinel_pool(case["n_pages"], n_kv, hd).to(DEV), K.sentinel_pool(case["n_pages"], n_kv, hd).to(DEV)
    tab = (case["table"] if table is None else table).to(DEV)
    KP.kvp_append(case["kst"].to(DEV), case["vst"].to(DEV), kp, vp, tab, _i32(slot), _i32(pos), len(slot))
    torch.cuda.synchronize()
    return kp, vp


@pytest.mark.parametrize("hd,n_kv,rows", [(128, 2, 1), (64, 8, 7), (128, 8, 129)])
def test_append_equals_the_reference_and_writes_only_the_named_cells(hd, n_kv, rows):
    """The whole pools compared: the named cells hold the staging cells and every other byte, page 0
    included, still holds the sentinel."""
    case = K.append_case(hd, n_kv, rows)
    if rows >= 7:
        assert {(0, 63), (0, 64)} <= set(zip(case["slot"], case["pos"]))           # both sides of a page edge
    kp, vp = _run_append(case, case["slot"], case["pos"])
    _same_bits(kp, case["exp"][0], "append K")
    _same_bits(vp, case["exp"][1], "append V")
    blank = K.sentinel_pool(case["n_pages"], n_kv, hd)
    _same_bits(kp[0], blank[0], "page 0 of K")
    _same_bits(vp[0], blank[0], "page 0 of V")
    assert not torch.equal(K.bits(kp), K.bits(blank))                  # (something was written)


def test_append_skips_rows_outside_the_cache_and_null_entries():
    case = K.append_case(64, 8, 7)
    S, n_kv, T, hd = case["shape"]
    blank = K.sentinel_pool(case["n_pages"], n_kv, hd)
    assert int(case["table"][4, 2]) == 0                               # slot 4's last page is not assigned
    extra_slot, extra_pos = [1, 2, 3, -1, S, 4], [-1, T, T + 5, 3, 3, 2 * PAGE + 9]
    kp, vp = _run_append(case, list(case["slot"]) + extra_slot, list(case["pos"]) + extra_pos)
    _same_bits(kp, case["exp"][0], "append with skipped rows: K")
    _same_bits(vp, case["exp"][1], "append with skipped rows: V")
    kp, vp = _run_append(case, extra_slot, extra_pos)
    _same_bits(kp, blank, "append of skipped rows only: K")
    _same_bits(vp, blank, "append of skipped rows only: V")
    # entries outside [1, n_pages) are null: nothing is written, whatever they hold
    bad = case["table"].clone()
    bad[0, :] = torch.tensor([case["n_pages"], -3, 2 ** 30], dtype=torch.int32)
    kp, vp = _run_append(case, [0, 0, 0], [5, 64, 130], table=bad)
    _same_bits(kp, blank, "append through out-of-range entries: K")
    _same_bits(vp, blank, "append through out-of-range entries: V")


# ------------------------------------------------------------------------------ gather
@pytest.mark.parametrize("hd,n_kv", [(128, 2), (64, 3)])
def test_gather_equals_the_reference_and_writes_only_the_prefixes(hd, n_kv):
    lens = (0, 1, 63, 64, 65, 130)
    S, T, n_pages = len(lens) + 1, 192, 16
    g = torch.Generator().manual_seed(hd)
    kp = torch.randn(n_pages, n_kv, PAGE, hd, generator=g).to(torch.bfloat16)
    vp = torch.randn(n_pages, n_kv, PAGE, hd, generator=g).to(torch.bfloat16)
    kp[0], vp[0] = 0, 0
    table = K.shuffled_table(lens + (PAGE,), T, n_pages, seed=hd)
    table[5, 1] = 0                                                    # a null entry inside a prefix: zeros
    jobs = [(s, n) for s, n in enumerate(lens)]                        # slot 6 is never named
    ek = K.sentinel_pool(S * T // PAGE, n_kv, hd).view(S, n_kv, T, hd).clone()
    ev = ek.clone()
    kst, vst = ek.clone().to(DEV), ev.clone().to(DEV)
    KP.gather_reference(kp, vp, table, ek, ev, jobs)
    assert not bool(ek[5, :, PAGE:2 * PAGE].float().abs().sum()) and bool(ek[5, :, 2 * PAGE:130].float().abs().sum())
    KP.kvp_gather(kp.to(DEV), vp.to(DEV), table.to(DEV), kst, vst, jobs)
    torch.cuda.synchronize()
    _same_bits(kst, ek, "gather K")
    _same_bits(vst, ev, "gather V")


def test_gather_validates():
    n_kv, hd, T, S, n_pages = 2, 64, 128, 3, 8
    kp = torch.zeros(n_pages, n_kv, PAGE, hd, dtype=torch.bfloat16, device=DEV)
    st = torch.zeros(S, n_kv, T, hd, dtype=torch.bfloat16, device=DEV)
    tab = torch.zeros(S, T // PAGE, dtype=torch.int32, device=DEV)
    for jobs in ([(3, 1)], [(0, T + 1)], [(1, 4), (1, 5)], [(-1, 2)]):
        with pytest.raises(ValueError):
            KP.kvp_gather(kp, kp.clone(), tab, st, st.clone(), jobs)
    with pytest.raises(ValueError):
        KP.kvp_gather(kp, kp.clone(), tab, st[:, :, :-1], st.clone(), [(0, 1)])      # staging shape
    with pytest.raises(ValueError):
        KP.kvp_gather(kp, kp.clone(), tab.long(), st, st.clone(), [(0, 1)])          # int64 table
    KP.kvp_gather(kp, kp.clone(), tab, st, st.clone(), [])                           # no jobs: no launch


# ------------------------------------------------------------------------------ attention
_DEV_CASES = {}


def _dev_case(hd, g):
    if (hd, g) not in _DEV_CASES:
        c = K.attn_case(hd, g)
        _DEV_CASES[(hd, g)] = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in c.items()}
    return _DEV_CASES[(hd, g)]


def _attn_pair(c, slot, lens, nsplit, form):
    rows, nh, nkv, hd = len(slot), c["n_heads"], c["n_kv"], c["hd"]
    sl = _i32(slot)
    pos = _i32([n - 1 for n in lens]) if form == "pos" else _i32([0] * rows)
    kvl = None if form == "pos" else _i32(lens)
    outs = []
    for paged in (False, True):
        po = torch.zeros(rows * nh * nsplit * hd, device=DEV)
        pl = torch.zeros(rows * nh * nsplit, device=DEV)
        cnt = torch.zeros(rows * nkv, dtype=torch.int32, device=DEV)
        out = torch.full((rows, nh * hd), 7.0, dtype=torch.bfloat16, device=DEV)
        if paged:
            KP.attn_paged(c["q"], c["kp"], c["vp"], c["table"], sl, pos, rows, nh, nkv, hd, nsplit, po, pl, out,
                          kv_len=kvl, counters=cnt)
        else:
            hip.attn(c["q"], c["k"], c["v"], sl, pos, rows, nh, nkv, hd, nsplit, po, pl, out, kv_len=kvl, counters=cnt)
        torch.cuda.synchronize()
        assert not bool(cnt.any()), "counters left non-zero"
        outs.append(out)
    return outs


@pytest.mark.parametrize("rows", [1, 7, 129])
@pytest.mark.parametrize("nsplit", [1, 4, 16])
@pytest.mark.parametrize("g", [1, 3, 4])
@pytest.mark.parametrize("hd", [64, 128])
def test_attention_equals_the_static_kernel_bit_for_bit(hd, g, nsplit, rows):
    """lsa_attn_decode_paged over the pages == lsa_attn_decode over the static cache they were cut
    from, contexts 1 / 63 / 64 / 65 / 130 / 1100 (and shorter prefixes) mixed across the rows, in
    the ``pos`` and the ``kv_len`` form. Every page no row owns, page 0 included, is NaN, and so is
    the static cache beyond each context: equality with a finite result is also the proof that
    exactly the row's keys were read. rows 1 and 7 with one split take the 8-wave one-trip kernel."""
    c = _dev_case(hd, g)
    cpu = K.attn_case(hd, g)
    assert rows * c["n_kv"] < hip.ATTN_MFMA_MIN_ITEMS                  # hip.attn takes lsa_attn_decode
    launches = [K.attn_rows(1, first=s) for s in range(len(K.CONTEXTS))] if rows == 1 else [K.attn_rows(rows)]
    for slot, lens in launches:
        # the static kernel alone meets the condition only if every live page is assigned
        assert K.live_pages_assigned(cpu["table"], slot, lens, cpu["n_pages"])
        for form in ("pos", "kv_len"):
            static, paged = _attn_pair(c, slot, lens, nsplit, form)
            assert bool(torch.isfinite(static.float()).all()), (form, slot, lens)
            _same_bits(paged, static, f"hd={hd} g={g} nsplit={nsplit} rows={rows} {form} lens={lens[:6]}")


def test_attention_is_the_reference_attention():
    """Against the fp64 reference over the gathered pages: the rounding of a bf16 output plus the
    fp32 accumulation of up to 1100 terms (2^-8 relative covers both with room)."""
    c, cpu = _dev_case(128, 4), K.attn_case(128, 4)
    slot, lens = K.attn_rows(7)
    _, paged = _attn_pair(c, slot, lens, 4, "pos")
    ref = K.attn_reference(cpu["q"], torch.nan_to_num(cpu["kp"]), torch.nan_to_num(cpu["vp"]), cpu["table"], slot, lens,
                           cpu["n_heads"])
    err = (paged.cpu().double() - ref).abs().max() / ref.abs().max()
    assert float(err) < 2.0 ** -8, float(err)


def test_three_launches_and_five_graph_replays_are_bitwise_equal():
    c = _dev_case(128, 4)
    slot, lens = K.attn_rows(129)
    rows, nh, nkv, hd, nsplit = 129, c["n_heads"], c["n_kv"], c["hd"], 4
    eager = [_attn_pair(c, slot, lens, nsplit, "pos")[1] for _ in range(3)]
    assert torch.equal(eager[0], eager[1]) and torch.equal(eager[0], eager[2])
    sl, pos = _i32(slot), _i32([n - 1 for n in lens])
    po = torch.zeros(rows * nh * nsplit * hd, device=DEV)
    pl = torch.zeros(rows * nh * nsplit, device=DEV)
    cnt = torch.zeros(rows * nkv, dtype=torch.int32, device=DEV)
    out = torch.zeros(rows, nh * hd, dtype=torch.bfloat16, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        KP.attn_paged(c["q"], c["kp"], c["vp"], c["table"], sl, pos, rows, nh, nkv, hd, nsplit, po, pl, out, counters=cnt)
    for i in range(5):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager[0]), i
        assert not bool(cnt.any()), i


def test_attention_refusals_launch_nothing():
    c = _dev_case(64, 1)
    rows, nh, nkv, hd = 2, c["n_heads"], c["n_kv"], c["hd"]
    sl, pos = _i32([1, 2]), _i32([10, 20])
    po, pl = torch.zeros(rows * nh * 16 * hd, device=DEV), torch.zeros(rows * nh * 16, device=DEV)
    cnt = torch.zeros(rows * nkv, dtype=torch.int32, device=DEV)
    out = torch.full((rows, nh * hd), 7.0, dtype=torch.bfloat16, device=DEV)

    def call(q=c["q"], kp=c["kp"], vp=c["vp"], table=c["table"], slot=sl, pos=pos, rows=rows, nh=nh, nkv=nkv, hd=hd,
             nsplit=2, po=po, pl=pl, out=out, **kw):
        KP.attn_paged(q, kp, vp, table, slot, pos, rows, nh, nkv, hd, nsplit, po, pl, out, counters=cnt, **kw)

    bad = [dict(nh=5 * nkv), dict(nh=7 * nkv), dict(nsplit=0), dict(nsplit=17), dict(rows=0), dict(table=None),
           dict(table=c["table"].long()), dict(slot=sl.long()), dict(min_chunk=0), dict(po=None), dict(hd=32),
           dict(kp=c["kp"][:, :, :32]), dict(kp=c["kp"].float()), dict(kv_len=sl.long()), dict(rows=3),
           dict(nkv=nkv + 1)]
    for kw in bad:
        with pytest.raises(ValueError):
            call(**kw)
    kp32 = torch.zeros(4, nkv, PAGE, 32, dtype=torch.bfloat16, device=DEV)           # a head size not built
    with pytest.raises(ValueError):
        KP.attn_paged(c["q"], kp32, kp32, c["table"], sl, pos, rows, nh, nkv, 32, 1, None, None, out)
    # the library's own refusals (no Python check in front): LSA_BAD_SHAPE -> ValueError
    L, p = KP._lib(), hip._p
    rc = L.lsa_attn_decode_paged(p(c["q"]), c["q"].stride(0), p(c["kp"]), p(c["vp"]), None, c["n_pages"], p(sl), p(pos),
                                 None, rows, nh, nkv, hd, K.ATTN_MAX_SEQ, 0.125, 1, 64, 128, None, None, p(out),
                                 out.stride(0), None, hip._stream())
    assert rc == 1                                                                   # a null table
    rc = L.lsa_attn_decode_paged(p(c["q"]), c["q"].stride(0), p(c["kp"]), p(c["vp"]), p(c["table"]), c["n_pages"], p(sl),
                                 p(pos), None, rows, nh, nkv, hd, K.ATTN_MAX_SEQ - 1, 0.125, 1, 64, 128, None, None,
                                 p(out), out.stride(0), None, hip._stream())
    assert rc == 1                                                                   # max_seq % PAGE
    rc = L.lsa_attn_decode_paged(p(c["q"]), c["q"].stride(0), p(c["kp"]), p(c["vp"]), p(c["table"]), c["n_pages"], p(sl),
                                 p(pos), None, rows, 5 * nkv, nkv, hd, K.ATTN_MAX_SEQ, 0.125, 1, 64, 128, None, None,
                                 p(out), out.stride(0), None, hip._stream())
    assert rc == 1                                                                   # GQA group 5
    with pytest.raises(ValueError):
        KP._check(1, "lsa_attn_decode_paged")
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and not bool(cnt.any())                          # nothing ran


# ------------------------------------------------------------------------------ engine
def _engines(max_slots=4, max_seq=256, kv_pages=14, layers=2, **kw):
    from llm_sharding_amd.runtime.engine import RandomSource
    from llm_sharding_amd.runtime.engine_int4 import make_stage_engine
    cfg = tiny(layers=layers)
    base = dict(has_embed=True, has_head=True, max_slots=max_slots, max_seq=max_seq, max_prefill_rows=256)
    base.update(kw)
    e16 = make_stage_engine(cfg, 0, layers, DEV, torch.bfloat16, source=RandomSource(cfg, 5), **base)
    ep = make_stage_engine(cfg, 0, layers, DEV, torch.bfloat16, source=RandomSource(cfg, 5), kv_layout="paged",
                           kv_pages=kv_pages, **base)
    return cfg, e16, ep


def _shuffle_pool(ep, seed=0):
    """Hand the allocator its free pages in a shuffled order, so consecutive reservations get
    non-monotone pages and two slots growing in turn interleave."""
    g = torch.Generator().manual_seed(seed)
    free = ep.pool._free
    ep.pool._free = [free[i] for i in torch.randperm(len(free), generator=g).tolist()]   # (no longer a heap)


def test_engine_equals_the_bf16_engine_bit_for_bit():
    """Two sequences, a 150-token prompt each as chunks of 64 (128 rows: the decode-attention route)
    and 86 (172 rows: flash prefill whose tiles start at p0 = 64 > 0, so the prefix is gathered from
    the pages), then 40 decode steps across the page edge at 192; hidden states after every forward
    and the greedy tokens are equal. Then slot 0 is released, a new prompt admitted into the
    recycled pages, and they are equal again."""
    from llm_sharding_amd.runtime.engine_paged import PagedKVStageEngine
    cfg, e16, ep = _engines(kv_pages=7)                                                   # six pages: all of them used
    assert type(ep) is PagedKVStageEngine and ep.paged and len(ep.kvp) == 2
    assert ep.k_cache[0] is ep.k_cache[1] and ep.v_cache[0] is ep.v_cache[1]             # one staging layer
    assert ep.kv_free_pages == 6
    _shuffle_pool(ep)
    for kp, vp, _ in ep.kvp:                                                              # unwritten cells are never read
        kp[1:].fill_(float("nan"))
        vp[1:].fill_(float("nan"))
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(3, cfg.vocab_size, (400,), generator=g).to(DEV)

    def run(e, slots, chunks, steps, at):
        hs, toks = [], []
        for n in chunks:
            slot, pos = e.prefill_rows(slots, [n] * len(slots))
            rows = len(slot)
            h = e.forward(e.embed(ids[at:at + rows]), slot, pos).clone()
            at += rows
            e.advance(slots, [n] * len(slots))
            hs.append(h)
        tok = e.head(hs[-1], [chunks[-1] * (i + 1) - 1 for i in range(len(slots))]).to(torch.int32)
        for _ in range(steps):
            slot, pos = e.prefill_rows(slots, [1] * len(slots))
            h = e.forward(e.embed(tok), slot, pos).clone()
            e.advance(slots, [1] * len(slots))
            tok = e.head(h).to(torch.int32)
            hs.append(h)
            toks.append(tok.clone())
        return hs, toks

    a = run(e16, [0, 1], [64, 86], 40, 0)
    b = run(ep, [0, 1], [64, 86], 40, 0)
    torch.cuda.synchronize()
    assert len(a[0]) == len(b[0]) == 42
    for i, (x, y) in enumerate(zip(a[0], b[0])):
        _same_bits(y, x, f"hidden after forward {i}")
    assert bool(torch.isfinite(b[0][-1].float()).all())
    for i, (x, y) in enumerate(zip(a[1], b[1])):
        assert torch.equal(x, y), i
    assert ep.seq_len[:2] == [190, 190] and ep.kv_free_pages == 0
    p0, p1 = ep.pool.pages_of(0), ep.pool.pages_of(1)
    assert sorted(p0) != p0 or sorted(p1) != p1                                           # shuffled
    assert torch.equal(ep.kv_table.cpu(), ep.pool.table)
    # layer 0's K / V do not depend on attention: its pages are the bf16 engine's layer-0 cache
    ks, vs = KP.to_static(ep.kvp[0][0].cpu(), ep.kvp[0][1].cpu(), ep.pool.table, lens=ep.seq_len)
    _same_bits(ks[:2, :, :190], e16.k_cache[0][:2, :, :190], "layer-0 K pages")
    _same_bits(vs[:2, :, :190], e16.v_cache[0][:2, :, :190], "layer-0 V pages")
    for kp, vp, _ in ep.kvp:
        assert not bool(kp[0].any()) and not bool(vp[0].any())                            # the null page stays zero
    # recycle: slot 0 leaves, a new 100-token prompt takes its pages
    for e in (e16, ep):
        e.reset([0])
    assert ep.kv_free_pages == 3 and ep.pool.pages_of(0) == [] and not bool(ep.kv_table[0].any())
    a = run(e16, [0], [100], 30, 300)
    b = run(ep, [0], [100], 30, 300)
    torch.cuda.synchronize()
    assert sorted(ep.pool.pages_of(0)) == sorted(p0)                                      # recycled pages
    for i, (x, y) in enumerate(zip(a[0], b[0])):
        _same_bits(y, x, f"recycled slot: hidden after forward {i}")
    for i, (x, y) in enumerate(zip(a[1], b[1])):
        assert torch.equal(x, y), i
    assert not bool(ep.attn_cnt.any())


def test_decode_graph_equals_the_eager_step_and_an_unreserved_replay_skips_the_append():
    from llm_sharding_amd.runtime.engine import DecodeGraph
    cfg, _, ep = _engines(max_slots=4, max_seq=128, kv_pages=6)
    _shuffle_pool(ep, 1)
    g = torch.Generator().manual_seed(4)
    ids = torch.randint(3, cfg.vocab_size, (128,), generator=g).to(DEV)
    slot, pos = ep.prefill_rows([0, 1], [62, 17])
    ep.forward(ep.embed(ids[:79]), slot, pos)
    ep.advance([0, 1], [62, 17])
    tok = ids[79:81].to(torch.int32)
    # three eager steps: the third crosses slot 0's page edge (position 63 -> 64)
    want = []
    t = tok
    for _ in range(3):
        slot, pos = ep.prefill_rows([0, 1], [1, 1])
        h = ep.forward(ep.embed(t), slot, pos).clone()
        ep.advance([0, 1], [1, 1])
        t = ep.head(h).to(torch.int32)
        want.append((h, t.clone()))
    assert len(ep.pool.pages_of(0)) == 2
    # rewind: keep the table (so the graph is reserved ahead) and forget the appended cells
    ep.seq_len[0], ep.seq_len[1] = 62, 17
    pg0 = ep.pool.pages_of(0)
    for kp, vp, _ in ep.kvp:
        kp[pg0[0], :, 62:] = 0
        vp[pg0[0], :, 62:] = 0
        kp[pg0[1]] = 0
        vp[pg0[1]] = 0
        kp[ep.pool.pages_of(1)[0], :, 17:] = 0
        vp[ep.pool.pages_of(1)[0], :, 17:] = 0
    dg = DecodeGraph(ep, 2, "full", slots=[0, 1])
    dg.tokens.copy_(tok)
    dg.capture()
    for i in range(3):                                                  # reserved ahead (pages_of(0) has 2 pages)
        dg.replay()
        torch.cuda.synchronize()
        assert torch.equal(dg.out_hidden, want[i][0]) and torch.equal(dg.tokens, want[i][1]), i
    assert dg.pos.tolist() == [65, 20]
    assert not bool(ep.attn_cnt.any())
    # one replay without the reservation: slot 1 loses its pages, its append is skipped
    ep.kv_release(1)
    before = [(kp.clone(), vp.clone()) for kp, vp, _ in ep.kvp]
    dg.replay()
    torch.cuda.synchronize()
    cell = (pg0[1], 65 - PAGE)                                          # slot 0's cell of this step
    for (kp, vp, _), (k0, v0) in zip(ep.kvp, before):
        for new, old in ((kp, k0), (vp, v0)):
            assert bool(new[cell[0], :, cell[1]].float().abs().sum() > 0)
            new[cell[0], :, cell[1]] = old[cell[0], :, cell[1]]
            _same_bits(new, old, "pool after an unreserved replay")    # nothing else moved; page 0 still zero
    assert dg.pos.tolist() == [66, 21]


def test_engine_memory_is_the_models_plus_pages_staging_and_table():
    from llm_sharding_amd.parallel.scheduler import stage_memory
    cfg, e16, ep = _engines(max_slots=6, max_seq=64, kv_pages=5)
    tok = cfg.kv_bytes_per_token_per_layer(2)
    m16 = stage_memory(cfg, 2, slots=6, max_seq=64, prefill_rows=0, has_embed=True, head_rows=cfg.head_rows)
    assert e16.memory_bytes() == m16["weights"] + m16["kv"]
    pages, staging, table = 2 * tok * 5 * PAGE, tok * 6 * 64, 6 * 1 * 4
    assert ep.memory_bytes() == m16["weights"] + pages + staging + table
    m = stage_memory(cfg, 2, slots=6, max_seq=64, prefill_rows=0, has_embed=True, head_rows=cfg.head_rows,
                     kv_layout="paged", kv_pages=5)
    assert m["kv"] == pages and m["scratch"] - m16["scratch"] == staging + table
    assert ep.memory_bytes() == m["weights"] + m["kv"] + staging + table


def test_engine_refusals():
    from llm_sharding_amd.ops.kvcache import fork_slots
    from llm_sharding_amd.runtime.engine import RandomSource
    from llm_sharding_amd.runtime.engine_int4 import make_stage_engine
    cfg = tiny(layers=1)
    kw = dict(has_embed=True, has_head=True, source=RandomSource(cfg, 0), max_slots=3, max_seq=64)
    with pytest.raises(ValueError, match="int4"):
        make_stage_engine(cfg, 0, 1, DEV, torch.bfloat16, kv_layout="paged", kv_pages=4, weight_dtype="int4", **kw)
    with pytest.raises(ValueError, match="fp8"):
        make_stage_engine(cfg, 0, 1, DEV, torch.bfloat16, kv_layout="paged", kv_pages=4, kv_dtype="fp8", **kw)
    with pytest.raises(ValueError, match="kv_layout"):
        make_stage_engine(cfg, 0, 1, DEV, torch.bfloat16, kv_layout="blocked", **kw)
    with pytest.raises(ValueError, match="kv_pages"):
        make_stage_engine(cfg, 0, 1, DEV, torch.bfloat16, kv_layout="paged", kv_pages=1, **kw)
    with pytest.raises(ValueError, match="multiple of the page"):
        make_stage_engine(cfg, 0, 1, DEV, torch.bfloat16, kv_layout="paged", kv_pages=4, **dict(kw, max_seq=96))
    g2 = tiny_gpt2(layers=1)
    with pytest.raises(NotImplementedError, match="GPT-2"):
        make_stage_engine(g2, 0, 1, DEV, torch.bfloat16, kv_layout="paged", kv_pages=4, has_embed=True, has_head=True,
                          source=RandomSource(g2, 0), max_slots=2, max_seq=64)
    ep = make_stage_engine(cfg, 0, 1, DEV, torch.bfloat16, kv_layout="paged", kv_pages=3, **kw)
    with pytest.raises(NotImplementedError, match="fork"):
        fork_slots(ep, 0, [1, 2], 4)
    with pytest.raises(NotImplementedError, match="fork"):
        ep.kv_fork(0, [1], 4)
    # the pool is short: the third slot's first page cannot be had, and nothing changed
    ep.kv_reserve(0, 64)
    ep.kv_reserve(1, 1)
    with pytest.raises(RuntimeError, match="exhausted"):
        ep.kv_reserve(2, 1)
    assert ep.kv_free_pages == 0 and not bool(ep.kv_table[2].any())
    epw = make_stage_engine(cfg, 0, 1, DEV, torch.bfloat16, kv_layout="paged", kv_pages=3, weight_dtype="fp8", **kw)
    assert epw.fp8 and epw.paged                                        # fp8 weights + paged KV: the base body serves both
    slot, pos = epw.prefill_rows([0], [5])
    assert bool(torch.isfinite(epw.forward(epw.embed(torch.arange(3, 8, device=DEV)), slot, pos).float()).all())


def test_sampling_graph_through_the_paged_engine_gives_the_bf16_engines_tokens():
    from llm_sharding_amd.runtime.sampling import SamplingDecodeGraph, SamplingParams
    cfg, e16, ep = _engines(max_slots=4, max_seq=128, kv_pages=6)
    _shuffle_pool(ep, 2)
    g = torch.Generator().manual_seed(6)
    ids = torch.randint(3, cfg.vocab_size, (81,), generator=g).to(DEV)
    hist = []
    for e in (e16, ep):
        slot, pos = e.prefill_rows([0, 1], [60, 17])
        e.forward(e.embed(ids[:77]), slot, pos)
        e.advance([0, 1], [60, 17])
        if e is ep:
            ep.kv_reserve(0, 60 + 8)                                   # the replays cross a page edge: reserved ahead
            ep.kv_reserve(1, 17 + 8)
        sg = SamplingDecodeGraph(e, 2, "full", slots=[0, 1], history_len=8)
        sg.set_params(1, SamplingParams(0.7, top_k=20, seed=5))
        sg.tokens.copy_(ids[77:79].to(torch.int32))
        sg.capture()
        for _ in range(8):
            sg.replay()
        torch.cuda.synchronize()
        assert sg.pos.tolist() == [68, 25]
        hist.append(sg.history.clone())
    assert torch.equal(hist[0], hist[1])
    assert len(set(hist[0][:, 1].tolist())) > 1                         # the sampled row moves
