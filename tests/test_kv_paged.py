"""CPU side of the paged KV cache (ops/kv_paged.py, runtime/engine_paged.py, the scheduler's
pricing and the server's admission by reservation): the page allocator's invariants, the torch
references of append / gather, the forward-body pin, the option checks, and servers on CPU engines
(the cache stays static there, the page accounting runs all the same) against the golden model."""
import multiprocessing as mp
import random
import socket

import pytest
import torch

import kv_paged_cases as K
from llm_sharding_amd.config import get_preset, tiny, tiny_gpt2
from llm_sharding_amd.models import weights as W
from llm_sharding_amd.models.reference import ReferenceLlama
from llm_sharding_amd.ops import kv_paged as KP
from llm_sharding_amd.ops.kv_paged import PAGE, PagePool
from llm_sharding_amd.parallel.scheduler import plan_stages
from llm_sharding_amd.runtime.engine import RandomSource

# ------------------------------------------------------------------------------ PagePool


def test_pool_hands_out_the_lowest_pages_first_and_never_page_zero():
    p = PagePool(8, 3, 256)
    assert p.free_pages == 7 and p.pages_for(0) == 0 and p.pages_for(1) == 1 and p.pages_for(64) == 1 and p.pages_for(65) == 2
    assert p.reserve(1, 65) == [(1, 0, 1), (1, 1, 2)]
    assert p.reserve(0, 1) == [(0, 0, 3)]
    assert p.reserve(1, 129) == [(1, 2, 4)]                            # interleaved with slot 0's
    assert p.pages_of(1) == [1, 2, 4] and p.pages_of(0) == [3] and p.pages_of(2) == []
    assert p.table.dtype == torch.int32 and tuple(p.table.shape) == (3, 4)
    assert p.table.tolist() == [[3, 0, 0, 0], [1, 2, 4, 0], [0, 0, 0, 0]]
    assert p.release(1) == [(1, 0, 0), (1, 1, 0), (1, 2, 0)] and p.table[1].tolist() == [0, 0, 0, 0]
    assert p.reserve(2, 256) == [(2, 0, 1), (2, 1, 2), (2, 2, 4), (2, 3, 5)]       # the lowest free ones again
    assert 0 not in p.pages_of(2) and p.free_pages == 2


def test_reserve_is_idempotent_and_grows_only():
    p = PagePool(6, 2, 256)
    assert len(p.reserve(0, 100)) == 2
    before = p.table.clone()
    assert p.reserve(0, 100) == [] and p.reserve(0, 128) == [] and p.reserve(0, 3) == [] and p.reserve(0, 0) == []
    assert torch.equal(p.table, before) and p.free_pages == 3
    assert p.reserve(0, 129) == [(0, 2, 3)]


def test_exhaustion_raises_and_changes_nothing():
    p = PagePool(4, 2, 256)
    p.reserve(0, 128)
    before, free = p.table.clone(), p.free_pages
    with pytest.raises(RuntimeError, match="exhausted"):
        p.reserve(1, 129)                                              # needs 3, 1 is free
    with pytest.raises(RuntimeError, match="exhausted"):
        p.reserve(0, 256)                                              # needs 2 more, 1 is free
    assert torch.equal(p.table, before) and p.free_pages == free == 1 and p.pages_of(1) == []
    assert p.reserve(1, 64) == [(1, 0, 3)]
    with pytest.raises(ValueError):
        p.reserve(2, 1)
    with pytest.raises(ValueError):
        p.reserve(0, 257)
    for bad in (dict(n_pages=1, max_slots=2, max_seq=128), dict(n_pages=4, max_slots=2, max_seq=96),
                dict(n_pages=4, max_slots=0, max_seq=128), dict(n_pages=4, max_slots=2, max_seq=0)):
        with pytest.raises(ValueError):
            PagePool(**bad)


def test_a_random_trace_keeps_the_invariants():
    rnd = random.Random(7)
    n_pages, S, T = 23, 6, 512
    p = PagePool(n_pages, S, T)
    lens = [0] * S
    for _ in range(600):
        s = rnd.randrange(S)
        if rnd.random() < 0.2:
            p.release(s)
            lens[s] = 0
        else:
            want = min(T, lens[s] + rnd.choice((1, 1, 1, 70, 200)))
            try:
                changed = p.reserve(s, want)
                assert len(changed) == KP.pages_for(want) - KP.pages_for(lens[s])
                lens[s] = want
            except RuntimeError:
                assert KP.pages_for(want) - KP.pages_for(lens[s]) > p.free_pages
        held = [pg for i in range(S) for pg in p.pages_of(i)]
        assert len(set(held)) == len(held) and 0 not in held and all(1 <= pg < n_pages for pg in held)   # disjoint
        assert p.free_pages + len(held) == n_pages - 1
        for i in range(S):
            assert len(p.pages_of(i)) == KP.pages_for(lens[i])
            assert p.table[i, len(p.pages_of(i)):].tolist() == [0] * (T // PAGE - len(p.pages_of(i)))


# ------------------------------------------------------------------------------ references
def test_append_then_gather_round_trips():
    case = K.append_case(64, 2, 129)
    S, n_kv, T, hd = case["shape"]
    kp, vp = (t.clone() for t in case["exp"])
    written = torch.zeros(S, T, dtype=torch.bool)
    written[torch.tensor(case["slot"]), torch.tensor(case["pos"])] = True
    k = torch.zeros(S, n_kv, T, hd, dtype=torch.bfloat16)
    v = torch.zeros_like(k)
    KP.gather_reference(kp, vp, case["table"], k, v, [(s, T if s < 4 else T - PAGE) for s in range(S)])
    w = written[:, None, :, None].expand(S, n_kv, T, hd)
    assert torch.equal(K.bits(k)[w], K.bits(case["kst"])[w]) and torch.equal(K.bits(v)[w], K.bits(case["vst"])[w])
    live = torch.ones(S, T, dtype=torch.bool)
    live[4, T - PAGE:] = False
    rest = (~written & live)[:, None, :, None].expand(S, n_kv, T, hd)
    assert bool((K.bits(k)[rest] == K.bits(K.sentinel_pool(1, 1, 8))[0, 0, 0, 0]).all())       # never appended: sentinel
    assert not bool(k[4, :, T - PAGE:].any())                                                 # never gathered
    kp[0], vp[0] = 0, 0                                                # the null page of a real pool
    ks, vs = KP.to_static(kp, vp, case["table"])
    assert torch.equal(K.bits(ks[:4]), K.bits(k[:4])) and not bool(ks[4, :, T - PAGE:].any())  # a null entry: zeros


def test_an_out_of_range_entry_behaves_as_null():
    case = K.append_case(64, 2, 7)
    S, n_kv, T, hd = case["shape"]
    n_pages = case["n_pages"]
    blank = K.sentinel_pool(n_pages, n_kv, hd)
    for bad in (n_pages, n_pages + 5, -1, 2 ** 31 - 1, -2 ** 31):
        tab = case["table"].clone()
        tab[0, 1] = bad
        assert int(KP.sanitize_table(tab, n_pages)[0, 1]) == 0
        kp, vp = blank.clone(), blank.clone()
        KP.append_reference(case["kst"], case["vst"], kp, vp, tab, [0], [PAGE + 3])
        assert torch.equal(K.bits(kp), K.bits(blank)) and torch.equal(K.bits(vp), K.bits(blank))
        kp[0], vp[0] = 0, 0
        k = torch.ones(S, n_kv, T, hd, dtype=torch.bfloat16)
        v = torch.ones_like(k)
        KP.gather_reference(kp, vp, tab, k, v, [(0, 130)])
        assert not bool(k[0, :, PAGE:2 * PAGE].any()) and not bool(v[0, :, PAGE:2 * PAGE].any())
        assert bool((k[0, :, 130:] == 1).all()) and bool((k[1:] == 1).all())


def test_attention_cases_have_all_their_live_pages_assigned():
    for hd, g in ((64, 1), (128, 3), (128, 4)):
        c = K.attn_case(hd, g)
        for rows in (1, 7, 129):
            slot, lens = K.attn_rows(rows)
            assert K.live_pages_assigned(c["table"], slot, lens, c["n_pages"])
        assert bool(torch.isnan(c["kp"][0].float()).all())                               # page 0 is NaN there
        owners = [pg for row in c["table"].tolist() for pg in row if pg]
        assert len(owners) == len(set(owners)) < c["n_pages"] - 1                         # spare NaN pages exist
        assert any(sorted(r for r in row if r) != [r for r in row if r] for row in c["table"].tolist())   # non-monotone
        # the reference over the gathered pages sees the static cache's keys
        slot, lens = K.attn_rows(7)
        ks, _ = KP.to_static(c["kp"], c["vp"], c["table"])
        for s, n in zip(slot, lens):
            assert torch.equal(K.bits(ks[s, :, :n]), K.bits(c["k"][s, :, :n]))
        assert not K.live_pages_assigned(c["table"], [0], [PAGE + 1], c["n_pages"])      # slot 0 owns one page


# ------------------------------------------------------------------------------ forward body
def test_paged_forward_is_the_base_forward_with_the_paged_calls():
    """PagedKVStageEngine._forward_hip is StageEngine's body: only the lines that name the kv_paged
    calls (prefix gather, append, decode attention) and the attn_oproj switch differ, so every
    projection route is the base engine's, and a change of the base forward fails here until it is
    carried over."""
    import difflib
    import inspect
    from llm_sharding_amd.runtime.engine import StageEngine
    from llm_sharding_amd.runtime.engine_paged import PagedKVStageEngine
    a = inspect.getsource(StageEngine._forward_hip).splitlines()
    b = inspect.getsource(PagedKVStageEngine._forward_hip).splitlines()
    changed = [ln for ln in difflib.unified_diff(a, b, lineterm="", n=0) if not ln.startswith(("---", "+++", "@@"))]
    assert 0 < len(changed) <= 12, changed
    removed = [ln[1:].strip() for ln in changed if ln[0] == "-"]
    added = [ln[1:].strip() for ln in changed if ln[0] == "+"]
    assert len(removed) == 3, removed                         # the two-line ao switch, the hip.attn line
    for body in removed:
        assert "ATTN_OPROJ" in body or "ao_sync is not None" in body or "hip.attn(" in body, body
    for body in added:
        assert "kv_paged" in body or "kvp_jobs" in body, body
    assert sum("kv_paged.attn(" in x for x in added) == 1 and sum("kv_paged.kvp_append(" in x for x in added) == 1
    assert sum("kv_paged.kvp_gather(" in x for x in added) == 1
    assert "ao = False  # kv_paged: attn_oproj reads a bf16 static cache" in added


# ------------------------------------------------------------------------------ scheduler
def test_scheduler_prices_the_paged_cache():
    from llm_sharding_amd.parallel.scheduler import kv_pages_for_memory, kv_token_bytes, stage_memory
    cfg = get_preset("llama2-7b")
    assert kv_token_bytes(cfg) == 16384
    kw = dict(slots=512, max_seq=4096, prefill_rows=2048)
    m16, mp_ = stage_memory(cfg, 32, **kw), stage_memory(cfg, 32, kv_layout="paged", kv_pages=1000, **kw)
    assert m16 == stage_memory(cfg, 32, kv_layout="static", **kw)
    assert m16["kv"] == 32 * 16384 * 512 * 4096 and mp_["kv"] == 32 * 16384 * 1000 * 64
    assert mp_["scratch"] - m16["scratch"] == 16384 * 512 * 4096 + 4 * 512 * 64       # the staging layer + the table
    assert mp_["weights"] == m16["weights"] and mp_["total"] == mp_["weights"] + mp_["kv"] + mp_["scratch"] + mp_["io"]
    for bad in (dict(kv_layout="paged"), dict(kv_layout="paged", kv_pages=1), dict(kv_layout="blocked"),
                dict(kv_layout="paged", kv_pages=8, kv_dtype="fp8"), dict(kv_pages=8)):
        with pytest.raises(ValueError):
            stage_memory(cfg, 32, **bad, **kw)
    # pages: the staging layer over all slots and the table are charged first
    mem, w, res = 288e9, 13.5e9, 8e9
    free = mem - res - w - (16384.0 * 512 * 4096 + 4 * 512 * 64)
    assert kv_pages_for_memory(cfg, 32, 512, 4096, mem, w, reserve_bytes=res) == int(free // (16384.0 * 32 * 64)) == 6918
    assert kv_pages_for_memory(cfg, 16, 512, 4096, mem, w / 2, reserve_bytes=res) > 2 * 6918
    assert kv_pages_for_memory(cfg, 32, 2, 128, mem, w) == 2 * 2 + 1                    # never more than the slots can fill
    with pytest.raises(ValueError):
        kv_pages_for_memory(cfg, 32, 512, 4096, 50e9, w)                               # the staging layer alone does not fit
    with pytest.raises(ValueError):
        kv_pages_for_memory(cfg, 32, 4, 100, mem, w)
    # the planner: 512 x 4096 static tokens do not fit two GPUs' worth of one stage each, pages do
    a = plan_stages(cfg, 2, kv_tokens=512 * 4096, kv_layout="paged", kv_pages=4000)
    assert a.ranges() == [(0, 16), (16, 32)] and a.stages[0].kv_bytes == 16 * 16384 * 4000 * 64
    with pytest.raises(ValueError):
        plan_stages(cfg, 1, kv_tokens=512 * 4096)
    assert plan_stages(cfg, 1, kv_tokens=512 * 4096, kv_layout="paged", kv_pages=6000).ranges() == [(0, 32)]
    # serve.py --kv-pages 0: the pages are those of the plan they give (a fixed point), on every world size
    from llm_sharding_amd.parallel.scheduler import DeviceSpec, size_kv_pages
    assert size_kv_pages(cfg, 1, 512, 4096, 309e9, 12e9)[0] > 6918   # a device larger than DeviceSpec's default fits its own pages
    for world in (1, 2, 3):
        pages, plan = size_kv_pages(cfg, world, 512, 4096, mem, res)
        devs = [DeviceSpec(mem_bytes=mem, reserve_bytes=res)] * world
        assert plan.ranges() == plan_stages(cfg, devs, kv_tokens=512 * 4096, kv_layout="paged", kv_pages=pages).ranges()
        assert pages == min(kv_pages_for_memory(cfg, s.n_layers, 512, 4096, mem, s.weight_bytes, res) for s in plan.stages)
    assert size_kv_pages(cfg, 1, 512, 4096, mem, res)[0] == kv_pages_for_memory(
        cfg, 32, 512, 4096, mem, plan_stages(cfg, 1).stages[0].weight_bytes, res)


# ------------------------------------------------------------------------------ options
def test_option_checks_hold_on_every_device():
    from llm_sharding_amd.runtime.engine import StageEngine
    from llm_sharding_amd.runtime.engine_int4 import make_stage_engine
    from llm_sharding_amd.runtime.engine_paged import check_kv_layout
    cfg = tiny(layers=1)
    kw = dict(has_embed=True, has_head=True, source=RandomSource(cfg, 0), max_slots=2, max_seq=128)
    for bad, what in ((dict(kv_layout="blocked"), "kv_layout"), (dict(kv_layout="paged", kv_pages=1), "kv_pages"),
                      (dict(kv_layout="paged", kv_pages=4, weight_dtype="int4"), "int4"),
                      (dict(kv_layout="paged", kv_pages=4, kv_dtype="fp8"), "fp8"),
                      (dict(kv_layout="static", kv_pages=4), "kv_pages"),
                      (dict(kv_layout="paged", kv_pages=4, max_seq=96), "multiple of the page")):
        with pytest.raises(ValueError, match=what):
            make_stage_engine(cfg, 0, 1, "cpu", torch.float32, **dict(kw, **bad))
    e = make_stage_engine(cfg, 0, 1, "cpu", torch.float32, kv_layout="paged", kv_pages=3, **kw)
    assert type(e) is StageEngine                                      # a CPU device ignores the option
    g2 = tiny_gpt2(layers=1)
    assert type(make_stage_engine(g2, 0, 1, "cpu", torch.float32, kv_layout="paged", kv_pages=3, has_embed=True,
                                  has_head=True, source=RandomSource(g2, 0), max_slots=2, max_seq=128)) is StageEngine
    check_kv_layout("static")
    check_kv_layout("paged", 2)
    check_kv_layout("paged", None)


def test_inference_cli_refuses_speculative_with_a_paged_cache():
    import inference
    with pytest.raises(SystemExit, match="paged"):
        inference.main(["--random", "tiny", "--device", "cpu", "--kv-layout", "paged", "--speculative", "3",
                        "--max-new-tokens", "4"])
    with pytest.raises(SystemExit, match="kv-pages"):
        inference.main(["--random", "tiny", "--device", "cpu", "--kv-pages", "9", "--max-new-tokens", "4"])


# ------------------------------------------------------------------------------ server on CPU engines
SEED, NEW, B, M = 11, 30, 2, 2
KV_PAGES = 4     # three pages: requests 0 (2 pages) and 1 (1 page) fill them


def _cfg():
    return tiny(layers=4)


def _prompts(cfg):
    g = torch.Generator().manual_seed(5)
    return [torch.randint(3, cfg.vocab_size, (n,), generator=g).tolist() for n in (40, 17, 25)]


def _golden(cfg, prompts, n):
    dt = torch.float32
    ref = ReferenceLlama(cfg, W.random_embedding(cfg, dt, seed=SEED),
                         [W.random_layer(cfg, i, dt, seed=SEED) for i in range(cfg.num_hidden_layers)],
                         W.random_final_norm(cfg, dt, seed=SEED), W.random_lm_head(cfg, dt, seed=SEED), max_pos=128)
    return [ref.generate(torch.tensor([p]), n)[0].tolist() for p in prompts]


@pytest.fixture(scope="module")
def golden():
    cfg = _cfg()
    return _golden(cfg, _prompts(cfg), NEW)


def _server(cfg, rank=0, world=1, ctrl=None, **kw):
    from llm_sharding_amd.parallel.server import PipelineServer
    st = plan_stages(cfg, world).stages[rank]
    args = dict(device="cpu", batch=B, microbatches=M, max_seq=128, prefill_budget=16, dtype=torch.float32,
                ctrl_group=ctrl, kv_layout="paged", kv_pages=KV_PAGES)
    args.update(kw)
    return PipelineServer(cfg, RandomSource(cfg, SEED), rank, world, st.start, st.end, **args)


def test_server_admits_by_reservation(golden):
    """Four slots, three pages: requests 0 and 1 hold 2 + 1 pages from admission on, so request 2
    (1 page) keeps its place in the queue, although two slots are free, until one of them finishes."""
    cfg = _cfg()
    srv = _server(cfg)
    prompts = _prompts(cfg)
    assert [srv.kv_pool.pages_for(len(p) + NEW) for p in prompts] == [2, 1, 1]
    seen = []

    def on_token(r, t):
        held = [pg for s in range(B * M) for pg in srv.kv_pool.pages_of(s)]
        assert sum(srv.kv_held.values()) <= KV_PAGES - 1 and srv.kv_pool.free_pages + len(held) == KV_PAGES - 1
        assert len(set(held)) == len(held) and 0 not in held
        if r.rid == rids[2] and len(r.output_ids) == 1:
            seen.append([srv.requests[x].state for x in rids[:2]])

    rids = [srv.submit(p, NEW, eos_ids=(), on_token=on_token) for p in prompts]
    srv.serve(stop_when_idle=True)
    assert [srv.requests[r].output_ids for r in rids] == golden
    assert len(seen) == 1 and "done" in seen[0]                        # admitted only after one had finished
    assert srv.stats()["peak_in_flight"] == 2
    assert srv.kv_pool.free_pages == KV_PAGES - 1 and not srv.kv_held and not srv.kv_len and not bool(srv.kv_pool.table.any())
    # with room for all three they run together
    srv = _server(cfg, kv_pages=5)
    assert srv.generate(prompts, NEW, eos_ids=()) == golden and srv.stats()["peak_in_flight"] == 3


def test_a_reused_slot_releases_the_finished_requests_pages_before_the_pool_is_handed_on():
    """Three pages, four slots, 16 prefill tokens per command. Request 0 finishes early; request 2 is
    admitted into its slot in the same scheduling call (which would cancel a static server's reset) and
    has an 80-token prompt, so for several commands the prefill budget goes to the lower slot and
    request 2's first item is not in the command: the finished request's pages must be back in every
    rank's pool by then, because rank 0 has already handed their budget on. Every pool stays inside
    what rank 0 has reserved, at every command, and the outputs are the golden model's."""
    cfg = _cfg()
    g = torch.Generator().manual_seed(9)
    reqs = [(17, 5), (40, 30), (80, 30), (20, 10), (20, 10)]
    prompts = [torch.randint(3, cfg.vocab_size, (n,), generator=g).tolist() for n, _ in reqs]
    want = [_golden(cfg, [p], new)[0] for p, (_, new) in zip(prompts, reqs)]
    srv = _server(cfg)
    seen = []
    exec_body = srv._exec_body

    def checked(cmd, mb, items, resets, ids=None):
        out = exec_body(cmd, mb, items, resets, ids)
        held = sum(len(srv.kv_pool.pages_of(s)) for s in range(B * M))
        assert held <= sum(srv.kv_held.values()) <= KV_PAGES - 1, (cmd, items, resets, srv.kv_held)
        assert held + srv.kv_pool.free_pages == KV_PAGES - 1
        seen.append((cmd, [it[0] for it in items], list(resets)))
        return out

    srv._exec_body = checked
    rids = [srv.submit(p, new, eos_ids=()) for p, (_, new) in zip(prompts, reqs)]
    srv.serve(stop_when_idle=True)
    assert [srv.requests[r].output_ids for r in rids] == want
    assert any(r and set(r) & set(it) for _, it, r in seen)            # a reset travelled with its slot's reuse
    assert srv.kv_pool.free_pages == KV_PAGES - 1 and not srv.kv_held and not srv.kv_len


def test_server_refusals():
    cfg = _cfg()
    srv = _server(cfg, kv_pages=2)                                     # one page
    with pytest.raises(ValueError, match="pages"):
        srv.submit(list(range(3, 43)), 30)                             # 70 tokens: two pages, more than the pool has
    assert srv.submit(list(range(3, 43)), 24) == 0                     # 64 tokens fit
    with pytest.raises(ValueError, match="prefix_slots"):
        _server(cfg, prefix_slots=2)
    with pytest.raises(ValueError, match="kv_pages"):
        _server(cfg, kv_pages=1)
    with pytest.raises(ValueError, match="multiple of the page"):
        _server(cfg, max_seq=100)
    with pytest.raises(ValueError, match="fp8"):
        _server(cfg, kv_dtype="fp8")
    with pytest.raises(ValueError, match="kv_pages"):
        _server(cfg, kv_layout="static")
    assert _server(cfg, kv_pages=None).kv_pages == B * M * 2 + 1      # default: every slot at max_seq


def _worker(rank, world, port, q):
    import torch.distributed as dist
    torch.set_num_threads(1)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        ctrl = dist.new_group(backend="gloo")
        cfg = _cfg()
        srv = _server(cfg, rank, world, ctrl)
        if rank == 0:
            q.put(srv.generate(_prompts(cfg), NEW, eos_ids=()))
        else:
            srv.serve()
        # every rank drove its own pool from the command stream, and every page came back
        assert srv.kv_pool.free_pages == KV_PAGES - 1 and not srv.kv_len and not bool(srv.kv_pool.table.any())
    finally:
        dist.barrier()
        dist.destroy_process_group()


def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_ranks_over_gloo_match_golden(golden):
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in ps:
        p.start()
    try:
        res = q.get(timeout=240)
    finally:
        for p in ps:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in ps), [p.exitcode for p in ps]
    assert res == golden
