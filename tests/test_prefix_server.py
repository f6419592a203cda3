"""Prefix pool and n parallel samples of the PipelineServer on CPU (fp32, tiny(layers=4)): every
request that forks its prefix from the pool - on one stage or over gloo pipelines, through a hit, a
partial match, a refill after an eviction or a bypass - generates the golden model's greedy tokens,
and ``stats()`` counts what the pool did."""
import multiprocessing as mp
import socket

import pytest
import torch

from llm_sharding_amd.config import tiny
from llm_sharding_amd.models import weights as W
from llm_sharding_amd.models.reference import ReferenceLlama
from llm_sharding_amd.parallel import server as S
from llm_sharding_amd.parallel.scheduler import plan_stages
from llm_sharding_amd.parallel.server import PipelineServer
from llm_sharding_amd.runtime.engine import RandomSource
from llm_sharding_amd.runtime.sampling import SamplingParams

SEED, NEW, B, M, PRE = 11, 6, 2, 2, 20


def _cfg():
    return tiny(layers=4)


def _rand(cfg, g, n):
    return torch.randint(3, cfg.vocab_size, (n,), generator=g).tolist()


# prompts of _prompts() whose greedy output changes when the fork copies nothing (the tiny random
# model ignores the prefix for the others): the tests that fork for one prompt only use these
SENSITIVE = (0, 2, 3, 6)


def _prompts(cfg):
    """Seven prompts that share a 20-token prefix, with distinct suffixes of 1..25 tokens."""
    g = torch.Generator().manual_seed(5)
    pre = _rand(cfg, g, PRE)
    return [pre + _rand(cfg, g, n) for n in (3, 9, 25, 1, 17, 6, 12)]


class _Golden:
    """The fp32 golden model; outputs are computed once per prompt and shared."""

    def __init__(self):
        cfg, dt = _cfg(), torch.float32
        self.ref = ReferenceLlama(cfg, W.random_embedding(cfg, dt, seed=SEED),
                                  [W.random_layer(cfg, i, dt, seed=SEED) for i in range(cfg.num_hidden_layers)],
                                  W.random_final_norm(cfg, dt, seed=SEED), W.random_lm_head(cfg, dt, seed=SEED),
                                  max_pos=128)
        self.memo = {}

    def __call__(self, prompt):
        k = tuple(prompt)
        if k not in self.memo:
            self.memo[k] = self.ref.generate(torch.tensor([prompt]), NEW)[0].tolist()
        return self.memo[k]


@pytest.fixture(scope="module")
def golden():
    return _Golden()


def _server(cfg, rank=0, world=1, ctrl=None, prefix_slots=2, **kw):
    st = plan_stages(cfg, world).stages[rank]
    return PipelineServer(cfg, RandomSource(cfg, SEED), rank, world, st.start, st.end, device="cpu",
                          batch=B, microbatches=M, max_seq=128, prefill_budget=16, dtype=torch.float32,
                          ctrl_group=ctrl, prefix_slots=prefix_slots, **kw)


def _run(srv, prompts, **kw):
    rids = [srv.submit(p, NEW, eos_ids=(), **kw) for p in prompts]
    srv.serve(stop_when_idle=True)
    return [srv.requests[r].output_ids for r in rids]


def _pstats(srv):
    st = srv.stats()
    return tuple(st[k] for k in ("prefix_fills", "prefix_hits", "prefix_tokens_forked", "prefix_evictions",
                                 "prefix_bypass"))


def _record_commands(srv):
    seen = []
    ex = srv._exec
    srv._exec = lambda cmd, *a, **k: (seen.append(cmd), ex(cmd, *a, **k))[1]
    return seen


def test_shared_prefix_load(golden):
    cfg = _cfg()
    srv = _server(cfg)
    cmds = _record_commands(srv)
    prompts = _prompts(cfg)
    assert _run(srv, prompts, cache_prefix=PRE) == [golden(p) for p in prompts]
    assert _pstats(srv) == (1, 6, 6 * PRE, 0, 0)
    assert S.CMD_FORK in cmds
    assert srv.stats()["requests"] == 7 and srv.stats()["tokens"] == 7 * NEW
    assert all(e is None or e.pins == 0 for e in srv.pool)


def test_lookup_without_declaration_partial_match_and_clamp(golden):
    cfg = _cfg()
    srv = _server(cfg)
    prompts = _prompts(cfg)
    assert _run(srv, prompts[:1], cache_prefix=PRE) == [golden(prompts[0])]
    assert _pstats(srv) == (1, 0, 0, 0, 0)
    # an undeclared request finds the ready entry
    assert _run(srv, prompts[1:2]) == [golden(prompts[1])]
    assert _pstats(srv) == (1, 1, PRE, 0, 0)
    # a prompt that shares only the first 12 tokens of the entry forks 12
    g = torch.Generator().manual_seed(9)
    part = prompts[0][:12] + _rand(cfg, g, 7)
    assert part[12] != prompts[0][12]
    assert _run(srv, [part]) == [golden(part)]
    assert _pstats(srv) == (1, 2, PRE + 12, 0, 0)
    # a prompt equal to the declared prefix forks len - 1: its last token is computed
    whole = prompts[0][:PRE]
    assert _run(srv, [whole], cache_prefix=PRE) == [golden(whole)]
    assert _pstats(srv) == (1, 3, PRE + 12 + PRE - 1, 0, 0)


def test_min_match_keeps_short_matches_out(golden):
    cfg = _cfg()
    srv = _server(cfg, prefix_min_match=13)
    prompts = _prompts(cfg)
    g = torch.Generator().manual_seed(9)
    part = prompts[0][:12] + _rand(cfg, g, 7)
    assert _run(srv, prompts[:1], cache_prefix=PRE) == [golden(prompts[0])]
    assert _run(srv, [part]) == [golden(part)]
    assert _pstats(srv) == (1, 0, 0, 0, 0)


def test_eviction_and_refill(golden):
    cfg = _cfg()
    srv = _server(cfg)
    g = torch.Generator().manual_seed(21)
    a, b, c = (_rand(cfg, g, 18) for _ in range(3))
    for i, p in enumerate((a, b)):
        assert _run(srv, [p], cache_prefix=10) == [golden(p)]
    assert _run(srv, [a[:10] + b[10:]]) == [golden(a[:10] + b[10:])]  # a hit makes a's entry the recent one
    assert _pstats(srv) == (2, 1, 10, 0, 0)
    assert _run(srv, [c], cache_prefix=10) == [golden(c)]  # evicts b's entry
    assert _pstats(srv) == (3, 1, 10, 1, 0)
    assert sorted(e.tokens for e in srv.pool) == sorted([a[:10], c[:10]])
    assert _run(srv, [b], cache_prefix=10) == [golden(b)]  # refills it, evicting a's
    assert _pstats(srv) == (4, 1, 10, 2, 0)
    assert sorted(e.tokens for e in srv.pool) == sorted([b[:10], c[:10]])


def test_bypass_when_every_slot_is_pinned(golden):
    cfg = _cfg()
    srv = _server(cfg, prefix_slots=1)
    g = torch.Generator().manual_seed(22)
    ps = [_rand(cfg, g, 30) for _ in range(3)]
    assert _run(srv, ps, cache_prefix=24) == [golden(p) for p in ps]
    fills, hits, _, evictions, bypass = _pstats(srv)
    assert bypass >= 1 and fills + bypass == 3 and hits == 0 and evictions == fills - 1


def test_chosen_prompts_depend_on_the_forked_prefix(golden, monkeypatch):
    """With a fork that copies nothing the SENSITIVE prompts miss the golden tokens: a test on one
    of them notices wrong fork data."""
    from llm_sharding_amd.ops import kvcache
    monkeypatch.setattr(kvcache, "kv_fork_reference", lambda *a, **k: None)
    cfg = _cfg()
    for i in SENSITIVE:
        p = _prompts(cfg)[i]
        assert _run(_server(cfg), [p], cache_prefix=PRE) != [golden(p)], i


def test_submit_n_greedy(golden):
    cfg = _cfg()
    srv = _server(cfg)
    p = _prompts(cfg)[SENSITIVE[0]]
    rids = srv.submit_n(p, 3, NEW, eos_ids=())
    assert rids == sorted(rids) and len(set(rids)) == 3
    srv.serve(stop_when_idle=True)
    assert [srv.requests[r].output_ids for r in rids] == [golden(p)] * 3
    assert _pstats(srv) == (1, 2, 2 * (len(p) - 1), 0, 0)  # one prefill of len - 1 tokens for the three
    assert srv.pool[0].tokens == p[:-1] and srv.pool[0].pins == 0


def test_submit_n_more_children_than_slots(golden):
    cfg = _cfg()
    srv = _server(cfg, prefix_slots=1)
    p = _prompts(cfg)[SENSITIVE[1]]
    other = _prompts(cfg)[SENSITIVE[3]][5:]
    pins = []

    def watch(r, t):  # the entry stays pinned for the children that wait for a slot
        late = sum(1 for w in srv.waiting if w.group is not None)
        pins.append((late, srv.pool[0].pins if srv.pool[0] is not None and srv.pool[0].tokens == p[:-1] else -1))

    rids = srv.submit_n(p, 6, NEW, eos_ids=(), on_token=watch)
    rid = srv.submit(other, NEW, eos_ids=(), cache_prefix=8)  # cannot take the slot while children are left
    srv.serve(stop_when_idle=True)
    assert [srv.requests[r].output_ids for r in rids] == [golden(p)] * 6
    assert srv.requests[rid].output_ids == golden(other)
    assert any(late == 2 for late, _ in pins) and all(n >= late for late, n in pins if late)
    fills, hits, forked, _, bypass = _pstats(srv)
    assert (hits, forked) == (5, 5 * (len(p) - 1)) and fills + bypass == 2


def _sampled(seed):
    cfg = _cfg()
    srv = _server(cfg)
    rids = srv.submit_n(_prompts(cfg)[0], 3, 12, eos_ids=(), sampling=SamplingParams(0.8, seed=seed))
    srv.serve(stop_when_idle=True)
    return srv, [srv.requests[r] for r in rids]


def test_submit_n_sampled():
    srv, rs = _sampled(1234)
    _, rs2 = _sampled(1234)
    outs = [r.output_ids for r in rs]
    assert outs == [r.output_ids for r in rs2]
    assert not (outs[0] == outs[1] == outs[2])
    assert [r.sampling.seed for r in rs] == [1234, 1235, 1236]
    assert _pstats(srv)[0] == 1


def test_submit_n_draws_one_seed():
    srv = _server(_cfg())
    rids = srv.submit_n([5, 6, 7], 3, 2, eos_ids=(), sampling=SamplingParams(0.8))
    srv._intake()
    seeds = [srv.requests[r].sampling.seed for r in rids]
    assert seeds[1] == (seeds[0] + 1) % (1 << 64) and seeds[2] == (seeds[0] + 2) % (1 << 64)


def test_errors():
    cfg = _cfg()
    with pytest.raises(ValueError):
        _server(cfg, prefix_slots=0).submit_n([1, 2, 3], 2)
    with pytest.raises(ValueError):
        _server(cfg, prefix_slots=1, causal=False)
    with pytest.raises(ValueError):
        _server(cfg, prefix_slots=1).submit_n([1, 2, 3], 0)


def test_prefix_slots_zero_is_inert(golden):
    cfg = _cfg()
    srv = _server(cfg, prefix_slots=0)
    assert srv.eng.max_slots == B * M and srv.eng.k_cache[0].shape[0] == B * M
    cmds = _record_commands(srv)
    prompts = _prompts(cfg)
    assert _run(srv, prompts, cache_prefix=PRE) == [golden(p) for p in prompts]  # the declaration is ignored
    assert set(cmds) <= {S.CMD_PREFILL, S.CMD_DECODE}
    assert _pstats(srv) == (0, 0, 0, 0, 0)
    assert _server(cfg, prefix_slots=3).eng.max_slots == B * M + 3


def test_replan_drops_the_registry(golden):
    cfg = _cfg()
    srv = _server(cfg)
    prompts = _prompts(cfg)
    assert _run(srv, prompts[:1], cache_prefix=PRE) == [golden(prompts[0])]
    srv.request_replan([[0, cfg.num_hidden_layers]])
    assert _run(srv, prompts[1:3], cache_prefix=PRE) == [golden(p) for p in prompts[1:3]]
    assert srv.replans == 1 and srv.eng.max_slots == B * M + 2
    assert _pstats(srv) == (2, 1, PRE, 0, 0)  # the entry was filled again on the new engine


@pytest.mark.parametrize("which", SENSITIVE[:3])
def test_submit_n_across_a_replan(golden, which):
    """More children than slots, a re-plan while two of them wait: the entry and its K/V went with
    the engine, so the late children must refill the prefix, not fork the empty pool slot."""
    cfg = _cfg()
    srv = _server(cfg, prefix_slots=1)
    p = _prompts(cfg)[which]
    cmds = []
    ex = srv._exec
    srv._exec = lambda cmd, mb, items, *a, **k: (cmds.append((cmd, srv.replans, list(items))), ex(cmd, mb, items, *a, **k))[1]

    def replan(r, t):
        if srv.replans == 0 and srv._replan is None:
            assert sum(1 for w in srv.waiting if w.group is not None) == 2
            srv.request_replan([[0, cfg.num_hidden_layers]])

    rids = srv.submit_n(p, 6, NEW, eos_ids=(), on_token=replan)
    srv.serve(stop_when_idle=True)
    assert srv.replans == 1
    assert [srv.requests[r].output_ids for r in rids] == [golden(p)] * 6
    # after the re-plan: a fill of the pool slot comes before the first fork from it
    after = [(c, it) for c, n, it in cmds if n == 1]
    first_fork = next(i for i, (c, _) in enumerate(after) if c == S.CMD_FORK)
    assert any(c == S.CMD_PREFILL and any(s == B * M for s, _, _, _ in it) for c, it in after[:first_fork])
    fills, hits, forked, _, _ = _pstats(srv)
    assert (fills, hits, forked) == (2, 4, 4 * (len(p) - 1))
    assert srv.pool[0].pins == 0


def _worker(rank, world, port, q):
    import torch.distributed as dist
    torch.set_num_threads(1)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        ctrl = dist.new_group(backend="gloo")
        cfg = _cfg()
        srv = _server(cfg, rank, world, ctrl)
        if rank == 0:
            q.put((_run(srv, _prompts(cfg), cache_prefix=PRE), _pstats(srv)))
        else:
            srv.serve()
    finally:
        dist.barrier()
        dist.destroy_process_group()


def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("world", [2, 3])
def test_multiprocess_shared_prefix_matches_golden(world, golden):
    """Every stage holds only its own layers' K/V: golden tokens on every request prove that
    CMD_FORK ran on every stage."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in ps:
        p.start()
    try:
        res, stats = q.get(timeout=240)
    finally:
        for p in ps:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in ps), [p.exitcode for p in ps]
    assert res == [golden(p) for p in _prompts(_cfg())]
    assert stats == (1, 6, 6 * PRE, 0, 0)


class _Replies:
    def __init__(self):
        self.sent, self.errors = [], []

    def error(self, reply_to, reason, request_id=None):
        self.errors.append(reason)


def test_ingress_n_and_cache_prefix(golden):
    from llm_sharding_amd.parallel.ingress import Replies, submit_message
    cfg = _cfg()
    srv = _server(cfg)
    sent = []
    replies = Replies(verbose=False)
    replies._send = lambda reply_to, payload: sent.append((reply_to, payload))
    p = _prompts(cfg)[0]
    assert submit_message(srv, {"command": "user_request", "input_ids": p, "max_new_tokens": NEW, "n": 2,
                                "reply_to": "tcp://client:1"}, None, NEW, replies) == 2
    assert submit_message(srv, {"command": "user_request", "input_ids": _prompts(cfg)[1], "max_new_tokens": NEW,
                                "cache_prefix": PRE, "reply_to": "tcp://client:2"}, None, NEW, replies) == 1
    srv.serve(stop_when_idle=True)
    from llm_sharding_amd.parallel import protocol
    msgs = {to: protocol.decode(raw) for to, raw in sent}
    assert len(sent) == 2
    many = msgs["tcp://client:1"]
    eos = set(cfg.eos_ids)
    want = golden(p)
    if any(t in eos for t in want):
        want = want[:next(i for i, t in enumerate(want) if t in eos) + 1]
    assert [c["output_ids"] for c in many["choices"]] == [want, want]
    assert [c["index"] for c in many["choices"]] == [0, 1] and many["output_ids"] == want
    one = msgs["tcp://client:2"]
    assert "choices" not in one and set(one) == {"request_id", "output_ids", "text", "ttft_ms", "tpot_ms"}
    assert _pstats(srv)[:3] == (1, 2, len(p) - 1 + PRE)  # the children's entry covers the declared prefix
    # a child that will never finish must not hold back its finished siblings
    sent.clear()
    g = {"n": 3, "rids": [7, 8, 9]}

    class R:
        eos_ids, max_new_tokens, reply_to, group, ttft_ms, tpot_ms = (), 1, "tcp://client:3", g, 1.0, 0.0

        def __init__(self, rid):
            self.rid, self.output_ids = rid, [rid]

    replies(R(9), 9)
    replies.error("tcp://client:3", "dropped", request_id=7)
    assert [protocol.decode(raw).get("error") for _, raw in sent] == ["dropped"]
    replies(R(8), 8)
    part = protocol.decode(sent[-1][1])
    assert len(sent) == 2 and [(c["index"], c["output_ids"]) for c in part["choices"]] == [(1, [8]), (2, [9])]
    # without a pool, n > 1 is rejected with an error reply
    bare = _server(cfg, prefix_slots=0)
    rep = _Replies()
    assert submit_message(bare, {"command": "user_request", "input_ids": p, "n": 2}, None, NEW, rep) == 0
    assert len(rep.errors) == 1
