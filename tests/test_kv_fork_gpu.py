"""lsa_kv_fork on the GPU, compared bitwise (int16 views, random bit patterns with NaN encodings)
with kv_fork_reference over whole tensors - exactness and the write footprint at once - plus the
host-side refusals, a destination beyond byte offset 2^32, stream ordering, and the fork inside the
engine and the server (prefix hit, submit_n)."""
import pytest
import torch

from llm_sharding_amd.config import tiny
from llm_sharding_amd.ops import kvcache
from llm_sharding_amd.ops.kvcache import fork_slots, kv_fork, kv_fork_raw, kv_fork_reference
from llm_sharding_amd.parallel.server import PipelineServer
from llm_sharding_amd.runtime.engine import RandomSource, StageEngine
from llm_sharding_amd.runtime.sampling import SamplingParams

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TMAX = 40


def _bits(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-32768, 32768, shape, dtype=torch.int16, generator=g).to(DEV).view(torch.bfloat16)


def _caches(slots, nkv, hd, seed=0, layers=2):
    return ([_bits((slots, nkv, TMAX, hd), seed + i) for i in range(layers)],
            [_bits((slots, nkv, TMAX, hd), seed + 100 + i) for i in range(layers)])


def _same(a, b):
    return all(torch.equal(x.view(torch.int16), y.view(torch.int16)) for x, y in zip(a, b))


def _check(ks, vs, jobs, flags=None):
    wk, wv = [t.clone() for t in ks], [t.clone() for t in vs]
    kv_fork_reference(wk, wv, jobs)
    kv_fork(ks, vs, jobs, flags)
    torch.cuda.synchronize()
    assert _same(ks + vs, wk + wv), jobs


@pytest.mark.parametrize("hd", [16, 64, 128])
@pytest.mark.parametrize("nkv", [1, 3])
def test_small_grid(nkv, hd):
    ks, vs = _caches(6, nkv, hd)
    for n in (0, 1, 7, 39, 40):
        _check(ks, vs, [(0, n, 1)])
        _check(ks, vs, [(5, n, 2, 3, 4)])
    for n in (7, 40):  # two and three jobs with different lengths, one source twice
        _check(ks, vs, [(1, n, 0), (2, 40 - n, 3, 4)])
        _check(ks, vs, [(0, n, 1), (2, 1, 3), (0, 39, 4, 5)])
    ks, vs = _caches(10, nkv, hd, seed=7)
    for n in (0, 1, 7, 39, 40):
        _check(ks, vs, [(9, n, 0, 1, 2, 3, 4, 5, 6, 7)])


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_non_temporal_variants_are_exact(flags):
    ks, vs = _caches(10, 3, 64, seed=3)
    _check(ks, vs, [(9, 39, 0, 1, 2, 3, 4, 5, 6, 7)], flags)
    _check(ks, vs, [(1, 7, 0), (2, 33, 3, 4)], flags)


def test_more_jobs_than_one_launch_holds():
    slots = 80
    ks, vs = _caches(slots, 1, 16, seed=5, layers=1)
    jobs = [(2 * i, 1 + i, 2 * i + 1) for i in range(slots // 2)]
    calls = kvcache.kv_fork_calls()
    _check(ks, vs, jobs)
    assert kvcache.kv_fork_calls() - calls == 2  # 40 jobs: chunks of 24 and 16
    _check(ks, vs, [(0, 40, 1)])
    assert kvcache.kv_fork_calls() - calls == 3  # all tensors, heads and destinations in one launch


@pytest.mark.parametrize("jobs", [
    [(6, 1, (0,))], [(-1, 1, (0,))], [(0, 1, (6,))], [(0, 1, (-1,))],  # a slot out of range
    [(0, -1, (1,))], [(0, TMAX + 1, (1,))],  # len outside [0, t_max]
    [(0, 1, (0,))],  # a destination equal to its source
    [(0, 1, (1, 1))], [(0, 1, (1,)), (2, 1, (1,))],  # a destination twice
    [(0, 1, (1,)), (1, 1, (2,))], [(0, 1, (1,)), (2, 1, (0,))],  # a source that is a destination
])
def test_refusals_leave_the_tensors_unchanged(jobs):
    ks, vs = _caches(6, 3, 64)
    wk, wv = [t.clone() for t in ks], [t.clone() for t in vs]
    rc = kv_fork_raw([t.data_ptr() for t in ks + vs], kvcache.flatten_jobs(jobs), len(jobs), 6, 3, TMAX, 64)
    assert rc == 1  # LSA_BAD_SHAPE, from the launcher's own checks
    with pytest.raises(ValueError):
        kv_fork(ks, vs, jobs)
    torch.cuda.synchronize()
    assert _same(ks + vs, wk + wv)


def test_beyond_4gib():
    slots, nkv, tmax, hd = 260, 32, 2048, 128
    slot_elems = nkv * tmax * hd
    n = slots * slot_elems  # 4.36 GB per tensor
    buf = torch.empty(2 * n + 64, dtype=torch.bfloat16, device=DEV)
    k, v = buf[:n].view(slots, nkv, tmax, hd), buf[n:2 * n].view(slots, nkv, tmax, hd)
    src, dst = 1, 259
    assert dst * slot_elems * 2 > 1 << 32
    want = [_bits((nkv, tmax, hd), 11), _bits((nkv, tmax, hd), 12)]
    guards = []
    for i, t in enumerate((k, v)):
        t[src] = want[i]
        t[dst].zero_()
        flat = buf[i * n:]
        for lo in (dst * slot_elems - 64, (dst + 1) * slot_elems):  # just before and just after the destination
            flat[lo:lo + 64] = _bits((64,), 20 + len(guards))
            guards.append((flat[lo:lo + 64], flat[lo:lo + 64].clone()))
    kv_fork([k], [v], [(src, tmax, dst)])
    torch.cuda.synchronize()
    for i, t in enumerate((k, v)):
        assert torch.equal(t[dst].view(torch.int16), want[i].view(torch.int16))
        assert torch.equal(t[src].view(torch.int16), want[i].view(torch.int16))
    for now, before in guards:
        assert torch.equal(now.view(torch.int16), before.view(torch.int16))


def test_fork_on_a_side_stream_waits_for_the_fill():
    ks, vs = _caches(4, 3, 128, seed=9)
    fill_k, fill_v = _bits((3, TMAX, 128), 31), _bits((3, TMAX, 128), 32)
    side = torch.cuda.Stream(DEV)
    busy = torch.empty(1 << 28, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    for _ in range(8):  # the main stream is busy in front of the fill
        busy.add_(1.0)
    for t in ks:
        t[0] = fill_k
    for t in vs:
        t[0] = fill_v
    ev = torch.cuda.Event()
    ev.record()
    with torch.cuda.stream(side):
        side.wait_event(ev)
        kv_fork(ks, vs, [(0, TMAX, 2, 3)])
    side.synchronize()
    for t, f in zip(ks + vs, [fill_k] * 2 + [fill_v] * 2):
        for d in (2, 3):
            assert torch.equal(t[d].view(torch.int16), f.view(torch.int16))
    torch.cuda.synchronize()


def test_engine_fork_continues_bit_identically():
    cfg = tiny(layers=2)
    eng = StageEngine(cfg, 0, 2, DEV, torch.bfloat16, has_embed=True, source=RandomSource(cfg, 3), max_slots=4,
                      max_seq=64, max_prefill_rows=64)
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(3, cfg.vocab_size, (23,), generator=g).tolist()
    L = 14

    def prefill(chunk, slot, p0):
        eng.seq_len[slot] = p0
        h = eng.forward(eng.embed(torch.tensor(chunk)), [slot] * len(chunk), list(range(p0, p0 + len(chunk))))
        eng.seq_len[slot] = p0 + len(chunk)
        return h.clone()

    prefill(ids[:L], 0, 0)
    ha = prefill(ids[L:], 0, L)
    prefill(ids[:L], 3, 0)
    calls = kvcache.kv_fork_calls()
    fork_slots(eng, 3, [1, 2], L)
    assert kvcache.kv_fork_calls() == calls + 1 and eng.seq_len[1] == eng.seq_len[2] == L
    hb = prefill(ids[L:], 2, L)
    torch.cuda.synchronize()
    assert torch.equal(ha, hb)
    for kc, vc in zip(eng.k_cache, eng.v_cache):
        assert torch.equal(kc[2].view(torch.int16), kc[0].view(torch.int16))
        assert torch.equal(vc[2].view(torch.int16), vc[0].view(torch.int16))


def _gpu_server(cfg, **kw):
    return PipelineServer(cfg, RandomSource(cfg, 11), 0, 1, 0, cfg.num_hidden_layers, device=DEV, batch=2,
                          microbatches=2, max_seq=128, prefill_budget=16, streams=2, prefix_slots=2, **kw)


def _one(srv, prompt, new=8, **kw):
    rid = srv.submit(prompt, new, eos_ids=(), **kw)
    srv.serve(stop_when_idle=True)
    return srv.requests[rid].output_ids


@pytest.fixture(scope="module")
def prompt():
    g = torch.Generator().manual_seed(5)
    return torch.randint(3, tiny(layers=2).vocab_size, (29,), generator=g).tolist()


def test_server_hit_equals_cold(prompt):
    srv = _gpu_server(tiny(layers=2))
    assert srv.graph_mode and srv.S == 2 and srv.eng.max_slots == 6
    calls = kvcache.kv_fork_calls()
    cold = _one(srv, prompt, cache_prefix=20)
    hit = _one(srv, prompt, cache_prefix=20)
    assert len(cold) == 8 and hit == cold
    st = srv.stats()
    assert (st["prefix_fills"], st["prefix_hits"], st["prefix_tokens_forked"]) == (1, 1, 20)
    assert kvcache.kv_fork_calls() == calls + 2


def test_server_submit_n_children_equal_lone_requests(prompt):
    srv = _gpu_server(tiny(layers=2))
    rids = srv.submit_n(prompt, 3, 8, eos_ids=(), sampling=SamplingParams(0.7, seed=5))
    srv.serve(stop_when_idle=True)
    outs = [srv.requests[r].output_ids for r in rids]
    assert srv.stats()["prefix_fills"] == 1
    for i in range(3):
        lone = _one(srv, prompt, sampling=SamplingParams(0.7, seed=5 + i), cache_prefix=len(prompt) - 1)
        assert lone == outs[i], i
    assert srv.stats()["prefix_fills"] == 1
