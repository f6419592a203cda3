"""KV-cache fork on CPU: the torch reference of the contract against a hand-written loop, the
validation rules, and fork_slots on a StageEngine (a prefix prefilled in one slot and forked into
another continues bit-identically to a prefill that never left its slot)."""
import pytest
import torch

from llm_sharding_amd.config import tiny
from llm_sharding_amd.ops.kvcache import fork_slots, kv_fork_reference, normalize_jobs
from llm_sharding_amd.runtime.engine import RandomSource, StageEngine

LAYERS, SLOTS, NKV, TMAX, HD = 2, 10, 3, 12, 16


def _caches(seed=0):
    g = torch.Generator().manual_seed(seed)
    mk = lambda: [torch.randn((SLOTS, NKV, TMAX, HD), generator=g) for _ in range(LAYERS)]  # noqa: E731
    return mk(), mk()


def _hand_loop(ks, vs, jobs):
    for src, length, dsts in jobs:
        for t in ks + vs:
            for d in dsts:
                for h in range(NKV):
                    for p in range(length):
                        for c in range(HD):
                            t[d, h, p, c] = t[src, h, p, c]


@pytest.mark.parametrize("jobs", [
    [(0, 5, (1,))],
    [(2, 0, (3,))],
    [(4, TMAX, (0, 1, 2))],
    [(9, 1, (0, 1, 2, 3, 4, 5, 6, 7))],
    [(0, 7, (1, 2)), (3, 11, (4,)), (5, 2, (6, 7, 8))],
    [(0, 4, (1,)), (0, 9, (2,))],  # one source, two lengths
])
def test_reference_matches_hand_loop(jobs):
    ks, vs = _caches()
    wk, wv = [t.clone() for t in ks], [t.clone() for t in vs]
    _hand_loop(wk, wv, jobs)
    kv_fork_reference(ks, vs, [(s, n, *d) for s, n, d in jobs])
    for a, b in zip(ks + vs, wk + wv):
        assert torch.equal(a, b)


def test_default_variant_follows_the_call_size():
    from llm_sharding_amd.ops import kvcache
    assert kvcache.default_flags(0) == kvcache.default_flags(kvcache.NT_MIN_BYTES - 1) == 0
    assert kvcache.default_flags(kvcache.NT_MIN_BYTES) == kvcache.NT_LOADS | kvcache.NT_STORES == 3


def test_job_forms():
    assert normalize_jobs([(0, 3, 1, 2), (4, 2, [5])], SLOTS, TMAX) == [(0, 3, (1, 2)), (4, 2, (5,))]


@pytest.mark.parametrize("jobs", [
    [(SLOTS, 1, 0)],  # source out of range
    [(-1, 1, 0)],
    [(0, 1, SLOTS)],  # destination out of range
    [(0, 1, -1)],
    [(0, -1, 1)],  # len outside [0, t_max]
    [(0, TMAX + 1, 1)],
    [(0, 1, 0)],  # destination equal to its source
    [(0, 1, 1, 1)],  # a destination twice in one job
    [(0, 1, 1), (2, 1, 1)],  # ... and in two jobs
    [(0, 1, 1), (1, 1, 2)],  # a destination that is a later source
    [(0, 1, 1), (2, 1, 0)],  # a source that is a later destination
    [(0, 1)],  # no destination
    [(0, 1, 1, 2, 3, 4, 5, 6, 7, 8, 9)],  # fan-out 9
])
def test_refusals_raise_and_write_nothing(jobs):
    ks, vs = _caches()
    wk, wv = [t.clone() for t in ks], [t.clone() for t in vs]
    with pytest.raises(ValueError):
        kv_fork_reference(ks, vs, jobs)
    for a, b in zip(ks + vs, wk + wv):
        assert torch.equal(a, b)


def test_reference_refuses_mismatched_tensors():
    ks, vs = _caches()
    with pytest.raises(ValueError):
        kv_fork_reference(ks, [v[:, :, :-1] for v in vs], [(0, 1, 1)])


def _engine(cfg, slots):
    return StageEngine(cfg, 0, cfg.num_hidden_layers, "cpu", torch.float32, has_embed=True, source=RandomSource(cfg, 3),
                       max_slots=slots, max_seq=64, max_prefill_rows=64)


def _prefill(eng, ids, slot, p0):
    n = len(ids)
    eng.seq_len[slot] = p0
    h = eng.forward(eng.embed(torch.tensor(ids)), [slot] * n, list(range(p0, p0 + n)))
    eng.seq_len[slot] = p0 + n
    return h


def test_fork_slots_continues_bit_identically():
    cfg = tiny(layers=2)
    eng = _engine(cfg, 12)
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(3, cfg.vocab_size, (23,), generator=g).tolist()
    L = 14
    # path A: the whole prompt in slot 0, in two chunks
    _prefill(eng, ids[:L], 0, 0)
    ha = _prefill(eng, ids[L:], 0, L)
    # path B: the prefix in slot 11, forked into ten slots (two fan-out jobs), the rest in two of them
    _prefill(eng, ids[:L], 11, 0)
    fork_slots(eng, 11, list(range(1, 11)), L)
    assert [eng.seq_len[s] for s in range(1, 11)] == [L] * 10 and eng.seq_len[11] == L
    for s in (1, 10):
        assert torch.equal(_prefill(eng, ids[L:], s, L), ha)
    for kc, vc in zip(eng.k_cache, eng.v_cache):
        for s in (1, 10):
            assert torch.equal(kc[s, :, :len(ids)], kc[0, :, :len(ids)])
            assert torch.equal(vc[s, :, :len(ids)], vc[0, :, :len(ids)])
        assert not kc[5, :, L:].any() and not vc[5, :, L:].any()  # nothing beyond the fork length
