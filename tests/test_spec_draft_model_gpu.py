"""Speculative decoding with a draft model on the GPU: lsa_spec_dm_begin / lsa_spec_dm_chain bitwise
against the numpy references (footprints included), the captured SpecDecodeGraph(draft=...) against
its eager twin, the draft source not changing the output, run-to-run determinism and the comparison
with the plain DecodeGraph (reported only)."""
import numpy as np
import pytest
import torch

import spec_cases as C
from llm_sharding_amd.config import tiny
from llm_sharding_amd.ops import speculative as OS
from llm_sharding_amd.runtime.engine import DecodeGraph, RandomSource, StageEngine
from llm_sharding_amd.runtime.engine_int4 import make_stage_engine
from llm_sharding_amd.runtime.sampling import SamplingParams
from llm_sharding_amd.runtime.speculative import EagerSpecDecode, SpecDecodeGraph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -7


def _dev(a, pad=0):
    """``a`` on the device, followed by ``pad`` sentinel cells."""
    a = np.ascontiguousarray(a)
    t = torch.full((a.size + pad,), SENT, dtype=torch.int32, device=DEV)
    t[:a.size].copy_(torch.from_numpy(a.reshape(-1)))
    return t


# ------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("k", [1, 3, 15])
@pytest.mark.parametrize("n_seq", [1, 3, 17])
def test_kernels_bitwise(n_seq, k):
    max_seq, ld, dmax, vocab = 64, 67, 80, 32000
    if n_seq * (k + 1) > OS.MAX_ROWS:  # 17 x 16 rows: refused
        hist = torch.zeros((n_seq, ld), dtype=torch.int32, device=DEV)
        v = lambda n: torch.zeros(n, dtype=torch.int32, device=DEV)  # noqa: E731
        with pytest.raises(ValueError):
            OS.spec_dm_begin(hist, v(n_seq) + 2, v(n_seq), k, max_seq, dmax, v(2 * n_seq), v(2 * n_seq), v(2 * n_seq),
                             v(n_seq * (k + 1)), v(n_seq * (k + 1)))
        with pytest.raises(ValueError):
            OS.spec_dm_chain(v(n_seq), v(n_seq) + 2, ld, k, 0, max_seq, dmax, v(n_seq * (k + 1)), v(n_seq), v(n_seq))
        return
    rng = np.random.default_rng(100 * n_seq + k)
    limit = max_seq - k
    hist = rng.integers(0, vocab, (n_seq, ld)).astype(np.int32)
    # the minimum history, a history at its limit, anything in between; every third of them finished
    hlen = np.array([(2, limit, int(rng.integers(3, limit)))[s % 3] for s in range(n_seq)], dtype=np.int32)
    done = np.array([int(s % 3 == 1 or s % 5 == 2) for s in range(n_seq)], dtype=np.int32)
    slots = rng.permutation(n_seq + 2)[:n_seq].astype(np.int32)
    rows = n_seq * (k + 1)
    want_ctr = np.arange(n_seq, dtype=np.int32)
    want = OS.dm_begin_reference(hist, hlen, slots, k, max_seq, dmax, done, want_ctr)
    assert want["d_pos"].max() < dmax and want["d_pos"].min() >= 0 and want["pos"].max() < max_seq
    hist_d = _dev(hist, 4)
    hist_v = hist_d[:hist.size].view(n_seq, ld)
    hlen_d, slots_d, done_d = _dev(hlen), _dev(slots), _dev(done)
    for _ in range(2):
        d_tok, d_pos, d_slot = (_dev(np.full(2 * n_seq, SENT, np.int32), 4) for _ in range(3))
        tokens, pos = _dev(np.full(rows, SENT, np.int32), 4), _dev(np.full(rows, SENT, np.int32), 4)
        matched, ctr = _dev(np.full(n_seq, SENT, np.int32), 4), _dev(np.arange(n_seq, dtype=np.int32), 4)
        OS.spec_dm_begin(hist_v, hlen_d, slots_d, k, max_seq, dmax, d_tok, d_pos, d_slot, tokens, pos, matched, done_d,
                         ctr)
        got_tokens = tokens.cpu().numpy()
        r0 = np.arange(n_seq) * (k + 1)
        assert np.array_equal(d_tok.cpu().numpy()[:2 * n_seq], want["d_tokens"])
        assert np.array_equal(d_pos.cpu().numpy()[:2 * n_seq], want["d_pos"])
        assert np.array_equal(d_slot.cpu().numpy()[:2 * n_seq], want["d_slot"])
        assert np.array_equal(got_tokens[r0], want["tokens"][r0])
        assert (np.delete(got_tokens, r0) == SENT).all()  # begin writes row 0's token only
        assert np.array_equal(pos.cpu().numpy()[:rows], want["pos"])
        assert np.array_equal(matched.cpu().numpy()[:n_seq], want["matched"])
        assert np.array_equal(ctr.cpu().numpy()[:n_seq], want_ctr)
        for t in (d_tok, d_pos, d_slot, tokens, pos, matched, ctr):
            assert (t[-4:] == SENT).all()
        # the chain, fed arbitrary arg-max tokens
        want_tokens = want["tokens"].copy()
        d_tok1, d_pos1 = _dev(np.full(n_seq, SENT, np.int32), 4), _dev(np.full(n_seq, SENT, np.int32), 4)
        for j in range(k):
            amax = rng.integers(0, vocab, n_seq).astype(np.int32)
            nxt = OS.dm_chain_reference(amax, hlen, ld, k, j, max_seq, dmax, want_tokens)
            before = (d_tok1.clone(), d_pos1.clone())
            OS.spec_dm_chain(_dev(amax), hlen_d, ld, k, j, max_seq, dmax, tokens, d_tok1, d_pos1)
            got = tokens.cpu().numpy()
            written = np.concatenate([r0 + i for i in range(j + 2)])
            assert np.array_equal(got[written], want_tokens[written]), (n_seq, k, j)
            assert (np.delete(got, written) == SENT).all()
            if nxt is None:
                assert torch.equal(d_tok1, before[0]) and torch.equal(d_pos1, before[1])
            else:
                assert np.array_equal(d_tok1.cpu().numpy()[:n_seq], nxt[0])
                assert np.array_equal(d_pos1.cpu().numpy()[:n_seq], nxt[1]) and nxt[1].max() < dmax
            assert (d_tok1[-4:] == SENT).all() and (d_pos1[-4:] == SENT).all()
        assert np.array_equal(tokens.cpu().numpy()[:rows], want_tokens)
    # the kernels wrote nothing they only read
    assert np.array_equal(hist_v.cpu().numpy(), hist) and (hist_d[-4:] == SENT).all()
    assert np.array_equal(hlen_d.cpu().numpy(), hlen) and np.array_equal(slots_d.cpu().numpy(), slots)
    # the composed reference, fed the same chain, says the same
    seq = iter(rng.integers(0, vocab, (k, n_seq)).astype(np.int32))
    t, p, m, fed = OS.draft_model_reference(hist, hlen, k, max_seq, dmax, lambda *a: next(seq), slots, done)
    assert np.array_equal(p, want["pos"]) and np.array_equal(fed[0][0], want["d_tokens"]) and len(fed) == k


def test_refusals():
    v = lambda n, fill=0: torch.full((n,), fill, dtype=torch.int32, device=DEV)  # noqa: E731
    hist = torch.zeros((4, 64), dtype=torch.int32, device=DEV)
    ok = dict(hist=hist, hlen=v(4, 2), slots=v(4), k=3, max_seq=64, draft_max_seq=64, d_tokens=v(8), d_pos=v(8),
              d_slot=v(8), tokens=v(16), pos=v(16))
    OS.spec_dm_begin(**ok)
    for bad in (dict(k=0, tokens=v(4), pos=v(4)), dict(k=16, tokens=v(68), pos=v(68)), dict(max_seq=65),
                dict(draft_max_seq=63), dict(d_tokens=v(7)), dict(slots=v(3))):
        with pytest.raises(ValueError):
            OS.spec_dm_begin(**{**ok, **bad})
    ch = dict(amax=v(4), hlen=v(4, 2), ld=64, k=3, j=0, max_seq=64, draft_max_seq=64, tokens=v(16), d_tokens1=v(4),
              d_pos1=v(4))
    OS.spec_dm_chain(**ch)
    OS.spec_dm_chain(**{**ch, "j": 2, "d_tokens1": None, "d_pos1": None})  # the last iteration feeds no further row
    for bad in (dict(j=3), dict(j=-1), dict(draft_max_seq=63), dict(d_tokens1=None), dict(tokens=v(15))):
        with pytest.raises(ValueError):
            OS.spec_dm_chain(**{**ch, **bad})
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------ engine
CFG = tiny(layers=2)
NEW = 24          # tokens per sequence, and replays: a step accepts at least one token
N_SEQ, K = 3, 3
SLOTS = [2, 0, 3]  # permuted, one slot of the engines unused
LENS = ((12, 7), (6, 3), (9, 5))
_ENG = {}
_RUNS = {}


def _engine(name):
    """target; twin: its weights again; other: other weights; fp8 / int4: the twin's weights quantised."""
    if name not in _ENG:
        seed = 1 if name == "other" else 11
        wd = name if name in ("fp8", "int4") else "bf16"
        _ENG[name] = make_stage_engine(CFG, 0, 2, DEV, torch.bfloat16, has_embed=True, has_head=True,
                                       source=RandomSource(CFG, seed), max_slots=4, max_seq=128, max_prefill_rows=64,
                                       weight_dtype=wd)
    return _ENG[name]


def _prompts(n_seq=N_SEQ):
    return [C.prompt(CFG, 40 + i, *LENS[i]) for i in range(n_seq)]


def _params(sampled):
    if not sampled:
        return [None] * N_SEQ
    return [SamplingParams(0.7, top_p=0.9, seed=11), None, SamplingParams(1.0, top_k=20, seed=5)]


def _start(g, scripts=None, sampled=False):
    """Prefill the target's slots and admit every sequence (which prefills the draft's)."""
    eng, prompts = _engine("target"), _prompts(g.n_seq)
    eng.reset()
    for s, p in zip(g.slots, prompts):
        slot, pos = eng.prefill_rows([s], [len(p) - 1])
        eng.forward(eng.embed(torch.tensor(p[:-1])), slot, pos)
        eng.advance([s], [len(p) - 1])
    for i, p in enumerate(prompts):
        g.admit(i, p, NEW, _params(sampled)[i], n_prompt=len(p))
        if scripts is not None:
            g.set_script(i, scripts[i])


def _finish(g):
    for _ in range(NEW):
        g.replay()
        if isinstance(g, EagerSpecDecode) and g.all_done():
            break
    st = g.host_state()
    return {"tokens": [r["tokens"] for r in g.results()], "accepted": st["acc_history"][:NEW].tolist(),
            "hlen": st["hlen"].tolist(), "done": st["done"].tolist(), "graph": g}


def _run(cls, draft, sampled, scripts=None, n_seq=N_SEQ, k=K):
    g = cls(_engine("target"), n_seq, k, slots=SLOTS[:n_seq], script=scripts is not None, sampling=sampled,
            history_len=NEW + 4, draft=None if draft is None else _engine(draft))
    _start(g, scripts, sampled)
    g.capture()
    return _finish(g)


def _graph_run(draft, sampled):
    if (draft, sampled) not in _RUNS:
        _RUNS[draft, sampled] = _run(SpecDecodeGraph, draft, sampled)
    return _RUNS[draft, sampled]


def _same(a, b):
    return all(a[f] == b[f] for f in ("tokens", "accepted", "hlen", "done"))


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
@pytest.mark.parametrize("draft", ["twin", "other", "fp8", "int4"])
def test_graph_equals_eager_twin(draft, sampled):
    """24 replays of the captured step against the numpy reference around the engines' eager calls:
    tokens and per-step accepted counts."""
    a = _graph_run(draft, sampled)
    assert all(a["done"]) and all(len(t) == NEW for t in a["tokens"])
    assert [sum(col) for col in zip(*a["accepted"])] == [NEW] * N_SEQ
    b = _run(EagerSpecDecode, draft, sampled)
    assert _same(a, b), (a["tokens"], b["tokens"], a["accepted"], b["accepted"])


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
def test_graph_equals_eager_twin_one_sequence(sampled):
    """One sequence, k = 7: the draft engine's 2-row and 1-row steps."""
    a = _run(SpecDecodeGraph, "other", sampled, n_seq=1, k=7)
    b = _run(EagerSpecDecode, "other", sampled, n_seq=1, k=7)
    assert a["done"] == [1] and len(a["tokens"][0]) == NEW
    assert _same(a, b), (a["tokens"], b["tokens"], a["accepted"], b["accepted"])


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
def test_the_draft_source_does_not_change_the_output(sampled):
    """The target itself (a second engine of its weights), a draft of other weights and script mode
    fed the run's own output: the same tokens, only the step counts differ."""
    a, b = _graph_run("twin", sampled), _graph_run("other", sampled)
    scripts = [p + t for p, t in zip(_prompts(), a["tokens"])]
    c = _run(SpecDecodeGraph, None, sampled, scripts)
    assert a["tokens"] == b["tokens"] == c["tokens"], (a["tokens"], b["tokens"], c["tokens"])
    steps = [sum(1 for row in r["accepted"] if any(row)) for r in (a, b, c)]
    assert steps[2] == -(-NEW // (K + 1)) and steps[2] <= min(steps[0], steps[1]) and max(steps) <= NEW


def test_three_runs_of_one_graph_are_bitwise_equal():
    first = _graph_run("other", True)
    g = first["graph"]
    for _ in range(2):
        _start(g, sampled=True)
        g.step_ctr.zero_()
        g.acc_history.zero_()
        again = _finish(g)
        assert _same(first, again)


def test_against_the_plain_decode_graph_report_only(capsys):
    """The common prefix with the 1-row DecodeGraph is printed, not asserted: another row count may
    select another GEMV configuration, hence other bf16 rounding at near-ties."""
    eng, p = _engine("target"), _prompts()[0]
    spec = _graph_run("twin", False)["tokens"][0]
    eng.reset()
    slot, pos = eng.prefill_rows([0], [len(p) - 1])
    eng.forward(eng.embed(torch.tensor(p[:-1])), slot, pos)
    eng.advance([0], [len(p) - 1])
    g = DecodeGraph(eng, 1, "full", history_len=NEW)
    g.tokens.copy_(torch.tensor([p[-1]], dtype=torch.int32))
    g.capture()
    for _ in range(NEW):
        g.replay()
    torch.cuda.synchronize()
    plain = g.history[:NEW, 0].tolist()
    same = next((i for i, (x, y) in enumerate(zip(spec, plain)) if x != y), NEW)
    with capsys.disabled():
        print(f"\n[speculative, draft model] common prefix with the plain 1-row DecodeGraph: {same}/{NEW} tokens")
    assert len(plain) == len(spec) == NEW
