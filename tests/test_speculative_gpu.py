"""Speculative decoding on the GPU: lsa_spec_draft / lsa_spec_accept bitwise against the numpy
references (footprints included), the captured SpecDecodeGraph against its eager twin, acceptance
not changing the output (the stale-K/V check), the comparison with the plain DecodeGraph (reported
only) and the K/V write footprint."""
import numpy as np
import pytest
import torch

import spec_cases as C
from llm_sharding_amd.config import tiny
from llm_sharding_amd.ops import speculative as OS
from llm_sharding_amd.runtime.engine import DecodeGraph, RandomSource, StageEngine
from llm_sharding_amd.runtime.sampling import SamplingParams
from llm_sharding_amd.runtime.speculative import EagerSpecDecode, SpecDecodeGraph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAX_SEQ = 4128   # the longest history (4099) + k (15) fits
LD = MAX_SEQ + 3  # odd: every other row of hist starts off a 16-byte boundary
SENT = -7


def _dev_rows(a):
    """A [n_seq, LD] numpy matrix on the device, its first row one int32 past a 16-byte boundary."""
    flat = torch.full((a.size + 5,), SENT, dtype=torch.int32, device=DEV)
    view = flat[1:1 + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == 4
    return flat, view


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("vocab", [4, 32000])
@pytest.mark.parametrize("L", [1, 2, 3, 63, 64, 65, 257, 4099])
def test_kernels_bitwise(L, vocab):
    for n_seq in (1, 3, 64):
        for k in (1, 4, 15):
            if n_seq * (k + 1) > OS.MAX_ROWS:
                continue  # 64 x 5 and 64 x 16 rows: refused (test_refusals)
            st = C.random_state(n_seq, L, k, vocab, MAX_SEQ, LD, seed=1000 * n_seq + 10 * k + (vocab > 4))
            rows = n_seq * (k + 1)
            hflat, hist = _dev_rows(st["hist"])
            _, script = _dev_rows(st["script"])
            hlen, done = _dev(st["hlen"]), _dev(st["done"])
            for ngram in ((1, 1), (1, 3), (2, 8), None):  # None: script mode
                outs = []
                for _ in range(3):
                    tokens = torch.full((rows + 4,), SENT, dtype=torch.int32, device=DEV)
                    pos, matched = torch.full_like(tokens, SENT), torch.full((n_seq + 4,), SENT, dtype=torch.int32,
                                                                             device=DEV)
                    ctr = torch.arange(n_seq, dtype=torch.int32, device=DEV)
                    OS.spec_draft(hist, hlen, k, MAX_SEQ, tokens, pos, ngram or (1, 3),
                                  script if ngram is None else None, matched, done, ctr)
                    outs.append([t.cpu().numpy() for t in (tokens, pos, matched, ctr)])
                want_ctr = np.arange(n_seq, dtype=np.int32)
                wt, wp, wm = OS.draft_reference(st["hist"], st["hlen"], k, MAX_SEQ, ngram or (1, 3),
                                                st["script"] if ngram is None else None, st["done"], want_ctr)
                tag = (L, vocab, n_seq, k, ngram)
                for got in outs:
                    assert np.array_equal(got[0][:rows], wt) and np.array_equal(got[1][:rows], wp), tag
                    assert np.array_equal(got[2][:n_seq], wm) and np.array_equal(got[3], want_ctr), tag
                    assert (got[0][rows:] == SENT).all() and (got[1][rows:] == SENT).all(), tag
                    assert (got[2][n_seq:] == SENT).all(), tag
                assert wp.max() < MAX_SEQ and wp.min() >= 0
                if ngram == (1, 3) and vocab == 4 and L >= 63:
                    assert wm.min() >= 1  # matches abound
            # the draft kernel wrote nothing it only reads
            assert np.array_equal(hist.cpu().numpy(), st["hist"]) and (hflat[0] == SENT and (hflat[-4:] == SENT).all())
            assert np.array_equal(hlen.cpu().numpy(), st["hlen"])
            # accept, fed the lookup drafts
            tokens_np, _, _ = OS.draft_reference(st["hist"], st["hlen"], k, MAX_SEQ, (1, 3))
            cand_np = C.random_cand(tokens_np, n_seq, k, vocab, seed=L + k)
            want = {a: st[a].copy() for a in ("hist", "hlen", "done")}
            want_hist, want_step = np.full((3, n_seq + 2), SENT, dtype=np.int32), np.array([1], dtype=np.int32)
            want_nacc = OS.accept_reference(want["hist"], want["hlen"], st["limit"], want["done"], st["eos"], tokens_np,
                                            cand_np, k, MAX_SEQ, want_hist, want_step)
            for _ in range(3):
                hflat, hist = _dev_rows(st["hist"])
                hlen, done = _dev(st["hlen"]), _dev(st["done"])
                n_acc = torch.full((n_seq + 4,), SENT, dtype=torch.int32, device=DEV)
                acc_hist = torch.full((3, n_seq + 2), SENT, dtype=torch.int32, device=DEV)
                step = torch.ones(1, dtype=torch.int32, device=DEV)
                OS.spec_accept(hist, hlen, _dev(st["limit"]), done, _dev(st["eos"]), _dev(tokens_np), _dev(cand_np), k,
                               MAX_SEQ, n_acc, acc_hist, step)
                tag = (L, vocab, n_seq, k, "accept")
                assert np.array_equal(hist.cpu().numpy(), want["hist"]), tag
                assert hflat[0] == SENT and (hflat[-4:] == SENT).all(), tag
                assert np.array_equal(hlen.cpu().numpy(), want["hlen"]), tag
                assert np.array_equal(done.cpu().numpy(), want["done"]), tag
                assert np.array_equal(n_acc.cpu().numpy()[:n_seq], want_nacc) and (n_acc[n_seq:] == SENT).all(), tag
                assert np.array_equal(acc_hist.cpu().numpy(), want_hist) and int(step) == int(want_step[0]) == 2, tag


def test_script_mode_at_the_row_end():
    """L + j >= ld proposes token 0 (and reads nothing beyond the row)."""
    ld, k = 64, 4
    rng = np.random.default_rng(3)
    hist = rng.integers(1, 50, (4, ld)).astype(np.int32)
    script = rng.integers(1, 50, (4, ld)).astype(np.int32)
    hlen = np.array([ld - 5, ld - 2, ld - 1, ld], dtype=np.int32)
    tokens, pos = torch.full((20,), SENT, dtype=torch.int32, device=DEV), torch.full((20,), SENT, dtype=torch.int32,
                                                                                    device=DEV)
    OS.spec_draft(_dev(hist), _dev(hlen), k, ld, tokens, pos, script=_dev(script))
    wt, wp, _ = OS.draft_reference(hist, hlen, k, ld, script=script)
    assert np.array_equal(tokens.cpu().numpy(), wt) and np.array_equal(pos.cpu().numpy(), wp)
    assert wt[5:].tolist().count(0) == 2 + 3 + 4 and wt[1:5].min() >= 1


def test_refusals():
    hist = torch.zeros((4, 64), dtype=torch.int32, device=DEV)
    v = lambda n: torch.zeros(n, dtype=torch.int32, device=DEV)  # noqa: E731
    ok = dict(hist=hist, hlen=v(4) + 1, k=3, max_seq=64, tokens=v(16), pos=v(16))
    OS.spec_draft(**ok)
    for bad in (dict(k=0, tokens=v(4), pos=v(4)), dict(k=16, tokens=v(68), pos=v(68)), dict(ngram=(0, 3)),
                dict(ngram=(3, 2)), dict(ngram=(1, 9)), dict(max_seq=65)):
        with pytest.raises(ValueError):
            OS.spec_draft(**{**ok, **bad})
    big = torch.zeros((64, 64), dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):  # 64 x 5 = 320 rows
        OS.spec_draft(big, v(64) + 1, 4, 64, v(320), v(320))
    acc = dict(hist=hist, hlen=v(4) + 1, limit=v(4) + 9, done=v(4), eos=v(8) - 1, tokens=v(16), cand=v(16), k=3,
               max_seq=64, n_acc=v(4))
    OS.spec_accept(**acc)
    for bad in (dict(k=0), dict(k=16, tokens=v(68), cand=v(68)), dict(max_seq=65)):
        with pytest.raises(ValueError):
            OS.spec_accept(**{**acc, **bad})
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------ engine
CFG = tiny(layers=2)
NEW = 24
LENS = ((12, 7), (6, 3), (9, 5))  # prompts of 19, 9 and 14 tokens: random tokens, then their first ones again
KV_SENT = 0x3F80  # bf16 1.0 in every cell the engine has not written
_ENG = {}
_RUNS = {}


def _engine():
    if "eng" not in _ENG:
        _ENG["eng"] = StageEngine(CFG, 0, 2, DEV, torch.bfloat16, has_embed=True, has_head=True,
                                  source=RandomSource(CFG, 11), max_slots=4, max_seq=128, max_prefill_rows=64)
    return _ENG["eng"]


def _prompts(n_seq):
    return [C.prompt(CFG, 40 + i, *LENS[i]) for i in range(n_seq)]


def _params(n_seq, sampled):
    if not sampled:
        return [None] * n_seq
    return [SamplingParams(0.7, top_p=0.9, seed=11), None, SamplingParams(1.0, top_k=20, seed=5)][:n_seq]


def _prefill(eng, prompts):
    """All but the last token of every prompt, into slots 0.. (the caches start from the sentinel)."""
    for t in eng.k_cache + eng.v_cache:
        t.view(torch.int16).fill_(KV_SENT)
    eng.reset()
    for i, p in enumerate(prompts):
        slot, pos = eng.prefill_rows([i], [len(p) - 1])
        eng.forward(eng.embed(torch.tensor(p[:-1])), slot, pos)
        eng.advance([i], [len(p) - 1])


def _run(cls, n_seq, k, sampled, scripts=None, eos=(), extra_replays=0):
    """One run to completion on freshly prefilled slots: NEW replays cover every outcome (a step
    accepts at least one token); the graph is replayed with no host read in between."""
    eng, prompts = _engine(), _prompts(n_seq)
    _prefill(eng, prompts)
    g = cls(eng, n_seq, k, script=scripts is not None, sampling=sampled, history_len=NEW + 4, eos_ids=eos)
    for i, p in enumerate(prompts):
        g.admit(i, p, NEW, _params(n_seq, sampled)[i], n_prompt=len(p))
        if scripts is not None:
            g.set_script(i, scripts[i])
    g.capture()
    for _ in range(NEW):
        g.replay()
        if cls is EagerSpecDecode and g.all_done():
            break
    res = g.results()
    st = g.host_state()
    out = {"tokens": [r["tokens"] for r in res], "accepted": [r["accepted"] for r in res],
           "hlen": st["hlen"].tolist(), "done": st["done"].tolist(), "graph": g}
    if extra_replays:
        before = {a: getattr(g, a).clone() for a in ("hist", "hlen", "done", "limit", "match_ctr")}
        for _ in range(extra_replays):
            g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(getattr(g, a), v) for a, v in before.items())
        assert int(g.n_acc.abs().sum()) == 0
    return out


def _lookup_graph(n_seq, k, sampled):
    key = (n_seq, k, sampled)
    if key not in _RUNS:
        _RUNS[key] = _run(SpecDecodeGraph, n_seq, k, sampled, extra_replays=2)
    return _RUNS[key]


def _same(a, b):
    return all(a[f] == b[f] for f in ("tokens", "accepted", "hlen", "done"))


CASES = [(1, 3), (1, 7), (3, 3), (3, 7)]  # 4, 8, 12 and 24 rows


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
@pytest.mark.parametrize("n_seq,k", CASES)
def test_graph_equals_eager_twin_lookup(n_seq, k, sampled):
    a = _lookup_graph(n_seq, k, sampled)
    assert all(a["done"]) and all(len(t) == NEW for t in a["tokens"])
    assert all(sum(acc) == NEW for acc in a["accepted"])
    b = _run(EagerSpecDecode, n_seq, k, sampled)
    assert _same(a, b), (a["tokens"], b["tokens"], a["accepted"], b["accepted"])


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
@pytest.mark.parametrize("n_seq,k", CASES)
def test_graph_equals_eager_twin_script(n_seq, k, sampled):
    base, prompts = _lookup_graph(n_seq, k, sampled), _prompts(n_seq)
    scripts = [C.corrupt(p + t, len(p), CFG.vocab_size) for p, t in zip(prompts, base["tokens"])]
    a = _run(SpecDecodeGraph, n_seq, k, sampled, scripts, extra_replays=1)
    b = _run(EagerSpecDecode, n_seq, k, sampled, scripts)
    assert _same(a, b), (a["tokens"], b["tokens"], a["accepted"], b["accepted"])
    assert all(a["done"]) and min(min(acc) for acc in a["accepted"]) >= 1


def test_graph_equals_eager_twin_with_eos():
    base = _lookup_graph(3, 3, False)
    eos = [base["tokens"][1][5]]  # sequence 1 stops at (or before) its sixth token
    a = _run(SpecDecodeGraph, 3, 3, False, eos=eos, extra_replays=1)
    b = _run(EagerSpecDecode, 3, 3, False, eos=eos)
    assert _same(a, b)
    n1 = len(a["tokens"][1])
    assert n1 <= 6 and a["tokens"][1][-1] == eos[0] and a["tokens"][1] == base["tokens"][1][:n1] and all(a["done"])


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
@pytest.mark.parametrize("n_seq,k", [(1, 3), (3, 7)])
def test_acceptance_does_not_change_the_output(n_seq, k, sampled):
    """Run B drafts run A's own output, so every draft is accepted: the same tokens in fewer steps.
    A stale K/V cell surviving a rejected draft of run A would show as a different token here."""
    a, prompts = _lookup_graph(n_seq, k, sampled), _prompts(n_seq)
    scripts = [p + t for p, t in zip(prompts, a["tokens"])]
    b = _run(SpecDecodeGraph, n_seq, k, sampled, scripts)
    assert b["tokens"] == a["tokens"], (a["tokens"], b["tokens"])
    for acc_a, acc_b in zip(a["accepted"], b["accepted"]):
        want, left = [], NEW
        while left:
            want.append(min(k + 1, left))
            left -= want[-1]
        assert acc_b == want and len(acc_b) <= len(acc_a)
    assert max(len(x) for x in b["accepted"]) < max(len(x) for x in a["accepted"])


def test_against_the_plain_decode_graph_report_only(capsys):
    """The common prefix with the 1-row DecodeGraph is printed, not asserted: another row count may
    select another GEMV configuration, hence other bf16 rounding at near-ties."""
    eng, p = _engine(), _prompts(1)[0]
    spec = _lookup_graph(1, 3, False)["tokens"][0]
    _prefill(eng, [p])
    g = DecodeGraph(eng, 1, "full", history_len=NEW)
    g.tokens.copy_(torch.tensor([p[-1]], dtype=torch.int32))
    g.capture()
    for _ in range(NEW):
        g.replay()
    torch.cuda.synchronize()
    plain = g.history[:NEW, 0].tolist()
    same = next((i for i, (x, y) in enumerate(zip(spec, plain)) if x != y), NEW)
    with capsys.disabled():
        print(f"\n[speculative] common prefix with the plain 1-row DecodeGraph: {same}/{NEW} tokens")
    assert len(plain) == len(spec) == NEW


def test_kv_footprint():
    """Slots outside the graph and positions >= limit + k of its slots keep the sentinel."""
    n_seq, k = 3, 7
    out = _run(SpecDecodeGraph, n_seq, k, False)
    eng, g = _engine(), out["graph"]
    torch.cuda.synchronize()
    for t in eng.k_cache + eng.v_cache:
        bits = t.view(torch.int16)
        assert (bits[3] == KV_SENT).all()
        for i in range(n_seq):
            assert (bits[i, :, g.limits[i] + k:, :] == KV_SENT).all()
            assert not (bits[i, :, :g.limits[i] - 1, :] == KV_SENT).all()
