"""Speculative decoding with a draft model, without a GPU: ``draft_model_reference`` on a case
worked by hand (the minimum history, the missing cell after a step that accepted every draft, a
sequence at its limit, a finished one), the exactness of ``EagerSpecDecode(draft=...)`` against plain
decode on the fp32 CPU engine, the target as its own draft, and the refusals."""
import numpy as np
import pytest
import torch

import spec_cases as C
from llm_sharding_amd.config import tiny
from llm_sharding_amd.ops import speculative as OS
from llm_sharding_amd.runtime.engine import EagerDecode, RandomSource, StageEngine
from llm_sharding_amd.runtime.sampling import EagerSamplingDecode, Sampler, SamplingParams
from llm_sharding_amd.runtime.speculative import EagerSpecDecode, generate_speculative

MAX_SEQ = 32
K = 3


# ------------------------------------------------------------------------------ the reference, by hand
class SumDraft:
    """A draft 'model' one can run in one's head: a row writes its token into cell (slot, pos); the
    token it proposes is the sum of the cells 0 .. pos of its slot, modulo 97. A cell that was
    never written is an error, a stale one shows in the sum."""

    def __init__(self, n_slots, max_seq):
        self.cells = np.full((n_slots, max_seq), -1, dtype=np.int64)
        self.calls = []

    def prefill(self, slot, tokens):
        self.cells[slot, :len(tokens)] = tokens

    def __call__(self, tokens, pos, slot, out_rows):
        self.calls.append((tokens.tolist(), pos.tolist(), slot.tolist()))
        assert tokens.dtype == pos.dtype == slot.dtype == np.int32
        for t, p, s in zip(tokens, pos, slot):  # every row's K/V is appended before any row attends
            self.cells[s, p] = t
        out = []
        for r in out_rows:
            row = self.cells[slot[r], :pos[r] + 1]
            assert (row >= 0).all(), f"row {r} attends a cell nobody wrote: {row}"
            out.append(int(row.sum()) % 97)
        return out


def test_reference_by_hand():
    # sequence 0: the minimum history; 1: accepts every draft in step 1; 2: at its limit; 3: finished
    slots = [2, 0, 3, 1]
    rows = [[5, 6], [1, 2, 3, 4], list(range(1, 30)), [7, 7, 7]]
    hist, hlen = C.hist_matrix(rows, MAX_SEQ)
    done = np.array([0, 0, 1, 1], dtype=np.int32)
    ctr = np.array([10, 20, 30, 40], dtype=np.int32)
    assert int(hlen[2]) == MAX_SEQ - K  # limit + k == max_seq: the last target row sits at max_seq - 1
    dm = SumDraft(4, MAX_SEQ)
    for s, r in zip(slots, rows):  # admit: hist[0:L-1]
        dm.prefill(s, r[:-1])
    tokens, pos, matched, fed = OS.draft_model_reference(hist, hlen, K, MAX_SEQ, MAX_SEQ, dm, slots, done, ctr)
    assert tokens.tolist() == [6, 11, 22, 44, 4, 10, 20, 40, 29, 47, 94, 91, 7, 21, 42, 84]
    assert pos.tolist() == [1, 2, 3, 4, 3, 4, 5, 6, 28, 29, 30, 31, 2, 3, 4, 5]
    assert matched.tolist() == [1, 1, 1, 1] and ctr.tolist() == [11, 21, 30, 40]
    assert tokens.dtype == pos.dtype == matched.dtype == np.int32
    # iteration 0: two rows per sequence, then one; slots as given
    assert dm.calls[0] == ([5, 6, 3, 4, 28, 29, 7, 7], [0, 1, 2, 3, 27, 28, 1, 2], [2, 2, 0, 0, 3, 3, 1, 1])
    assert dm.calls[1] == ([11, 10, 47, 21], [2, 4, 29, 3], slots)
    assert dm.calls[2] == ([22, 20, 94, 42], [3, 5, 30, 4], slots)
    assert len(dm.calls) == K and [f[0].tolist() for f in fed] == [c[0] for c in dm.calls]
    assert max(max(c[1]) for c in dm.calls) < MAX_SEQ  # no draft row at or beyond the draft's max_seq
    # step 2: sequence 1 accepted all k drafts and the model's bonus token 9 (a == k): cell 6
    # (draft 40) was never fed to the draft - the second-to-last known token is the missing cell
    hist[1, 4:8], hlen[1] = [10, 20, 40, 9], 8
    assert dm.cells[0, 6] == -1 and (dm.cells[0, :6] >= 0).all()
    dm.calls.clear()
    tokens, pos, _, _ = OS.draft_model_reference(hist, hlen, K, MAX_SEQ, MAX_SEQ, dm, slots, done, ctr)
    assert dm.calls[0][0][2:4] == [40, 9] and dm.calls[0][1][2:4] == [6, 7]
    assert tokens[4:8].tolist() == [9, 89, 81, 65] and pos[4:8].tolist() == [7, 8, 9, 10]
    # the others were fed the same rows again: rewriting valid cells changes nothing
    assert tokens[:4].tolist() == [6, 11, 22, 44] and tokens[8:].tolist() == [29, 47, 94, 91, 7, 21, 42, 84]
    assert ctr.tolist() == [12, 22, 30, 40]
    # fewer accepted (a < k): nothing is missing, the catch-up rows rewrite valid cells
    hist[0, 2:4], hlen[0] = [11, 3], 4  # draft 11 accepted, then the model's own 3
    tokens, _, _, _ = OS.draft_model_reference(hist, hlen, K, MAX_SEQ, MAX_SEQ, dm, slots, done, ctr)
    assert tokens[:4].tolist() == [3, 25, 50, 3]  # 5+6+11+3 = 25, 50, 100 % 97


def test_reference_edges():
    dm = SumDraft(1, 8)
    hist, hlen = C.hist_matrix([[7]], 8)
    tokens, pos, _, fed = OS.draft_model_reference(hist, hlen, 2, 8, 8, dm)  # L == 1: the same row twice
    assert fed[0][0].tolist() == [7, 7] and fed[0][1].tolist() == [0, 0] and tokens.tolist() == [7, 7, 14]
    assert pos.tolist() == [0, 1, 2]
    # k == 1: the two catch-up rows are the whole draft
    dm = SumDraft(1, 8)
    hist, hlen = C.hist_matrix([[1, 2, 3]], 8)
    dm.prefill(0, [1, 2])
    tokens, pos, _, fed = OS.draft_model_reference(hist, hlen, 1, 8, 12, dm)
    assert len(fed) == 1 and tokens.tolist() == [3, 6] and pos.tolist() == [2, 3]
    with pytest.raises(ValueError, match="max_seq"):
        OS.draft_model_reference(hist, hlen, 1, 8, 7, dm)  # a draft engine shorter than the target
    with pytest.raises(ValueError):
        OS.draft_model_reference(hist, hlen, 16, 8, 8, dm)
    with pytest.raises(ValueError):
        OS.dm_chain_reference(np.zeros(1, np.int32), hlen, 8, 2, 2, 8, 8, np.zeros(3, np.int32))  # j == k


# ------------------------------------------------------------------------------ engine exactness
NEW = 40
PARAMS = {"greedy": None, "top-p": SamplingParams(0.7, top_p=0.9, seed=11), "top-k": SamplingParams(1.0, top_k=20, seed=5)}
_ENG = {}
_PLAIN = {}


def _engine(name, seed=0, layers=4, **kw):
    if name not in _ENG:
        c = tiny(layers=layers)
        kw = {"max_slots": 2, "max_seq": 128, "has_embed": True, "has_head": True, **kw}
        _ENG[name] = StageEngine(c, 0, kw.pop("end", layers), "cpu", torch.float32, source=RandomSource(c, seed), **kw)
    return _ENG[name]


def _target():
    return _engine("target")


def _plain(which):
    """Plain decode of the target: prefill, first token from the head, one row per step."""
    if which not in _PLAIN:
        eng, sp = _target(), PARAMS[which]
        p = C.prompt(eng.cfg, 0)
        eng.reset()
        slot, pos = eng.prefill_rows([0], [len(p)])
        h = eng.forward(eng.embed(torch.tensor(p)), slot, pos)
        eng.advance([0], [len(p)])
        if sp is None:
            first, g = eng.head(h, [len(p) - 1]), EagerDecode(eng, 1, "full", history_len=NEW)
        else:
            first = Sampler(eng).sample(h, [len(p) - 1], [sp], [len(p)])
            g = EagerSamplingDecode(eng, 1, "full", history_len=NEW)
            g.set_params(0, sp)
        g.tokens.copy_(first.to(torch.int32))
        for _ in range(NEW - 1):
            g.replay()
        _PLAIN[which] = [int(first[0])] + g.history[:NEW - 1, 0].tolist()
    return _PLAIN[which]


@pytest.mark.parametrize("k", [1, 3, 7])
@pytest.mark.parametrize("which", list(PARAMS))
def test_output_is_the_plain_output_with_a_draft_of_other_weights(which, k):
    eng, draft = _target(), _engine("other", seed=1, layers=2)
    p = C.prompt(eng.cfg, 0)
    out, st = generate_speculative(eng, [p], NEW, k=k, sampling=PARAMS[which], draft=draft, ngram=(8, 8))
    assert out == [_plain(which)], st
    assert st["tokens"] == NEW and sum(st["accepted"][0]) == NEW and st["matched_fraction"] == 1.0
    assert eng.seq_len[0] == len(p) + NEW - 1 and draft.seq_len[0] == len(p) + NEW - 2


@pytest.mark.parametrize("k", [1, 3, 7])
def test_the_target_as_its_own_draft_accepts_everything(k):
    """A second engine of the target's weights drafts what the target decodes: every step accepts
    all k drafts and the bonus token, so every step after the first needs the two-row catch-up."""
    eng, draft = _target(), _engine("twin", seed=0)
    out, st = generate_speculative(eng, [C.prompt(eng.cfg, 0)], NEW, k=k, draft=draft)
    assert out == [_plain("greedy")]
    want = [k + 1] * (NEW // (k + 1)) + ([NEW % (k + 1)] if NEW % (k + 1) else [])
    assert st["accepted"] == [want]


def test_two_sequences_permuted_slots_and_eos():
    eng, draft = _target(), _engine("twin", seed=0)
    want = _plain("greedy")
    eos = want[9]
    stop = want.index(eos) + 1
    pa, pb = C.prompt(eng.cfg, 0), C.prompt(eng.cfg, 7, 5, 2)
    eng.reset()
    for s, p in ((1, pa), (0, pb)):
        slot, pos = eng.prefill_rows([s], [len(p) - 1])
        eng.forward(eng.embed(torch.tensor(p[:-1])), slot, pos)
        eng.advance([s], [len(p) - 1])
    g = EagerSpecDecode(eng, 2, 3, slots=[1, 0], history_len=NEW, eos_ids=[eos], draft=draft)
    g.admit(0, pa, NEW, n_prompt=len(pa))
    g.admit(1, pb, 12, n_prompt=len(pb))
    while not g.all_done():
        g.replay()
    ra, rb = g.results()
    assert ra["tokens"] == want[:stop] and ra["done"] and rb["done"]
    g.sync_positions()
    assert eng.seq_len[1] == len(pa) + stop - 1 and draft.seq_len[1] == len(pa) + stop - 2


def test_refusals():
    eng = _target()
    ok = _engine("twin", seed=0)
    EagerSpecDecode(eng, 2, 3, draft=ok)
    with pytest.raises(ValueError, match="script"):
        EagerSpecDecode(eng, 1, 3, script=True, draft=ok)
    with pytest.raises(ValueError, match="engine of its own"):
        EagerSpecDecode(eng, 1, 3, draft=eng)
    with pytest.raises(ValueError, match="all its layers"):
        EagerSpecDecode(eng, 1, 3, draft=_engine("half", layers=4, end=2, has_head=False))
    with pytest.raises(ValueError, match="no lm_head"):
        EagerSpecDecode(eng, 1, 3, draft=_engine("headless", layers=2, has_head=False))
    with pytest.raises(ValueError, match="no embedding"):
        EagerSpecDecode(eng, 1, 3, draft=_engine("embedless", layers=2, has_embed=False))
    with pytest.raises(ValueError, match="whole lm_head"):
        EagerSpecDecode(eng, 1, 3, draft=_engine("split", layers=2, head_cols=(0, 256)))
    small = tiny(layers=2, vocab=384)
    with pytest.raises(ValueError, match="vocab_size 384"):
        EagerSpecDecode(eng, 1, 3, draft=StageEngine(small, 0, 2, "cpu", torch.float32, has_embed=True, has_head=True,
                                                     source=RandomSource(small, 1), max_slots=2, max_seq=128))
    with pytest.raises(ValueError, match="max_seq 64"):
        EagerSpecDecode(eng, 1, 3, draft=_engine("short", layers=2, max_seq=64))
    with pytest.raises(ValueError, match="slots"):
        EagerSpecDecode(eng, 2, 3, draft=_engine("one-slot", layers=2, max_slots=1))
    with pytest.raises(ValueError, match="two draft sources|script"):
        generate_speculative(eng, [[5, 6, 7]], 8, k=2, script=[[5, 6, 7, 8]], draft=ok)


# ------------------------------------------------------------------------------ inference.py
def test_inference_cli(capsys, tiny_shards):
    import inference
    argv = ["--random", "tiny", "--device", "cpu", "--max-new-tokens", "24", "--prompt", "abcabcabcabc"]

    def text(extra):
        capsys.readouterr()
        out = inference.main(argv + extra)
        lines = capsys.readouterr().out.splitlines()
        return out, [ln for ln in lines if not ln.startswith("[INFO]")], [ln for ln in lines if "draft model" in ln]

    plain, plain_text, _ = text([])
    spec, spec_text, info = text(["--speculative", "3", "--draft-random", "tiny8"])
    assert spec == plain and spec_text == plain_text and len(info) == 1 and "tokens per step" in info[0]
    # a checkpoint as the draft (other weights: seed 3), --spec-ngram ignored beside it
    spec, spec_text, info = text(["--speculative", "4", "--draft-shards", tiny_shards, "--spec-ngram", "2,4"])
    assert spec == plain and spec_text == plain_text and len(info) == 1
    for bad in (["--draft-random", "tiny"],                                          # no --speculative
                ["--speculative", "3", "--draft-random", "tiny", "--draft-shards", tiny_shards],
                ["--speculative", "3", "--draft-random", "tiny-gpt2"]):              # another vocabulary
        with pytest.raises(SystemExit):
            inference.main(argv + bad)
