"""Speculative decoding without a GPU: the draft / accept references on hand-built states, the
exactness of the speculative output against plain decode on the CPU engine (greedy and seeded
sampling, lookup and scripted drafts), the refusals and the inference.py flags."""
import numpy as np
import pytest
import torch

import spec_cases as C
from llm_sharding_amd.config import tiny, tiny_gpt2
from llm_sharding_amd.ops import speculative as OS
from llm_sharding_amd.runtime.engine import EagerDecode, RandomSource, StageEngine
from llm_sharding_amd.runtime.sampling import EagerSamplingDecode, Sampler, SamplingParams
from llm_sharding_amd.runtime.speculative import EagerSpecDecode, SpecDecodeGraph, generate_speculative

MAX_SEQ = 64


# ------------------------------------------------------------------------------ draft reference
@pytest.mark.parametrize("name,hist,k,ngram,want,matched", C.DRAFT_CASES, ids=[c[0] for c in C.DRAFT_CASES])
def test_draft_reference_by_hand(name, hist, k, ngram, want, matched):
    h, hlen = C.hist_matrix([hist], MAX_SEQ, fill=-9)
    tokens, pos, m = OS.draft_reference(h, hlen, k, MAX_SEQ, ngram)
    L = len(hist)
    assert tokens.tolist() == [hist[-1]] + want
    assert pos.tolist() == list(range(L - 1, L + k))
    assert m.tolist() == [matched]


def test_draft_reference_script_mode_and_counters():
    ld = MAX_SEQ
    h, hlen = C.hist_matrix([[1, 2, 3], list(range(40, 40 + ld - 2))], ld)  # 3 and ld - 2 known tokens
    script = np.arange(2 * ld, dtype=np.int32).reshape(2, ld) + 100
    ctr = np.zeros(2, dtype=np.int32)
    tokens, pos, m = OS.draft_reference(h, hlen, 5, MAX_SEQ, script=script, done=np.array([0, 1]), match_ctr=ctr)
    assert tokens[:6].tolist() == [3, 103, 104, 105, 106, 107] and pos[:6].tolist() == [2, 3, 4, 5, 6, 7]
    # the second sequence knows ld - 2 tokens: two proposals are left, L + j >= ld proposes token 0
    assert pos[6:].tolist() == list(range(61, 67)) and tokens[6] == 40 + 61
    assert tokens[7:].tolist() == [100 + ld + 62, 100 + ld + 63, 0, 0, 0]
    assert m.tolist() == [1, 1] and ctr.tolist() == [1, 0]  # a done sequence is drafted but not counted
    full, fl = C.hist_matrix([list(range(1, ld + 1))], ld)   # L = ld: nothing left to propose
    tokens, pos, _ = OS.draft_reference(full, fl, 2, MAX_SEQ, script=script[:1])
    assert tokens.tolist() == [ld, 0, 0] and pos.tolist() == [ld - 1, ld, ld + 1]


# ------------------------------------------------------------------------------ accept reference
def _accept(hist, cand, drafts, limit, done=0, eos=(), k=None):
    """One sequence: known ``hist``, the step's drafts and the model's tokens. Returns the reference's
    results and the history row (sentinel -9 beyond the known tokens)."""
    k = len(drafts) if k is None else k
    h, hlen = C.hist_matrix([hist], MAX_SEQ, fill=-9)
    tokens = np.array([hist[-1]] + list(drafts), dtype=np.int32)
    d = np.array([done], dtype=np.int32)
    ah, sc = np.full((2, 1), -9, dtype=np.int32), np.zeros(1, dtype=np.int32)
    n_acc = OS.accept_reference(h, hlen, np.array([limit]), d, OS.eos_array(eos), tokens, np.array(cand, dtype=np.int32),
                                k, MAX_SEQ, ah, sc)
    return int(n_acc[0]), int(hlen[0]), int(d[0]), h[0], ah[:, 0].tolist(), int(sc[0])


@pytest.mark.parametrize("cand,m", [([50, 51, 52, 53], 1),   # none of the drafts: the model's own token only
                                    ([11, 12, 52, 53], 3),   # two of three
                                    ([11, 12, 13, 53], 4)])  # all of them, plus the bonus token
def test_accept_reference_counts(cand, m):
    hist = [1, 2, 3, 4, 5]
    n_acc, hlen, done, row, ah, sc = _accept(hist, cand, [11, 12, 13], limit=40)
    assert (n_acc, hlen, done) == (m, 5 + m, 0)
    assert row[:5 + m].tolist() == hist + cand[:m] and (row[5 + m:] == -9).all()  # nothing beyond [L, L + m)
    assert ah == [m, -9] and sc == 1


def test_accept_reference_limit_eos_done():
    hist, drafts = [1, 2, 3, 4, 5], [11, 12, 13]
    # the limit clamp: one token remains, all drafts right
    assert _accept(hist, [11, 12, 13, 53], drafts, limit=6)[:3] == (1, 6, 1)
    assert _accept(hist, [11, 12, 13, 53], drafts, limit=8)[:3] == (3, 8, 1)
    assert _accept(hist, [11, 12, 13, 53], drafts, limit=9)[:3] == (4, 9, 1)
    assert _accept(hist, [11, 12, 13, 53], drafts, limit=10)[:3] == (4, 9, 0)
    # EOS at j = 0, in the middle, at the bonus token
    assert _accept(hist, [11, 12, 13, 53], drafts, 40, eos=[11])[:3] == (1, 6, 1)
    assert _accept(hist, [11, 12, 13, 53], drafts, 40, eos=[7, 12])[:3] == (2, 7, 1)
    assert _accept(hist, [11, 12, 13, 53], drafts, 40, eos=[53])[:3] == (4, 9, 1)
    # EOS beyond the accepted prefix does not end the sequence
    n_acc, hlen, done, row, _, _ = _accept(hist, [11, 50, 13, 2], drafts, 40, eos=[13, 2])
    assert (n_acc, hlen, done) == (2, 7, 0) and row[:7].tolist() == hist + [11, 50] and (row[7:] == -9).all()
    # ... nor does a draft that is an EOS id the model did not produce
    assert _accept(hist, [50, 51, 52, 53], [11, 12, 13], 40, eos=[11])[:3] == (1, 6, 0)
    # a done sequence is left untouched
    n_acc, hlen, done, row, ah, sc = _accept(hist, [11, 12, 13, 53], drafts, 40, done=1)
    assert (n_acc, hlen, done) == (0, 5, 1) and row[:5].tolist() == hist and (row[5:] == -9).all()
    assert ah == [-9, -9] and sc == 1
    with pytest.raises(ValueError):
        OS.eos_array(range(9))


def test_reference_refusals():
    h, hlen = C.hist_matrix([[1, 2, 3]], MAX_SEQ)
    for k in (0, 16):
        with pytest.raises(ValueError):
            OS.draft_reference(h, hlen, k, MAX_SEQ)
    for ngram in ((0, 3), (3, 2), (1, 9)):
        with pytest.raises(ValueError):
            OS.draft_reference(h, hlen, 3, MAX_SEQ, ngram)
    with pytest.raises(ValueError):
        OS.draft_reference(h, hlen, 3, MAX_SEQ + 1)  # ld < max_seq
    big, bl = C.hist_matrix([[1]] * 33, MAX_SEQ)
    with pytest.raises(ValueError):
        OS.draft_reference(big, bl, 3, MAX_SEQ)  # 132 rows


# ------------------------------------------------------------------------------ engine exactness
NEW = 64
PARAMS = {"greedy": None, "top-p": SamplingParams(0.7, top_p=0.9, seed=11), "top-k": SamplingParams(1.0, top_k=20, seed=5)}
_ENG = {}
_PLAIN = {}


def _engine(seed, cfg=None, **kw):
    key = (seed, None if cfg is None else cfg.name, tuple(sorted(kw.items())))
    if key not in _ENG:
        c = cfg or tiny()
        _ENG[key] = StageEngine(c, 0, c.num_hidden_layers, "cpu", torch.float32, has_embed=True, has_head=True,
                                source=RandomSource(c, seed), max_slots=2, max_seq=128, **kw)
    return _ENG[key]


def _plain(eng, prompt, new, sp=None):
    """Today's path: prefill, first token from the head, EagerDecode / EagerSamplingDecode."""
    eng.reset()
    slot, pos = eng.prefill_rows([0], [len(prompt)])
    h = eng.forward(eng.embed(torch.tensor(prompt)), slot, pos)
    eng.advance([0], [len(prompt)])
    if sp is None:
        first, g = eng.head(h, [len(prompt) - 1]), EagerDecode(eng, 1, "full", history_len=new)
    else:
        first = Sampler(eng).sample(h, [len(prompt) - 1], [sp], [len(prompt)])
        g = EagerSamplingDecode(eng, 1, "full", history_len=new)
        g.set_params(0, sp)
    g.tokens.copy_(first.to(torch.int32))
    for _ in range(new - 1):
        g.replay()
    return [int(first[0])] + g.history[:new - 1, 0].tolist()


def _plain_cached(seed, which):
    if (seed, which) not in _PLAIN:
        eng = _engine(seed)
        _PLAIN[seed, which] = _plain(eng, C.prompt(eng.cfg, seed), NEW, PARAMS[which])
    return _PLAIN[seed, which]


@pytest.mark.parametrize("which", list(PARAMS))
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_speculative_output_is_the_plain_output(seed, which):
    eng, sp = _engine(seed), PARAMS[which]
    p, want = C.prompt(eng.cfg, seed), _plain_cached(seed, which)
    for k in (1, 4, 7):
        out, st = generate_speculative(eng, [p], NEW, k=k, sampling=sp)
        assert out == [want], (k, st)
        assert st["tokens"] == NEW and sum(st["accepted"][0]) == NEW and st["steps"] == len(st["accepted"][0])
        assert eng.seq_len[0] == len(p) + NEW - 1
    # every draft right: 64 tokens in 12 steps of 5 and one of 4
    out, st = generate_speculative(eng, [p], NEW, k=4, sampling=sp, script=[p + want])
    assert out == [want] and st["steps"] == 13 and st["accepted"] == [[5] * 12 + [4]]
    assert st["mean_accepted"] == NEW / 13
    # every third generated position of the script wrong
    out, st = generate_speculative(eng, [p], NEW, k=4, sampling=sp,
                                   script=[C.corrupt(p + want, len(p), eng.cfg.vocab_size)])
    assert out == [want] and st["steps"] == 22 and st["accepted"] == [[1] + [3] * 21]


def test_two_sequences_one_hits_eos():
    eng = _engine(2)
    pa, pb = C.prompt(eng.cfg, 2), C.prompt(eng.cfg, 7, 5, 2)
    wa, wb = _plain_cached(2, "greedy"), _plain(eng, C.prompt(eng.cfg, 7, 5, 2), 40)
    eos = wb[9]
    stop_a = wa[:40].index(eos) + 1 if eos in wa[:40] else 40
    stop_b = wb.index(eos) + 1
    assert stop_b <= 10
    out, st = generate_speculative(eng, [pa, pb], 40, k=4, eos_ids=[eos])
    assert out == [wa[:stop_a], wb[:stop_b]]
    assert [sum(a) for a in st["accepted"]] == [stop_a, stop_b] and len(st["accepted"][1]) < len(st["accepted"][0])
    assert eng.seq_len[:2] == [len(pa) + stop_a - 1, len(pb) + stop_b - 1]


def test_tiny_gpt2_greedy():
    cfg = tiny_gpt2(layers=2)
    eng = _engine(3, cfg)
    p = C.prompt(cfg, 3)
    want = _plain(eng, p, 32)
    for k in (2, 5):
        out, _ = generate_speculative(eng, [p], 32, k=k)
        assert out == [want]


def test_admit_after_a_full_prefill_and_results():
    """The documented admission: the prompt prefilled whole, its first token from the head."""
    eng = _engine(1)
    p, want = C.prompt(eng.cfg, 1), _plain_cached(1, "greedy")
    eng.reset()
    slot, pos = eng.prefill_rows([1], [len(p)])
    h = eng.forward(eng.embed(torch.tensor(p)), slot, pos)
    eng.advance([1], [len(p)])
    first = int(eng.head(h, [len(p) - 1])[0])
    g = EagerSpecDecode(eng, 1, 4, slots=[1], history_len=NEW)
    with pytest.raises(ValueError):
        g.admit(0, p, NEW)                      # the slot holds one position more than that
    g.admit(0, p + [first], NEW)
    while not g.all_done():
        g.replay()
    r = g.results()[0]
    assert r["tokens"] == want and r["done"] and sum(r["accepted"]) == NEW - 1
    g.sync_positions()
    assert eng.seq_len[1] == len(p) + NEW - 1
    before = (g.hist.copy(), g.hlen.copy())
    g.replay()                                  # a finished sequence: nothing changes
    assert np.array_equal(g.hist, before[0]) and np.array_equal(g.hlen, before[1]) and g.n_acc.tolist() == [0]


# ------------------------------------------------------------------------------ refusals
def test_refusals():
    eng = _engine(0)
    eng.reset()
    for k in (0, 16):
        with pytest.raises(ValueError):
            EagerSpecDecode(eng, 1, k)
    with pytest.raises(ValueError, match="distinct"):
        EagerSpecDecode(eng, 2, 3, slots=[1, 1])
    with pytest.raises(ValueError):
        EagerSpecDecode(eng, 33, 3)             # 132 rows
    with pytest.raises(RuntimeError):
        SpecDecodeGraph(eng, 1, 3)              # a CPU engine
    g = EagerSpecDecode(eng, 1, 4, sampling=True)
    g.admit(0, [5], 128 - 4 - 1, n_prompt=1)                # limit + k == max_seq: the last admissible
    with pytest.raises(ValueError, match="max_seq"):
        g.admit(0, [5], 128 - 4, n_prompt=1)
    with pytest.raises(ValueError, match="max_seq"):
        generate_speculative(eng, [[5, 6, 7]], 122, k=4)
    for sp in (SamplingParams(0.7, seed=1, repetition_penalty=1.2), SamplingParams(0.7, seed=1, presence_penalty=0.5),
               SamplingParams(0.0, logprobs=0)):
        with pytest.raises(ValueError, match="penalties and logprobs"):
            g.admit(0, [5], 8, sp, n_prompt=1)
    with pytest.raises(ValueError, match="sampling=True"):
        EagerSpecDecode(eng, 1, 4).admit(0, [5], 8, SamplingParams(0.7, seed=1), n_prompt=1)
    with pytest.raises(ValueError, match="vocabulary"):
        g.admit(0, [eng.cfg.vocab_size], 8, n_prompt=1)
    split = _engine(0, head_cols=(0, eng.cfg.head_rows // 2))
    with pytest.raises(NotImplementedError, match="split head"):
        EagerSpecDecode(split, 1, 4)


# ------------------------------------------------------------------------------ inference.py
def test_inference_cli(capsys):
    import inference
    argv = ["--random", "tiny", "--device", "cpu", "--max-new-tokens", "24", "--prompt", "abcabcabcabc"]

    def text(extra):
        capsys.readouterr()
        out = inference.main(argv + extra)
        lines = capsys.readouterr().out.splitlines()
        return out, [ln for ln in lines if not ln.startswith("[INFO]")]

    plain, plain_text = text([])
    spec, spec_text = text(["--speculative", "4"])
    assert spec == plain and spec_text == plain_text
    capsys.readouterr()
    inference.main(argv + ["--speculative", "4", "--spec-ngram", "2,4"])
    assert "tokens per step" in capsys.readouterr().out
    sampled, sampled_text = text(["--temperature", "0.8", "--top-p", "0.9", "--seed", "4"])
    spec_s, spec_s_text = text(["--speculative", "3", "--temperature", "0.8", "--top-p", "0.9", "--seed", "4"])
    assert spec_s == sampled and spec_s_text == sampled_text
    for bad in (["--repetition-penalty", "1.2"], ["--presence-penalty", "0.5"], ["--frequency-penalty", "0.5"],
                ["--logprobs", "2"], ["--score"], ["--hf-compare", "x"]):
        with pytest.raises(SystemExit):
            inference.main(argv + ["--speculative", "4"] + bad)
    for bad in (["--speculative", "-1"], ["--speculative", "16"], ["--speculative", "4", "--spec-ngram", "3,2"],
                ["--speculative", "4", "--spec-ngram", "x"]):
        with pytest.raises(SystemExit):
            inference.main(argv + bad)
