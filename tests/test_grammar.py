"""Regex-constrained decoding, CPU side: the regex compiler against Python's ``re`` on bytes, the
liveness of prefixes against brute-force enumeration, every refusal, the canonical digest, the
piece-to-bytes tables, the numpy reference against the dense route (``to_token_automaton`` +
``logit_process_reference``) and against a per-token Python walk, and the CPU engine end to end
(EagerSamplingDecode and a one-stage PipelineServer)."""
import itertools
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import grammar_cases as GC
from llm_sharding_amd.config import tiny
from llm_sharding_amd.ops import constraints as K
from llm_sharding_amd.ops import grammar as G
from llm_sharding_amd.parallel.scheduler import plan_stages
from llm_sharding_amd.parallel.server import PipelineServer
from llm_sharding_amd.runtime.engine import RandomSource, StageEngine
from llm_sharding_amd.runtime.sampling import EagerSamplingDecode, GrammarState, Sampler, SamplingParams

SEED = 11

# (pattern, alphabet of the exhaustive check): every supported construct
PATTERNS = [
    (r"(yes|no)", b"yesno"), (r"-?[0-9]{1,3}(\.[0-9]{2})?", b"-.019"), (r"[a-c]{2,5}x", b"abcx"),
    (r"a*b+c?", b"abcd"), (r"(?:ab|a)(bc|c)*", b"abc"), (r"[^a]b.", b"ab\nc"), (r"\d\w\s", b"1a _\t"),
    (r"\D\W\S", b"1a _\t"), (r"a{2}", b"ab"), (r"a{2,}b", b"ab"), (r"a{,2}b", b"ab"), (r"(a|)b", b"ab"),
    (r"", b"ab"), (r"[]a]b", b"]ab["), (r"a{b", b"a{b}"), (r"\x61\.\\", b"a.\\b"), (r"[a\-c]+", b"a-bc"),
    (r"[\d_]*", b"1_a9"), (r"\n\t\r", b"\n\t\rn"), (r"\(\[\{\*\+\?\|\)", b"([{*+?|)"), (r"é(ab)?", "éab".encode()),
    (r"[^\x00-\x60\x7b-\xff]+", b"aZz\x00\xff"), (r"(a|b)*abb", b"abc"), (r"((a|b)(c|d)){1,2}", b"abcd"),
    (r"[a-]x|[-b]y", b"a-bxy"), (r".*a.", b"ab\n"),
]


def _all_strings(alphabet: bytes, n: int):
    for k in range(n + 1):
        for tup in itertools.product(sorted(set(alphabet)), repeat=k):
            yield bytes(tup)


@pytest.mark.parametrize("pattern,alphabet", PATTERNS, ids=[p for p, _ in PATTERNS])
def test_accepts_what_re_fullmatch_accepts(pattern, alphabet):
    d = G.ByteDFA.from_regex(pattern)
    rx = re.compile(pattern.encode())
    for s in _all_strings(alphabet, 5):
        assert d.accepts(s) == bool(rx.fullmatch(s)), s
    rng = np.random.default_rng(len(pattern))
    alpha = np.array(sorted(set(alphabet)), dtype=np.uint8)
    for _ in range(300):
        s = rng.choice(alpha, int(rng.integers(6, 14))).tobytes()
        assert d.accepts(s) == bool(rx.fullmatch(s)), s
    for _ in range(40):                                   # strings that stay alive: most random ones die at once
        s = GC.sample_walk(d, rng, 12)
        assert d.accepts(s) == bool(rx.fullmatch(s)), s
    # trimmed: every state reachable and co-reachable, so alive == a completion exists
    assert d.next.shape == (d.n_states, 256) and d.next.dtype == np.int16 and d.accept.any()


@pytest.mark.parametrize("pattern,alphabet,n", [(r"(yes|no)", b"yesno", 3), (r"-?[0-9]{1,3}(\.[0-9]{2})?", b"-.01", 7),
                                                (r"[a-c]{2,5}x", b"abx", 6), (r"(a|b)*abb", b"ab", 7)])
def test_a_prefix_is_alive_exactly_when_a_completion_exists(pattern, alphabet, n):
    d = G.ByteDFA.from_regex(pattern)
    rx = re.compile(pattern.encode())
    matches = [s for s in _all_strings(alphabet, n) if rx.fullmatch(s)]
    assert matches
    has_completion = {m[:k] for m in matches for k in range(len(m) + 1)}
    # every string of the language over this alphabet is at most n long, or the pattern is unbounded
    # and the prefixes are cut so that a completion within n still exists
    for s in _all_strings(alphabet, 4):
        assert (d.walk(s) != -1) == (s in has_completion), s
    assert d.walk(b"", 0) == 0 and d.walk(b"\xff" * 3) == -1


UNSUPPORTED = [r"^a", r"a$", r"a*?", r"a+?", r"a??", r"a{2}?", r"a*+", r"a++", r"\1", r"(?P<n>a)", r"(?=a)", r"(?!a)",
               r"(?<=a)b", r"(?<!a)b", r"(?i)a", r"(?#c)a", r"\bx", r"\Ax", r"x\Z", r"\Bx", r"[é]", r"é+", r"*a", r"a**",
               r"a{2}{3}", r"(a", r"a)", r"[a", r"[z-a]", r"[\d-z]", r"a{3,2}", r"\xZ1", "a\\", r"\q"]


@pytest.mark.parametrize("pattern", UNSUPPORTED)
def test_what_is_not_supported_raises_value_error(pattern):
    with pytest.raises(ValueError, match="regex"):
        G.ByteDFA.from_regex(pattern)


def test_empty_language_and_state_limit_raise():
    with pytest.raises(ValueError, match="empty language"):
        G.ByteDFA.from_regex(r"a[^\x00-\xff]")
    with pytest.raises(ValueError, match="more than 10"):
        G.ByteDFA.from_regex(r"[ab]{0,20}", max_states=10)
    assert G.ByteDFA.from_regex(r"[ab]{0,9}", max_states=10).n_states == 10
    with pytest.raises(ValueError, match="anchor"):
        G.ByteDFA.from_regex("^a")
    with pytest.raises(ValueError, match="look-ahead"):
        G.ByteDFA.from_regex("(?=a)")
    with pytest.raises(ValueError, match="back-reference"):
        G.ByteDFA.from_regex(r"(a)\1")
    with pytest.raises(ValueError, match="lazy"):
        G.ByteDFA.from_regex("a+?")
    with pytest.raises(ValueError, match="possessive"):
        G.ByteDFA.from_regex("a++")
    with pytest.raises(ValueError, match="flag"):
        G.ByteDFA.from_regex("(?i)a")


def test_two_spellings_of_one_language_share_a_digest():
    same = [(r"a|b", r"[ab]"), (r"(ab)*", r"(?:ab)*(ab)?|"), (r"[0-9]{1,3}", r"\d|\d\d|\d\d\d"),
            (r"a+", r"aa*"), (r"(a|b)*abb", r"[ab]*abb"), (r"x{2,4}", r"xx(x(x)?)?")]
    for p, q in same:
        a, b = G.ByteDFA.from_regex(p), G.ByteDFA.from_regex(q)
        assert a.digest == b.digest and a == b and a.n_states == b.n_states, (p, q)
    assert G.ByteDFA.from_regex("a+").digest != G.ByteDFA.from_regex("a*").digest
    d = G.ByteDFA.from_regex(GC.BIG)
    assert d.n_states == 2000 and d.accept.all()
    assert G.ByteDFA.from_regex(GC.PERMISSIVE).n_states == 1 and G.ByteDFA.from_regex(GC.TIGHT).n_states == 8


def test_pieces_to_bytes():
    sp = ["<unk>", "<s>", "</s>", "<0x0A>", "<0xFF>", "▁Hello", "▁", "world", "▁▁x", "é", "<0xZZ>", "<mask>", "<", "a<b>"]
    assert G.pieces_to_bytes(sp, "sentencepiece") == [b"", b"", b"", b"\n", b"\xff", b" Hello", b" ", b"world", b"  x",
                                                      "é".encode(), b"", b"", b"<", b"a<b>"]
    assert G.detect_kind(sp) == "sentencepiece"
    bl = ["Hello", "Ġworld", "Ċ", "ĠĠ", "Ã©", "<|endoftext|>", "!", "Ā", "日"]
    got = G.pieces_to_bytes(bl, "bytelevel", special=["<|endoftext|>"])
    assert got == [b"Hello", b" world", b"\n", b"  ", "é".encode(), b"", b"!", b"\x00", b""]
    assert G.detect_kind(bl) == "bytelevel"
    # GPT-2's table is a bijection between 256 characters and the 256 bytes
    assert sorted(G._U2B.values()) == list(range(256)) and len(G._U2B) == 256
    with pytest.raises(ValueError):
        G.pieces_to_bytes(sp, "wordpiece")
    vb = G.VocabBytes.from_pieces(G.pieces_to_bytes(sp, "sentencepiece"))
    assert vb.V == len(sp) and vb.token(5) == b" Hello" and vb.token(0) == b"" and vb.data.size % 4 == 0
    assert vb.decode([5, 7, 0, 3]) == b" Helloworld\n"
    from llm_sharding_amd.models.tokenizer import SyntheticByteTokenizer
    sv = G.VocabBytes.from_tokenizer(SyntheticByteTokenizer(300), 300)
    assert sv.V == 300 and sv.token(2) == b"" and sv.token(3) == b"\x00" and sv.token(258) == b"\xff" and sv.token(259) == b""

    class FakeHF:  # the subset of the HF API from_tokenizer touches
        all_special_tokens = ["<s>"]

        def __len__(self):
            return 4

        def convert_ids_to_tokens(self, ids):
            return ["<s>", "▁a", "<0x41>", "b"][:len(ids)]

    hv = G.VocabBytes.from_tokenizer(FakeHF(), 6)
    assert [hv.token(i) for i in range(6)] == [b"", b" a", b"A", b"b", b"", b""]


# ------------------------------------------------------------------------------ reference
def _python_allowed(d, vocab, q, eos):
    out = np.zeros(vocab.V, dtype=bool)
    for v in range(vocab.V):
        t = vocab.token(v)
        out[v] = bool(d.accept[q]) if v in eos else (len(t) > 0 and d.walk(t, q) >= 0)
    return out


@pytest.mark.parametrize("pattern", [r"(yes|no)", r"-?[0-9]{1,3}(\.[0-9]{2})?", r"[a-c]{2,5}x"])
def test_reference_equals_the_dense_route_and_a_python_walk(pattern):
    """Stuck-free cases: the masked sets and the state sequence of ``grammar_mask_reference`` equal
    those of the dense TokenAutomaton under ``logit_process_reference``."""
    V = 300
    vocab = G.VocabBytes.from_pieces(GC.tiny_pieces(V))
    d = G.ByteDFA.from_regex(pattern)
    dense = d.to_token_automaton(vocab, GC.EOS)
    assert dense.n_states == d.n_states + 1 and dense.vocab == V
    ar = GC.Arena(d.n_states + 3)
    base = ar.place(d, 2)
    tb = GC.tables(ar, vocab, 2)
    tb.gstate[1] = tb.gbase[1] = base
    ct = SimpleNamespace(arena=np.array(dense.next), astate=np.array([-1, 0], dtype=np.int32),
                         abase=np.zeros(2, dtype=np.int32), bias_n=np.zeros(2, dtype=np.int32),
                         bias_tok=np.zeros((2, K.BIAS_MAX), dtype=np.int32),
                         bias_val=np.zeros((2, K.BIAS_MAX), dtype=np.float32), min_until=np.zeros(2, dtype=np.int32),
                         minp_delta=np.full(2, -np.inf, dtype=np.float32), fault=np.zeros(2, dtype=np.int32), eos=tb.eos)
    rng = np.random.default_rng(5)
    tin, q = None, 0
    for step in range(12):
        logits = GC.random_logits(rng, 1, V, V + 2)
        got, gst, gflt = G.grammar_mask_reference(logits, V, tb, [1], tin)
        want, ast, aflt = K.logit_process_reference(logits, V, ct, [1], tin, [step])
        assert (got == want).all() and (got[:, V:] == GC.LOGIT_PAD).all(), step
        assert gflt.sum() == 0 and aflt.sum() == 0
        kept = _python_allowed(d, vocab, int(gst[1]) - base, GC.EOS)
        assert (got[0, :V] == np.where(kept, logits[0, :V], GC.NINF_BITS)).all()
        tb.gstate[:], ct.astate[:] = gst, ast
        if tin is not None and tin[0] not in GC.EOS:
            q = d.walk(vocab.token(tin[0]), q)
        assert int(gst[1]) == base + q and (int(ast[1]) == q or tin[0] in GC.EOS or q < 0)
        nxt = int(rng.choice(np.nonzero(kept)[0]))
        if nxt in GC.EOS:
            break
        tin = [nxt]
    # a second evaluation from the same inputs gives the same bits; the inputs are untouched
    snap = logits.copy()
    a = G.grammar_mask_reference(logits, V, tb, [1], tin)
    b = G.grammar_mask_reference(logits, V, tb, [1], tin)
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and (logits == snap).all()


def test_reference_modes_of_the_mixed_case():
    c = GC.mixed_case()
    got, gst, gflt = GC.cached_reference("mixed", c)
    assert set(c.modes) == set(GC.MODES)
    by_mode = {m: [r for r, x in enumerate(c.modes) if x == m] for m in GC.MODES}
    flt = lambda m: {int(gflt[c.slot[r]]) for r in by_mode[m]}  # noqa: E731
    assert flt("forbidden_in") == flt("empty_in") == flt("beyond_v_in") == {G.FAULT_TOKEN}
    assert flt("stuck") == {G.FAULT_STUCK} and flt("tight") == flt("eos_in") == flt("big_step") == {0}
    for r in by_mode["off"] + by_mode["stuck"]:
        assert (got[r] == c.logits[r]).all()
    changed = gst != c.tables.gstate
    assert changed.sum() >= 2 and all(changed[c.slot[r]] for r in by_mode["tight_step"] + by_mode["big_step"])
    assert not any(changed[c.slot[r]] for m in ("forbidden_in", "empty_in", "eos_in", "neg_in", "off") for r in by_mode[m])
    eos = GC.EOS[0]
    for r in by_mode["accept_eos"]:
        assert got[r, eos] == c.logits[r, eos]
    for r in by_mode["nonaccept_eos"]:
        assert got[r, eos] == GC.NINF_BITS
    for r in by_mode["eos_in"] + by_mode["based"]:          # nothing but EOS may follow
        assert ((got[r, :c.V] != GC.NINF_BITS).nonzero()[0] == [eos]).all()
    for r in by_mode["permissive"]:                          # every non-empty printable token survives
        ln = np.diff(c.vocab.offsets)
        printable = np.array([ln[v] > 0 and all(32 <= b < 127 for b in c.vocab.token(v)) for v in range(c.V)])
        assert (got[r, :c.V][printable] == c.logits[r, :c.V][printable]).all()
        printable[eos] = True                                # the state accepts: EOS stays
        assert (got[r, :c.V][~printable] == GC.NINF_BITS).all()
    assert (got[:, c.V:] == GC.LOGIT_PAD).all()
    nan = c.logits[:, :c.V] == GC.NAN_BITS                   # a NaN is masked like any value, or stays
    assert ((got[:, :c.V][nan] == GC.NAN_BITS) | (got[:, :c.V][nan] == GC.NINF_BITS)).all()
    # no input tokens: nothing advances, nothing faults but the stuck rows
    got0, gst0, gflt0 = GC.reference(c, tokens=None)
    assert (gst0 == c.tables.gstate).all() and set(gflt0.tolist()) == {0, G.FAULT_STUCK}
    # a state outside the arena is flagged and its row skipped
    tb = SimpleNamespace(**vars(c.tables))
    tb.gstate = c.tables.gstate.copy()
    s = c.slot[by_mode["tight"][0]]
    tb.gstate[s] = c.tables.arena.shape[0]
    g2 = G.grammar_mask_reference(c.logits[:14], c.V, tb, c.slot[:14], c.tokens[:14])
    assert g2[2][s] == G.FAULT_STATE and (g2[0][by_mode["tight"][0]] == c.logits[by_mode["tight"][0]]).all()


# ------------------------------------------------------------------------------ parameters
def test_sampling_params_regex_field():
    sp = SamplingParams(regex=r"(yes|no)")
    assert sp.grammar == G.ByteDFA.from_regex("(yes|no)") and not sp.plain and not sp.constrained
    assert SamplingParams().grammar is None and SamplingParams().plain
    assert SamplingParams.from_dict({"regex": "a+"}).regex == "a+" and SamplingParams.from_dict({"x": 1}) is None
    with pytest.raises(ValueError, match="regex"):
        SamplingParams(regex="a(")
    with pytest.raises(ValueError, match="str"):
        SamplingParams(regex=5)
    for kw in ({"allowed_token_ids": [3]}, {"choices": [[3]]}, {"automaton": K.TokenAutomaton.from_allowed([1], 8)},
               {"banned_token_ids": [5]}, {"logit_bias": {5: float("-inf")}}, {"min_tokens": 2}):
        with pytest.raises(ValueError, match="regex cannot be combined"):
            SamplingParams(regex="a+", **kw)
    ok = SamplingParams(0.7, top_k=5, top_p=0.9, seed=1, regex="a+", logit_bias={5: 1.5}, min_p=0.1, logprobs=3,
                        repetition_penalty=1.2)
    assert ok.constrained and ok.grammar is not None


# ------------------------------------------------------------------------------ end to end, CPU engine
E2E = [r"(yes|no)", r"-?[0-9]{1,3}(\.[0-9]{2})?", r"[a-c]{2,5}x"]


def _engine(cfg, slots=2):
    return StageEngine(cfg, 0, cfg.num_hidden_layers, "cpu", torch.float32, has_embed=True, has_head=True,
                       source=RandomSource(cfg, SEED), max_slots=slots, max_seq=128)


def _prompt(cfg, n=7, seed=5):
    return torch.randint(3, cfg.vocab_size, (n,), generator=torch.Generator().manual_seed(seed)).tolist()


def _vocab(cfg):
    return G.VocabBytes.from_pieces(GC.tiny_pieces(cfg.vocab_size))


def eager_run(eng, sp, prompt, n_new, slot=1, gs=None):
    """One request on EagerSamplingDecode until EOS or n_new tokens -> (tokens, GrammarState)."""
    from llm_sharding_amd.runtime.sampling import ConstraintState
    gs = GrammarState(eng, eng.max_slots, _vocab(eng.cfg), dfa_rows=64) if gs is None else gs
    cs = ConstraintState(eng, eng.max_slots, state_rows=2) if sp.constrained else None
    eng.reset()
    gs.admit(slot, sp)
    if cs is not None:
        cs.admit(slot, sp, len(prompt))
    sl, pos = eng.prefill_rows([slot], [len(prompt)])
    h = eng.forward(eng.embed(torch.tensor(prompt)), sl, pos)
    eng.advance([slot], [len(prompt)])
    first = Sampler(eng, None, cs, gs).sample(h, [len(prompt) - 1], [sp], [len(prompt)], slots=[slot])
    g = EagerSamplingDecode(eng, 1, "full", slots=[slot], history_len=n_new, constraints=cs, grammar=gs,
                            logprobs=sp.logprobs is not None)
    g.set_params(0, sp)
    g.tokens.copy_(first.to(torch.int32))
    out = [int(first[0])]
    while len(out) < n_new and out[-1] not in eng.cfg.eos_ids:
        g.replay()
        out.append(int(g.tokens[0]))
    return out, gs


def _check_output(pattern, vocab, out, eos=2):
    d = G.ByteDFA.from_regex(pattern)
    body = out[:-1] if out[-1] == eos else out
    assert eos not in body
    for k in range(len(body) + 1):                         # every prefix is alive
        assert d.walk(vocab.decode(body[:k])) >= 0, (pattern, out, k)
    if out[-1] == eos:                                     # finished by EOS: a full match
        assert re.fullmatch(pattern.encode(), vocab.decode(body)), (pattern, vocab.decode(body))
    return out[-1] == eos


@pytest.mark.parametrize("pattern", E2E)
def test_eager_generation_matches_the_pattern(pattern):
    cfg = tiny(layers=2)
    eng, vocab = _engine(cfg), _vocab(cfg)
    finished, multi = 0, 0
    runs = [SamplingParams(0.0, seed=1, regex=pattern)] + [SamplingParams(1.5, seed=s, regex=pattern) for s in (3, 4, 5, 6)]
    runs.append(SamplingParams(1.0, seed=8, regex=pattern, min_p=0.05, logit_bias={2: 1.0, 263: 4.0}, top_k=40))
    for sp in runs:
        out, gs = eager_run(eng, sp, _prompt(cfg), 12)
        finished += _check_output(pattern, vocab, out)
        multi += any(len(vocab.token(t)) > 1 for t in out)
        assert int(gs.gfault.sum()) == 0
        assert eager_run(eng, sp, _prompt(cfg), 12)[0] == out                # deterministic under its seed
    assert finished >= 3 and (multi >= 1 or pattern == E2E[2])
    gs.release(1)
    assert gs.alloc.rows_free() == 64 and int(gs.gstate[1]) == -1


def test_the_checker_fails_without_the_advance_step(monkeypatch):
    """Negative control: a reference that never advances the DFA keeps every row in the start
    state, and the outputs no longer match."""
    ref = G.grammar_mask_reference
    monkeypatch.setattr(G, "grammar_mask_reference", lambda lg, V, tb, slot, tokens_in: ref(lg, V, tb, slot, None))
    cfg = tiny(layers=2)
    eng, vocab = _engine(cfg), _vocab(cfg)
    bad = 0
    for s in (3, 4, 5):
        out, _ = eager_run(eng, SamplingParams(1.5, seed=s, regex=E2E[1]), _prompt(cfg), 12)
        try:
            _check_output(E2E[1], vocab, out)
        except AssertionError:
            bad += 1
    assert bad >= 1


def test_masked_tokens_have_logprob_minus_infinity_and_min_p_sees_the_masked_row():
    cfg = tiny(layers=2)
    eng, vocab = _engine(cfg), _vocab(cfg)
    V = cfg.vocab_size
    gs = GrammarState(eng, 2, vocab, dfa_rows=16)
    sp = SamplingParams(1.0, seed=1, regex=E2E[0], logprobs=5)
    gs.admit(0, sp)
    p = _prompt(cfg)
    sl, pos = eng.prefill_rows([0], [7])
    h = eng.forward(eng.embed(torch.tensor(p)), sl, pos)
    smp = Sampler(eng, None, None, gs)
    tok, lp = smp.sample(h, [6], [sp], [7], slots=[0], return_logprobs=True)
    y, n = GC.token_of(vocab, b"y"), GC.token_of(vocab, b"n")
    allowed = {y, n, GC.token_of(vocab, b"yes"), GC.token_of(vocab, b"no"), GC.token_of(vocab, b"ye")}
    assert int(tok[0]) in allowed
    top = [int(i) for i in lp.top_id[0][:5]]
    assert set(top) == allowed and torch.isfinite(lp.top_lp[0][:5]).all()      # exactly five tokens survive
    masked = gs.apply(smp.logits(h, [6]), [0], None)
    gone = [v for v in range(V) if v not in allowed]
    assert (masked[0, gone].float() == float("-inf")).all() and torch.isfinite(masked[0, sorted(allowed)].float()).all()
    assert float(smp.logprobs(masked, [gone[10]], 0).tok_lp[0]) == float("-inf")
    # min-p runs behind the mask: its maximum is the largest allowed logit, so the row never empties
    from llm_sharding_amd.runtime.sampling import ConstraintState
    cs = ConstraintState(eng, 2, state_rows=1)
    sq = SamplingParams(1.0, seed=1, regex=E2E[0], min_p=1.0)
    cs.admit(0, sq, 7)
    gs.admit(0, sq)
    tok = Sampler(eng, None, cs, gs).sample(h, [6], [sq], [7], slots=[0])
    best = max(allowed, key=lambda v: float(masked[0, v]))
    assert int(tok[0]) == best
    with pytest.raises(RuntimeError, match="GrammarState"):
        Sampler(eng).sample(h, [6], [sp], [7], slots=[0])


def test_grammar_state_admission_checks():
    cfg = tiny(layers=2)
    eng = _engine(cfg)
    with pytest.raises(ValueError, match="VocabBytes"):
        GrammarState(eng, 2, G.VocabBytes.from_pieces(GC.tiny_pieces(300)))
    gs = GrammarState(eng, 2, _vocab(cfg), dfa_rows=12)
    pieces = GC.tiny_pieces(cfg.vocab_size)
    pieces[3 + ord("z")] = b""                                           # a vocabulary without the byte 'z'
    gz = GrammarState(eng, 2, G.VocabBytes.from_pieces(pieces), dfa_rows=12)
    with pytest.raises(ValueError, match="allows no token"):
        gz.admit(0, SamplingParams(regex="az"))
    gz.admit(0, SamplingParams(regex="a[yz]"))                           # 'y' remains
    with pytest.raises(ValueError, match="does not fit"):
        gs.admit(0, SamplingParams(regex="[ab]{0,20}"))
    a, b = SamplingParams(regex="a|b"), SamplingParams(regex="[ab]")
    gs.admit(0, a)
    gs.admit(1, b)
    assert gs.alloc.rows_free() == 10 and int(gs.gstate[0]) == int(gs.gstate[1]) == 0      # shared by digest
    gs.release(0)
    assert gs.alloc.rows_free() == 10
    gs.release(1)
    assert gs.alloc.rows_free() == 12 and not gs.resident
    assert int(gs.accept[1]) == G.ACCEPT | G.LAST and int(gs.accept[0]) == 0


def _server(cfg, world=1, rank=0, batch=2, microbatches=2, **kw):
    st = plan_stages(cfg, world).stages[rank]
    return PipelineServer(cfg, RandomSource(cfg, SEED), rank, world, st.start, st.end, device="cpu", batch=batch,
                          microbatches=microbatches, max_seq=128, prefill_budget=16, dtype=torch.float32, **kw)


def test_server_mixes_regex_and_plain_requests():
    cfg = tiny(layers=2)
    vocab = _vocab(cfg)
    prompts = [_prompt(cfg, n, seed=n) for n in (7, 12, 5, 9, 6)]
    params = [SamplingParams(0.0, seed=1, regex=E2E[0]), SamplingParams(1.5, seed=3, regex=E2E[1]),
              SamplingParams(1.5, seed=4, regex=E2E[2], min_p=0.02), SamplingParams(1.2, seed=5, regex=E2E[1], logprobs=2)]
    plain = SamplingParams(0.8, seed=77)
    srv = _server(cfg, vocab_bytes=vocab, dfa_rows=64)
    assert srv.grammar is None and srv._garena is None
    rids = [srv.submit(p, 12, sampling=sp) for p, sp in zip(prompts, params)]
    rids += [srv.submit(prompts[4], 12, eos_ids=(), sampling=plain), srv.submit(prompts[3], 12, eos_ids=())]
    srv.serve(stop_when_idle=True)
    outs = [srv.requests[r].output_ids for r in rids]
    for sp, o in zip(params, outs):
        _check_output(sp.regex, vocab, o)
    assert sum(o[-1] == 2 for o in outs[:4]) >= 3
    assert all(np.isfinite(srv.requests[rids[3]].token_logprobs))
    assert srv.grammar is not None and int(srv.grammar.gfault.sum()) == 0
    assert srv._garena.rows_free() == 64 and not srv.grammar.held and (srv.grammar.gstate == -1).all()
    # the eager twin gives the same tokens, and requests without a regex what a server without a
    # GrammarState gives them
    eng = _engine(cfg)
    for p, sp, o in zip(prompts, params, outs):
        assert eager_run(eng, sp, p, 12)[0] == o
    bare = _server(cfg)
    b = [bare.submit(prompts[4], 12, eos_ids=(), sampling=plain), bare.submit(prompts[3], 12, eos_ids=())]
    bare.serve(stop_when_idle=True)
    assert bare.grammar is None and bare._garena is None
    assert [bare.requests[r].output_ids for r in b] == outs[4:]


def test_server_refuses_what_cannot_be_served():
    cfg = tiny(layers=2)
    p = _prompt(cfg)
    with pytest.raises(ValueError, match="vocab_bytes"):
        _server(cfg).submit(p, 4, sampling=SamplingParams(regex="a+"))
    srv = _server(cfg, vocab_bytes=_vocab(cfg), dfa_rows=6)
    pieces = GC.tiny_pieces(cfg.vocab_size)
    pieces[3 + ord("z")] = b""                                           # a vocabulary without the byte 'z'
    nz = _server(cfg, vocab_bytes=G.VocabBytes.from_pieces(pieces), dfa_rows=6)
    with pytest.raises(ValueError, match="does not fit"):
        srv.submit(p, 4, sampling=SamplingParams(regex="[ab]{0,20}"))
    with pytest.raises(ValueError, match="allows no token"):
        nz.submit(p, 4, sampling=SamplingParams(regex="az"))
    with pytest.raises(ValueError, match="covers"):
        _server(cfg, vocab_bytes=G.VocabBytes.from_pieces(GC.tiny_pieces(300))).submit(p, 4, sampling=SamplingParams(regex="a"))
    assert srv._garena.rows_free() == 6
    rid = srv.submit(p, 6, sampling=SamplingParams(regex="ab|cd"))
    srv.serve(stop_when_idle=True)
    assert _vocab(cfg).decode(srv.requests[rid].output_ids) in (b"ab", b"cd") and srv.requests[rid].output_ids[-1] == 2
    with pytest.raises(ValueError, match="single-stage"):
        _server(cfg, world=2, vocab_bytes=_vocab(cfg)).submit(p, 4, sampling=SamplingParams(regex="a+"))
    from llm_sharding_amd.runtime.speculative import EagerSpecDecode
    g = EagerSpecDecode(_engine(cfg), 1, 2, sampling=True, history_len=8, eos_ids=cfg.eos_ids)
    with pytest.raises(ValueError, match="regex"):
        g.admit(0, [5], 4, SamplingParams(0.5, seed=1, regex="a+"), n_prompt=1)
    from llm_sharding_amd.parallel.ingress import submit_message

    class Rep:
        errors = []

        def error(self, to, why):
            self.errors.append(why)

        def __call__(self, *a):
            pass

    assert submit_message(srv, {"input_ids": p, "regex": "a(", "max_new_tokens": 4}, None, 4, Rep()) == 0
    assert submit_message(srv, {"input_ids": p, "regex": "(yes|no)", "max_new_tokens": 6}, None, 4, Rep()) == 1
    assert len(Rep.errors) == 1 and "regex" in Rep.errors[0]
    srv.serve(stop_when_idle=True)
    assert _vocab(cfg).decode(srv.finished[-1].output_ids) in (b"yes", b"no")


def test_inference_cli_takes_a_pattern_that_starts_with_a_dash():
    import inference
    a = inference.build_parser().parse_args(inference.join_regex_arg(["--random", "tiny", "--regex", "-?[0-9]{1,3}"]))
    assert a.regex == "-?[0-9]{1,3}"
    sp = inference.sampling_from_args(a)
    assert sp.grammar.accepts(b"-12") and not sp.plain
    out = inference.main(["--random", "tiny", "--regex", "-?[0-9]{1,3}", "--max-new-tokens", "6"])
    body = [t for t in out if t != 2]
    assert re.fullmatch(rb"-?[0-9]{1,3}", bytes(t - 3 for t in body)) and out[-1] == 2
    with pytest.raises(SystemExit):
        inference.main(["--random", "tiny", "--regex", "a+", "--speculative", "2"])
