"""JSON mode off the device (ops/pda.py): the hand-built JSON automaton against an independent
oracle on a seeded corpus, the depth limit, the vectorised reference against the plain per-token
walker, the parameter checks, and generation end to end on the CPU engine (EagerSamplingDecode and a
one-stage PipelineServer beside a regex request and a plain one)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import grammar_cases as GC
import pda_cases as PC
from llm_sharding_amd.config import tiny
from llm_sharding_amd.ops import grammar as G
from llm_sharding_amd.ops import pda as J
from llm_sharding_amd.parallel.scheduler import plan_stages
from llm_sharding_amd.parallel.server import PipelineServer
from llm_sharding_amd.runtime.engine import RandomSource, StageEngine
from llm_sharding_amd.runtime.sampling import EagerSamplingDecode, GrammarState, Sampler, SamplingParams

SEED = 7
CORPUS_SEED = 5


# ------------------------------------------------------------------------------ the automaton
def test_tables_and_validation():
    pda = J.BytePDA.json()
    assert pda.next.shape == (3, pda.n_states, 256) and pda.next.dtype == np.int16 and pda.accept.dtype == np.uint8
    assert pda.n_states == 65 and 3 * pda.n_states * 512 <= 128 * 1024          # fits the kernel's LDS path
    assert J.BytePDA.json() is pda and J.BytePDA.json(max_ws=1) != pda
    assert J.BytePDA(pda.next, pda.accept) == pda and len({pda, J.BytePDA(pda.next, pda.accept)}) == 1
    # only , } ] depend on the top symbol
    differ = np.nonzero((pda.next[0] != pda.next[1]) | (pda.next[1] != pda.next[2]))[1]
    assert set(differ.tolist()) == {ord(","), ord("}"), ord("]")}
    bad = np.array(pda.next)
    for fix, err in ((lambda a: a[:2], "3, states, 256"), (lambda a: a[:, :, :255], "3, states, 256"),
                     (lambda a: np.full_like(a, 4 << 10), "op in 0..3"), (lambda a: np.full_like(a, -2), "op in 0..3"),
                     (lambda a: np.full_like(a, pda.n_states), "outside"),
                     (lambda a: np.zeros((3, 1024, 256), dtype=np.int16), "1023")):
        a = fix(bad.copy())
        with pytest.raises(ValueError, match=err):
            J.BytePDA(a, np.zeros(a.shape[1] if a.ndim == 3 else 1, dtype=np.uint8))
    for kw in ({"top_level": "array"}, {"max_ws": 9}, {"max_ws": -1}, {"max_ws": True}):
        with pytest.raises(ValueError):
            J.BytePDA.json(**kw)


@pytest.mark.parametrize("max_ws", (2, 0, 1))
def test_the_language_equals_an_independent_oracle(max_ws):
    pda = J.BytePDA.json(max_ws=max_ws)
    texts = PC.corpus(CORPUS_SEED, max_ws, n=260 if max_ws == 2 else 700)   # fewer separators fit a smaller max_ws
    assert all(len(t) <= 200 for t in texts)
    want = [PC.ok(t, max_ws) for t in texts]
    wrong = [t for t, w in zip(texts, want) if pda.accepts(t) != w]
    assert not wrong, wrong[:5]
    assert sum(want) >= 200 and len(want) - sum(want) >= 200, (sum(want), len(want))
    for t in [t for t, w in zip(texts, want) if w][::3]:                       # every proper prefix is alive
        c = (0, 0, 0)
        for b in t:
            c = pda.step(c, b)
            assert c is not None, t
    # what the corpus must hold to mean something
    assert any(b"\\u" in t for t, w in zip(texts, want) if w) and any(b"\xf0\x9f" in t for t, w in zip(texts, want) if w)
    assert any(b"NaN" in t or b"Infinity" in t for t in texts)


def test_hand_picked_texts():
    pda = J.BytePDA.json()
    yes = [b"{}", b' {"a":1} ', b'{"a":[1,2.5e-3,true,false,null,{"b":"\\u00e9\xc3\xa9\\n"}]}', b'{"":-0}', b'{"a":0E+1}',
           b'{"a" : [ ] }', b'{"a":"\xf4\x8f\xbf\xbf\xed\x9f\xbf\xee\x80\x80"}', b'{"a":"\\ud800"}', b'\r\n{"a":{}}\n\n']
    no = [b"", b"[]", b"12", b'"x"', b"null", b'{"a":01}', b'{"a":1.}', b'{"a":.5}', b'{"a":+1}', b'{"a":1e}', b"{'a':1}",
          b'{"a":1,}', b'{"a":[1,]}', b'{"a":[}', b'{"a":1]', b'{"a":tru}', b'{"a":"\t"}', b'{"a":"\\x"}', b'{"a":"\\u12g4"}',
          b'{"a":"\xc0\xaf"}', b'{"a":"\xe0\x9f\xbf"}', b'{"a":"\xed\xa0\x80"}', b'{"a":"\xf4\x90\x80\x80"}', b'{"a":"\xf8"}',
          b'{"a":"\x80"}', b'{"a":"\xc3"}', b'{"a":1}x', b'{"a":1}   ', b'   {"a":1}', b'{"a":   1}', b'{"a" 1}', b'{1:1}',
          b'{"a":NaN}', b'{"a":-Infinity}', b'{"a":1}{', b"{}}"]
    for t in yes:
        assert pda.accepts(t) and PC.ok(t), t
    for t in no:
        assert not pda.accepts(t) and not PC.ok(t), t


def test_depth_limit():
    """MAX_DEPTH = 64 counts every open bracket: the top-level object and 63 arrays inside it are
    alive, the 65th push dies."""
    pda = J.BytePDA.json()
    at64 = PC.deep(64)
    c = pda.walk(at64)
    assert c is not None and c[1] == 64 and c[2] == (1 << 64) - 2            # the object below 63 arrays
    assert pda.walk(at64 + b"[") is None and pda.walk(at64 + b"{") is None
    assert pda.walk(at64 + b'"x"') is not None
    closed = at64 + b"]" * 63 + b"}"
    assert pda.accepts(closed) and PC.ok(closed)
    over = PC.deep(65) + b"]" * 64 + b"}"
    assert not pda.accepts(over) and not PC.ok(over)
    assert pda.walk(PC.deep(63) + b"{")[1:] == (64, (1 << 63) - 2)            # an object on top: bit 63 clear


def test_top_level_any():
    a, o = J.BytePDA.json(top_level="any"), J.BytePDA.json()
    for t in (b"12", b'"x"', b"null", b" -1.5e3 ", b"[1,{}]", b"{}"):
        assert a.accepts(t), t
    for t in (b"12", b'"x"', b"null"):
        assert not o.accepts(t), t
    for t in (b"", b"1 2", b"12,", b"]", b"tru"):
        assert not a.accepts(t), t


# ------------------------------------------------------------------------------ the reference
def _configs(pda):
    return [(0, 0, 0), pda.walk(b"{"), pda.walk(b'{"a":"x'), pda.walk(b'{"a":[[1'), pda.walk(PC.deep(63)),
            pda.walk(PC.deep(64)), pda.walk(PC.deep(64) + b"1"), pda.walk(b"{}"), pda.walk(PC.deep(63) + b'{"k":7')]


def test_the_vectorised_reference_equals_the_python_walker():
    pda = J.BytePDA.json()
    vocab = PC.json_vocab(np.random.default_rng(31), 700, 14)
    assert all(GC.token_of(vocab, p) > 258 for p in PC.SPECIAL_TOKENS)
    configs = _configs(pda)
    assert {c[1] for c in configs} >= {0, 1, 63, 64}
    nxt = pda.next
    n_allowed = []
    for c in configs:
        got = J.allowed_reference(nxt, pda.accept, vocab, c, PC.EOS)
        want = J.allowed_python(pda, vocab, c, PC.EOS)
        assert (got == want).all(), (c, np.nonzero(got != want)[0][:5])
        n_allowed.append(int(got.sum()))
        q, d, st = J._walk_tokens(nxt, vocab, c)
        for v in range(0, vocab.V, 7):                                        # the walked configurations too
            w = pda.walk(vocab.token(v), c) if vocab.token(v) else None
            assert (w is None and q[v] < 0) or w == (int(q[v]), int(d[v]), int(st[v])), (c, v)
    assert min(n_allowed) >= 1 and n_allowed[5] < n_allowed[4]               # at depth 64 the pushes are gone
    assert got[PC.EOS[0]] == 0 and J.allowed_reference(nxt, pda.accept, vocab, configs[7], PC.EOS)[PC.EOS[0]]


def test_reference_contract_on_the_mixed_case():
    c = PC.mixed_case()
    assert set(c.modes) == set(PC.MODES) and len(c.modes) == 129
    lg, gstate, jstate, jdepth, jstack, gfault = PC.cached_reference("mixed", c)
    tb, eos = c.tables, PC.EOS[0]
    for r, m in enumerate(c.modes):
        s = int(c.slot[r])
        old = (int(tb.jstate[s]), int(tb.jdepth[s]), int(np.uint64(tb.jstack[s].view(np.uint64))))
        new = (int(jstate[s]), int(jdepth[s]), int(jstack[s].view(np.uint64)))
        alive = lg[r, :c.V] != GC.NINF_BITS
        if m == "off":
            assert (lg[r] == c.logits[r]).all() and gfault[s] == 0
        elif m == "regex":
            assert gstate[s] != tb.gstate[s] and new[0] == -1 and 0 < alive.sum() < c.V // 8 and gfault[s] == 0
        elif m in ("forbidden_in", "beyond_v_in", "empty_in"):
            assert gfault[s] == G.FAULT_TOKEN and new == old
        elif m in ("step_push", "step_pop"):
            want = c.pda.walk({"step_push": b'{"a":[[', "step_pop": b'{"b":[[7]]}'}[m])
            assert new == want and gfault[s] == 0 and bool(alive[eos]) == (m == "step_pop")
        else:
            assert new == old and gfault[s] == 0
        if m == "accept":
            assert alive[eos]
        if m in ("nonaccept", "d0", "in_string", "d64"):
            assert not alive[eos]
        if m == "d64":
            assert not alive[GC.token_of(c.vocab, b"[")] and alive[GC.token_of(c.vocab, b"]")]
        if m == "d63":
            assert alive[GC.token_of(c.vocab, b"[")] and not alive[GC.token_of(c.vocab, b'{"a":[[')]
        if m == "after_top0":
            assert alive[GC.token_of(c.vocab, b"}")] and not alive[GC.token_of(c.vocab, b"]")]
        if m == "after_top1":
            assert alive[GC.token_of(c.vocab, b"]")] and not alive[GC.token_of(c.vocab, b"}")]
        assert (lg[r, c.V:] == GC.LOGIT_PAD).all()
    # a configuration out of range, and one that allows nothing
    tb2 = SimpleNamespace(**vars(tb))
    tb2.jstate, tb2.jdepth = tb.jstate.copy(), tb.jdepth.copy()
    s2, s3 = int(c.slot[2]), int(c.slot[3])
    tb2.jstate[s2], tb2.jdepth[s3] = c.pda.n_states, 65
    out = J.pda_mask_reference(c.logits[2:4], c.V, tb2, c.slot[2:4], None)
    assert out[4][s2] == out[4][s3] == G.FAULT_STATE and (out[0] == c.logits[2:4]).all()


# ------------------------------------------------------------------------------ parameters
def test_sampling_params_json_object_field():
    sp = SamplingParams(json_object=True)
    assert sp.json_object and sp.greedy and not sp.plain and sp.grammar is None and GrammarState.wants(sp)
    assert not SamplingParams().json_object and SamplingParams().plain and not GrammarState.wants(SamplingParams(0.5))
    for kw in ({"regex": "a"}, {"allowed_token_ids": [1]}, {"choices": [[1]]}, {"banned_token_ids": [1]},
               {"logit_bias": {1: float("-inf")}}, {"min_tokens": 2},
               {"automaton": __import__("llm_sharding_amd.ops.constraints", fromlist=["x"]).TokenAutomaton.from_allowed([1], 4)}):
        with pytest.raises(ValueError, match="json_object cannot be combined"):
            SamplingParams(json_object=True, **kw)
    with pytest.raises(ValueError, match="bool"):
        SamplingParams(json_object=1)
    ok = SamplingParams(0.7, top_k=5, top_p=0.9, json_object=True, logit_bias={3: 1.5}, min_p=0.1, repetition_penalty=1.1,
                        logprobs=2)
    assert ok.json_object and ok.constrained and ok.penalized
    d = SamplingParams.from_dict
    assert d({"json_object": True}).json_object and d({"response_format": {"type": "json_object"}}).json_object
    assert d({"response_format": {"type": "text"}}) is None and d({"json_object": False}) is None and d({}) is None
    assert d({"temperature": 0.5, "response_format": {"type": "json_object"}}).temperature == 0.5
    for fmt in ({"type": "json_schema"}, "json_object", {}):
        with pytest.raises(ValueError, match="response_format"):
            d({"response_format": fmt})
    with pytest.raises(ValueError, match="cannot be combined"):
        d({"regex": "a+", "response_format": {"type": "json_object"}})


def _engine(cfg, slots=2):
    return StageEngine(cfg, 0, cfg.num_hidden_layers, "cpu", torch.float32, has_embed=True, has_head=True,
                       source=RandomSource(cfg, SEED), max_slots=slots, max_seq=128)


def _vocab(cfg):
    return G.VocabBytes.from_pieces(GC.tiny_pieces(cfg.vocab_size))


def _prompt(cfg, n=7, seed=5):
    return torch.randint(3, cfg.vocab_size, (n,), generator=torch.Generator().manual_seed(seed)).tolist()


def test_the_vocabulary_check():
    cfg = tiny(layers=2)
    eng, pda = _engine(cfg), J.BytePDA.json()
    J.check_vocab(pda, _vocab(cfg), cfg.eos_ids)
    pieces = GC.tiny_pieces(cfg.vocab_size)
    pieces[3 + ord('"')] = b""                                                # a vocabulary without '"'
    with pytest.raises(ValueError, match=r"state \d+ \((obj_open|key)\.2\).*allows no token"):
        GrammarState(eng, 2, G.VocabBytes.from_pieces(pieces), dfa_rows=8, pda=pda)
    # ... a longer token that spells a whole key is enough: the exact walk finds it
    J.check_vocab(pda, G.VocabBytes.from_pieces(pieces[:cfg.vocab_size - 1] + [b'"k":']), cfg.eos_ids)
    with pytest.raises(ValueError, match="allows no token"):                  # no EOS id: nothing can end
        J.check_vocab(pda, _vocab(cfg), ())
    # pushing tokens do not count (at depth 64 they die), nor does a token that pops twice (what
    # lies below the top is unknown)
    br = PC.bracket_pda()
    voc = lambda *more: G.VocabBytes.from_pieces([b""] * 3 + [b"(", b"[", b"))", b"]]", b"x", *more])  # noqa: E731
    with pytest.raises(ValueError, match="state 0 of the automaton under an object on top"):
        J.check_vocab(br, voc(), (2,))
    with pytest.raises(ValueError, match="state 0 of the automaton under an array on top"):
        J.check_vocab(br, voc(b")"), (2,))
    J.check_vocab(br, voc(b")", b"]"), (2,))
    # a two-state automaton whose second state is stuck
    with pytest.raises(ValueError, match="state 1 "):
        J.check_vocab(PC.bracket_pda(), _vocab(cfg), ())
    gs = GrammarState(eng, 2, _vocab(cfg), dfa_rows=8)
    with pytest.raises(ValueError, match="pda=BytePDA.json"):
        gs.admit(0, SamplingParams(json_object=True))
    assert not hasattr(gs, "jstate") and gs.DISTURBED == ("gstate", "gfault")
    with pytest.raises(ValueError, match="BytePDA"):
        GrammarState(eng, 2, _vocab(cfg), dfa_rows=8, pda=G.ByteDFA.from_regex("a"))


# ------------------------------------------------------------------------------ end to end, CPU engine
def _check_output(pda, vocab, out, eos=2, max_ws=2):
    """Every step's token is allowed; ended by EOS the text satisfies the oracle, else its prefix is alive."""
    c = (0, 0, 0)
    for i, t in enumerate(out):
        if t == eos:
            assert pda.accepting(c) and i == len(out) - 1, out
            assert PC.ok(vocab.decode(out[:i]), max_ws), vocab.decode(out[:i])
            return True
        c = pda.walk(vocab.token(t), c) if vocab.token(t) else None
        assert c is not None, (out, i)
    return False


def eager_run(eng, sp, prompt, n_new, slot=1, gs=None):
    """One request on EagerSamplingDecode until EOS or n_new tokens -> (tokens, GrammarState)."""
    from llm_sharding_amd.runtime.sampling import ConstraintState
    gs = GrammarState(eng, eng.max_slots, _vocab(eng.cfg), dfa_rows=64, pda=J.BytePDA.json()) if gs is None else gs
    cs = ConstraintState(eng, eng.max_slots, state_rows=2) if sp.constrained else None
    eng.reset()
    gs.admit(slot, sp)
    if cs is not None:
        cs.admit(slot, sp, len(prompt))
    sl, pos = eng.prefill_rows([slot], [len(prompt)])
    h = eng.forward(eng.embed(torch.tensor(prompt)), sl, pos)
    eng.advance([slot], [len(prompt)])
    first = Sampler(eng, None, cs, gs).sample(h, [len(prompt) - 1], [sp], [len(prompt)], slots=[slot])
    g = EagerSamplingDecode(eng, 1, "full", slots=[slot], history_len=n_new, constraints=cs, grammar=gs)
    g.set_params(0, sp)
    g.tokens.copy_(first.to(torch.int32))
    out = [int(first[0])]
    while len(out) < n_new and out[-1] not in eng.cfg.eos_ids:
        g.replay()
        out.append(int(g.tokens[0]))
    return out, gs


def test_eager_generation_is_json():
    cfg = tiny(layers=2)
    eng, vocab, pda = _engine(cfg), _vocab(cfg), J.BytePDA.json()
    runs = [SamplingParams(1.0, seed=s, json_object=True) for s in (1, 2, 3, 4)]
    runs.append(SamplingParams(0.0, seed=1, json_object=True))
    # the closing brace and EOS favoured, so that some runs end inside the budget
    runs += [SamplingParams(1.0, seed=s, json_object=True, logit_bias={2: 6.0, 3 + ord("}"): 6.0, 3 + ord('"'): 3.0}, min_p=0.01)
             for s in (5, 6, 7)]
    finished = 0
    for sp in runs:
        out, gs = eager_run(eng, sp, _prompt(cfg), 40)
        finished += _check_output(pda, vocab, out)
        assert int(gs.gfault.sum()) == 0
        assert eager_run(eng, sp, _prompt(cfg), 40)[0] == out                 # deterministic under its seed
    assert finished >= 2
    gs.release(1)
    assert int(gs.jstate[1]) == -1


def test_the_checker_fails_without_the_advance_step(monkeypatch):
    """Negative control: a reference that never advances the configuration keeps every row at the
    start, and the outputs stop being JSON prefixes."""
    ref = J.pda_mask_reference
    monkeypatch.setattr(J, "pda_mask_reference", lambda lg, V, tb, slot, tokens_in: ref(lg, V, tb, slot, None))
    cfg = tiny(layers=2)
    eng, vocab, pda = _engine(cfg), _vocab(cfg), J.BytePDA.json()
    out, _ = eager_run(eng, SamplingParams(1.0, seed=1, json_object=True), _prompt(cfg), 12)
    with pytest.raises(AssertionError):
        _check_output(pda, vocab, out)


def _server(cfg, **kw):
    st = plan_stages(cfg, 1).stages[0]
    return PipelineServer(cfg, RandomSource(cfg, SEED), 0, 1, st.start, st.end, device="cpu", batch=3,
                          microbatches=1, max_seq=128, prefill_budget=32, dtype=torch.float32, **kw)


def test_server_serves_json_beside_a_regex_and_a_plain_request():
    cfg = tiny(layers=2)
    vocab, pda = _vocab(cfg), J.BytePDA.json()
    prompts = [_prompt(cfg, n, seed=n) for n in (7, 12, 5)]
    js = SamplingParams(1.0, seed=6, json_object=True, logit_bias={2: 6.0, 3 + ord("}"): 6.0, 3 + ord('"'): 3.0})
    rx = SamplingParams(1.5, seed=3, regex=r"-?[0-9]{1,3}(\.[0-9]{2})?")
    plain = SamplingParams(0.8, seed=77)
    srv = _server(cfg, vocab_bytes=vocab, dfa_rows=64)
    assert srv.grammar is None
    rids = [srv.submit(prompts[0], 40, sampling=js), srv.submit(prompts[1], 12, sampling=rx),
            srv.submit(prompts[2], 12, eos_ids=(), sampling=plain)]
    srv.serve(stop_when_idle=True)
    outs = [srv.requests[r].output_ids for r in rids]
    assert srv.grammar is not None and srv.grammar.pda == pda and int(srv.grammar.gfault.sum()) == 0
    assert (srv.grammar.jstate == -1).all() and (srv.grammar.gstate == -1).all()
    _check_output(pda, vocab, outs[0])
    assert outs[0] == eager_run(_engine(cfg), js, prompts[0], 40)[0]         # the eager twin gives the same tokens
    assert G.ByteDFA.from_regex(rx.regex).walk(vocab.decode(outs[1])) >= 0
    # the neighbours get what they get in a server that never sees the JSON request
    bare = _server(cfg, vocab_bytes=vocab, dfa_rows=64)
    b = [bare.submit(prompts[1], 12, sampling=rx), bare.submit(prompts[2], 12, eos_ids=(), sampling=plain)]
    bare.serve(stop_when_idle=True)
    assert [bare.requests[r].output_ids for r in b] == outs[1:]
    # a server that sees neither builds no stage
    none = _server(cfg, vocab_bytes=vocab)
    none.submit(prompts[2], 4, eos_ids=(), sampling=plain)
    none.serve(stop_when_idle=True)
    assert none.grammar is None and none._json is None


def test_server_refuses_what_cannot_be_served():
    cfg = tiny(layers=2)
    js = SamplingParams(json_object=True)
    with pytest.raises(ValueError, match="vocab_bytes"):
        _server(cfg).submit([5, 6], 4, sampling=js)
    pieces = GC.tiny_pieces(cfg.vocab_size)
    pieces[3 + ord('"')] = b""
    srv = _server(cfg, vocab_bytes=G.VocabBytes.from_pieces(pieces))
    with pytest.raises(ValueError, match="allows no token"):
        srv.submit([5, 6], 4, sampling=js)
    rid = srv.submit([5, 6], 6, sampling=SamplingParams(1.0, seed=1, regex="[ab]{1,3}"))   # a regex is still served
    srv.serve(stop_when_idle=True)
    assert srv.grammar is not None and srv.grammar.pda is None and len(srv.requests[rid].output_ids) >= 1
    import dataclasses
    no_eos = dataclasses.replace(cfg, eos_token_id=None)
    with pytest.raises(ValueError, match="EOS"):
        _server(no_eos, vocab_bytes=_vocab(cfg)).submit([5, 6], 4, sampling=js)
    with pytest.raises(ValueError, match="json_max_ws"):
        _server(cfg, json_max_ws=9)
    wide = _server(cfg, vocab_bytes=_vocab(cfg), json_max_ws=0)
    rid = wide.submit([5, 6], 30, sampling=SamplingParams(1.0, seed=2, json_object=True))
    wide.serve(stop_when_idle=True)
    out = wide.requests[rid].output_ids
    assert wide.grammar.pda == J.BytePDA.json(max_ws=0)
    _check_output(wide.grammar.pda, _vocab(cfg), out, max_ws=0)
    # speculation refuses it, as it refuses a regex
    from llm_sharding_amd.runtime.speculative import EagerSpecDecode
    g = EagerSpecDecode(_engine(cfg), 1, 2, sampling=True, history_len=8, eos_ids=cfg.eos_ids)
    with pytest.raises(ValueError, match="json_object"):
        g.admit(0, [5], 4, SamplingParams(0.5, seed=1, json_object=True), n_prompt=1)
    # user_request messages take the two keys
    from llm_sharding_amd.parallel.ingress import submit_message

    class Rep:
        errors = []

        def error(self, to, why):
            self.errors.append(why)

        def __call__(self, *a):
            pass

    assert submit_message(wide, {"input_ids": [5, 6], "json_object": True, "regex": "a", "max_new_tokens": 4}, None, 4, Rep()) == 0
    assert submit_message(wide, {"input_ids": [5, 6], "json_object": True, "temperature": 1.0, "seed": 3,
                                 "max_new_tokens": 8}, None, 4, Rep()) == 1
    assert submit_message(wide, {"input_ids": [5, 6], "response_format": {"type": "json_object"}, "max_new_tokens": 8},
                          None, 4, Rep()) == 1
    assert len(Rep.errors) == 1 and "json_object" in Rep.errors[0]
    wide.serve(stop_when_idle=True)
    for r in wide.finished[-2:]:
        assert r.sampling.json_object
        _check_output(wide.grammar.pda, _vocab(cfg), r.output_ids, max_ws=0)


def test_inference_cli_json_flag(capsys):
    import inference
    out = inference.main(["--random", "tiny", "--json", "--temperature", "1", "--seed", "3", "--max-new-tokens", "24"])
    text = capsys.readouterr().out
    assert "pushdown automaton of 65 states" in text
    assert ("parses as a JSON object" in text) == (out[-1] == 2) and "DOES NOT PARSE" not in text
    assert ("live prefix" in text) == (out[-1] != 2)
    body = bytes(t - 3 for t in out if t != 2)
    assert J.BytePDA.json().alive(body)
    for extra in (["--speculative", "2"], ["--score"], ["--hf-compare", "x"], ["--regex", "a+"], ["--min-tokens", "2"]):
        with pytest.raises(SystemExit):
            inference.main(["--random", "tiny", "--json", *extra])
