"""Constrained decoding, CPU side: the numpy reference against transformers' MinPLogitsWarper,
SequenceBiasLogitsProcessor and MinNewTokensLengthLogitsProcessor, the automaton builders, every
validation error, the arena allocator, and the CPU engine end to end (EagerSamplingDecode and a
one-stage PipelineServer) with choices, allowed_token_ids and min_tokens."""
import itertools

import numpy as np
import pytest
import torch

import constraint_cases as C
from llm_sharding_amd.config import tiny
from llm_sharding_amd.ops import constraints as K
from llm_sharding_amd.parallel.scheduler import plan_stages
from llm_sharding_amd.parallel.server import PipelineServer
from llm_sharding_amd.runtime.engine import RandomSource, StageEngine
from llm_sharding_amd.runtime.sampling import (ConstraintState, EagerSamplingDecode, Sampler, SamplingParams,
                                               compile_constraints)

NINF = float("-inf")
SEED = 11


def _tables(V, n_slots=4, eos=()):
    tb = C.empty_tables(n_slots, 1, V, eos)
    return tb


def _kept(bits):
    return np.asarray(bits) != K.NEG_INF_BITS


# ------------------------------------------------------------------------------ reference vs HF
MINP_CASES = list(itertools.product((0.5, 1.0, 1.7), (0.05, 0.3, 1.0)))


def _gapped_logits(rng, rows, V, T, min_p):
    """bf16 logits with no value closer than 0.05 to the fp64 threshold l_max + T ln(min_p): such
    a value is moved 0.25 below it and rounded to bf16 again (the maximum itself stays), so the
    fp32 probability rule and the log-space rule cannot disagree."""
    x = C.bf16_bits(3.0 * rng.standard_normal((rows, V)))
    f = K.bf16_bits_to_f32(x).astype(np.float64)
    for r in range(rows):
        thr = f[r].max() + T * np.log(min_p)
        near = (np.abs(f[r] - thr) < 0.05) & (f[r] != f[r].max())
        f[r, near] = thr - 0.25
    x = C.bf16_bits(f.astype(np.float32))
    f = K.bf16_bits_to_f32(x).astype(np.float64)
    for r in range(rows):
        thr = f[r].max() + T * np.log(min_p)
        assert (np.abs(f[r][f[r] != f[r].max()] - thr) >= 0.05).all()
    return x


@pytest.mark.parametrize("T,min_p", MINP_CASES)
def test_min_p_keeps_what_hf_keeps(T, min_p):
    from transformers import MinPLogitsWarper
    rows, V = 4, 777
    rng = np.random.default_rng(int(100 * T + 1000 * min_p))
    bits = _gapped_logits(rng, rows, V, T, min_p)
    sp = SamplingParams(T, seed=1, min_p=min_p)
    tb = _tables(V, rows)
    tb.minp_delta[:] = compile_constraints(sp, V, [2]).minp_delta
    got, _, _ = K.logit_process_reference(bits, V, tb, list(range(rows)), None, [9] * rows)
    scores = torch.from_numpy(K.bf16_bits_to_f32(bits)) / T          # HF warps the temperature-scaled scores
    hf = MinPLogitsWarper(min_p=min_p)(None, scores.clone())
    hf_kept = torch.isfinite(hf).numpy()
    assert (_kept(got) == hf_kept).all()
    assert hf_kept.any(axis=1).all() and (min_p == 0.05 or not hf_kept.all())
    assert (got[_kept(got)] == bits[_kept(got)]).all()               # survivors keep their bits


def test_min_p_is_ignored_at_temperature_zero():
    c = compile_constraints(SamplingParams(0.0, seed=1, min_p=0.2), 100, [2])
    assert c.minp_delta == NINF
    assert compile_constraints(SamplingParams(0.5, seed=1, min_p=1.0), 100, [2]).minp_delta == 0.0
    assert compile_constraints(SamplingParams(2.0, seed=1, min_p=0.1), 100, [2]).minp_delta == float(
        np.float32(2.0 * np.log(0.1)))


def test_finite_bias_equals_hf_bitwise():
    from transformers import SequenceBiasLogitsProcessor
    rows, V = 3, 203
    rng = np.random.default_rng(5)
    sc = C.to_bf16(C.bf16_bits(3.0 * rng.standard_normal((rows, V))))
    bias = {0: 1.5, V - 1: -2.25, 200: 0.375, 77: 100.0, 13: -0.0078125}    # bf16-exact values
    hf = SequenceBiasLogitsProcessor(sequence_bias={(t,): b for t, b in bias.items()})(
        torch.zeros((rows, 4), dtype=torch.long), sc.clone())
    tb = _tables(V, rows)
    c = compile_constraints(SamplingParams(0.0, seed=1, logit_bias=bias), V, [2])
    for s in range(rows):
        C.set_bias(tb, s, c.bias_tok, c.bias_val)
    got, _, _ = K.logit_process_reference(sc, V, tb, list(range(rows)), None, [4] * rows)
    assert got.dtype == torch.bfloat16 and hf.dtype == torch.bfloat16
    assert torch.equal(got.view(torch.int16), hf.view(torch.int16))
    changed = (got.view(torch.int16) != sc.view(torch.int16)).any(dim=0).nonzero().flatten().tolist()
    assert set(changed) <= set(bias) and len(changed) >= 4


@pytest.mark.parametrize("n_new", [0, 3, 7, 8, 9])
def test_min_tokens_equals_hf(n_new):
    from transformers import MinNewTokensLengthLogitsProcessor
    V, prompt_len, min_tokens, eos = 97, 6, 8, [2, 96]
    rng = np.random.default_rng(n_new)
    sc = C.to_bf16(C.bf16_bits(3.0 * rng.standard_normal((2, V))))
    ids = torch.zeros((2, prompt_len + n_new), dtype=torch.long)
    hf = MinNewTokensLengthLogitsProcessor(prompt_len, min_tokens, eos)(ids, sc.clone())
    tb = _tables(V, 2, eos)
    tb.min_until[:] = prompt_len + min_tokens
    got, _, _ = K.logit_process_reference(sc, V, tb, [0, 1], None, [prompt_len + n_new] * 2)
    assert torch.equal(got.view(torch.int16), hf.view(torch.int16))
    assert bool(torch.isinf(got[:, eos]).all()) == (n_new < min_tokens)


def test_skipped_rows_and_foreign_slots_are_untouched():
    case = C.KERNEL_CASES[1]
    c = C.make_case(*case)
    lg, ast, flt = C.reference(*case)
    off = [r for r, m in enumerate(c.modes) if m in ("off", "eos_off")]
    assert len(off) >= 2 and (lg[off] == c.logits[off]).all()
    assert (lg[:, c.V:] == C.LOGIT_PAD).all()
    out = np.setdiff1d(np.arange(c.tables.astate.size), c.slot)
    assert (ast[out] == c.tables.astate[out]).all() and (flt[out] == 0).all()
    for r, m in enumerate(c.modes):
        s = int(c.slot[r])
        if m == "auto_fault":
            assert flt[s] == 1 and ast[s] == c.tables.astate[s]
        elif "auto" in m and c.tokens[r] >= 0:
            rel = int(c.tables.arena[c.tables.astate[s], c.tokens[r]])
            assert flt[s] == 0 and ast[s] == c.tables.abase[s] + rel
        if m not in ("off", "eos_off"):
            assert (lg[r, :c.V] != c.logits[r, :c.V]).any(), m
        if m == "minp_max_only":
            x = K.bf16_bits_to_f32(c.logits[r, :c.V])
            assert (_kept(lg[r, :c.V]) == (x == x.max())).all()           # the maximum (and its ties) alone
        if m == "minp_zero":
            assert sorted(np.nonzero(_kept(lg[r, :c.V]))[0]) == [5, c.V - 2]
    assert set(c.modes) == set(C.MODES)


# ------------------------------------------------------------------------------ automata
def test_from_choices_accepts_exactly_the_choices():
    V, eos = 7, [2, 6]
    choices = [[3, 4], [3], [5, 3, 4], [3, 4], [4]]
    a = K.TokenAutomaton.from_choices(choices, V, eos)
    end = a.n_states - 1
    assert (np.nonzero(a.next[end] >= 0)[0] == eos).all() and (a.next[end, eos] == end).all()
    for c in choices:
        for e in eos:
            assert a.walk(c + [e]) == end and a.walk(c + [e, e]) == end
    assert a.walk([3]) >= 0 and a.walk([3, 4]) >= 0              # a prefix choice may continue or end
    want = {tuple(c) for c in choices}
    alphabet = [t for t in range(V) if t not in eos]
    for n in range(0, 4):
        for seq in itertools.product(alphabet, repeat=n):
            for e in eos:
                assert (a.walk(list(seq) + [e]) == end) == (seq in want), seq
    assert a.walk([3, 4, 3]) == -1 and a.walk([2]) == -1
    assert a == K.TokenAutomaton.from_choices([[4], [5, 3, 4], [3], [3, 4]], V, eos)  # order, duplicates
    assert a.digest != K.TokenAutomaton.from_choices([[4], [5, 3, 4], [3]], V, eos).digest
    for bad in ([], [[]], [[3], []], [[7]], [[-1]], [[3, 2]]):
        with pytest.raises(ValueError):
            K.TokenAutomaton.from_choices(bad, V, eos)
    with pytest.raises(ValueError, match="EOS"):
        K.TokenAutomaton.from_choices([[3]], V, [])


def test_automaton_tables():
    a = K.TokenAutomaton.from_allowed([5, 1, 5], 8)
    assert a.n_states == 1 and np.nonzero(a.next[0] >= 0)[0].tolist() == [1, 5] and a.walk([1, 5, 5]) == 0
    assert a.walk([2]) == -1
    t = np.array([[1, -1], [-1, 0]])
    assert K.TokenAutomaton.from_table(t) == K.TokenAutomaton(t.astype(np.int16)) and a.next.dtype == np.int16
    for bad in (np.array([[1, -1], [-1, -1]]),        # a state without a token
                np.array([[2, -1], [-1, 0]]),         # a state that does not exist
                np.array([[-2, 0]]), np.zeros((0, 4), dtype=np.int16), np.zeros(4, dtype=np.int16),
                np.zeros((2, 2), dtype=np.float32), np.zeros((K.MAX_STATES + 1, 1), dtype=np.int16)):
        with pytest.raises(ValueError):
            K.TokenAutomaton(bad)
    with pytest.raises(ValueError):
        K.TokenAutomaton.from_allowed([8], 8)
    with pytest.raises(ValueError):
        K.TokenAutomaton.from_allowed([], 8)
    big = K.TokenAutomaton(C.chain_automaton())
    assert big.n_states == K.MAX_STATES and big.walk([i % 64 for i in range(K.MAX_STATES - 1)]) == K.MAX_STATES - 1


def test_allocator_shares_frees_and_refuses():
    al = K.ArenaAllocator(10)
    a = K.TokenAutomaton.from_choices([[3, 4]], 8, [2])           # 4 states
    b = K.TokenAutomaton.from_choices([[3, 5]], 8, [2])
    c = K.TokenAutomaton.from_allowed([1], 8)                     # 1 state
    assert a.n_states == 4 and al.acquire(a) == 0 and al.acquire(b) == 4
    assert al.acquire(K.TokenAutomaton.from_choices([[3, 4]], 8, [2])) == 0 and al.refs(a.digest) == 2
    assert al.rows_free() == 2
    big = K.TokenAutomaton.from_choices([[3, 4, 5]], 8, [2])      # 5 states
    with pytest.raises(ValueError, match="does not fit"):
        al.acquire(big)
    assert not al.release(a.digest) and al.rows_free() == 2       # still held once
    assert al.release(a.digest) and al.rows_free() == 6 and al.refs(a.digest) == 0
    with pytest.raises(ValueError, match="does not fit"):         # 6 rows free, but 4 + 2 apart
        al.acquire(big)
    assert al.acquire(c) == 0 and al.acquire(K.TokenAutomaton.from_allowed([2], 8)) == 1
    assert al.release(b.digest) and al.base(c.digest) == 0
    assert al.acquire(big) == 2 and al.rows_free() == 3           # rows 2..3 and 4..7 merged


# ------------------------------------------------------------------------------ validation
def test_sampling_params_constraint_fields():
    sp = SamplingParams(0.7, 40, 0.9, 5)
    assert not sp.constrained and SamplingParams().plain
    for kw in ({"logit_bias": {3: 1.0}}, {"banned_token_ids": [3]}, {"min_tokens": 1}, {"min_p": 0.1},
               {"allowed_token_ids": [3]}, {"choices": [[3]]}, {"automaton": K.TokenAutomaton.from_allowed([1], 8)}):
        sp = SamplingParams(seed=1, **kw)
        assert sp.constrained and not sp.plain and sp.greedy, kw
    sp = SamplingParams(seed=1, logit_bias={"7": 2, 3: NINF}, banned_token_ids=[9, 7, 9])
    assert sp.bias_entries() == [(3, NINF), (7, NINF), (9, NINF)] and sp.logit_bias == {7: 2.0, 3: NINF}
    assert SamplingParams(seed=1, logit_bias={}, banned_token_ids=[]).plain
    d = SamplingParams.from_dict({"logit_bias": {"5": -1.5}, "banned_token_ids": [1], "min_tokens": 2, "min_p": 0.5,
                                  "temperature": 0.5})
    assert (d.logit_bias, d.banned_token_ids, d.min_tokens, d.min_p) == ({5: -1.5}, [1], 2, 0.5)
    assert SamplingParams.from_dict({"choices": [[3, 4], [5]]}).choices == [[3, 4], [5]]
    assert SamplingParams.from_dict({"allowed_token_ids": [4, 3]}).allowed_token_ids == [3, 4]
    assert SamplingParams.from_dict({"max_new_tokens": 3}) is None
    auto = K.TokenAutomaton.from_allowed([1], 8)
    bad = [{"logit_bias": {3: float("nan")}}, {"logit_bias": {3: float("inf")}}, {"logit_bias": {-1: 1.0}},
           {"logit_bias": {"x": 1.0}}, {"logit_bias": [3]}, {"banned_token_ids": [-1]}, {"banned_token_ids": [1.5]},
           {"logit_bias": {i: 1.0 for i in range(200)}, "banned_token_ids": list(range(200, 321))},
           {"min_p": 0.0}, {"min_p": 1.5}, {"min_p": float("nan")}, {"min_tokens": -1}, {"min_tokens": 1.5},
           {"allowed_token_ids": []}, {"choices": []}, {"choices": [[]]}, {"choices": [3]}, {"automaton": "x"},
           {"allowed_token_ids": [1], "choices": [[1]]}, {"choices": [[1]], "automaton": auto},
           {"allowed_token_ids": [1], "automaton": auto},
           {"automaton": auto, "banned_token_ids": [1]}, {"choices": [[1]], "logit_bias": {3: NINF}},
           {"allowed_token_ids": [1], "min_tokens": 2}]
    for kw in bad:
        with pytest.raises(ValueError):
            SamplingParams(seed=1, **kw)
    SamplingParams(seed=1, logit_bias={i: 1.0 for i in range(200)}, banned_token_ids=list(range(200, 320)))
    SamplingParams(seed=1, choices=[[1]], logit_bias={3: 2.0}, min_p=0.3)     # finite bias and min-p may ride along


def test_compile_checks_against_the_configuration():
    V, eos = 16, [2]
    for kw in ({"logit_bias": {16: 1.0}}, {"banned_token_ids": [16]}, {"allowed_token_ids": [16]},
               {"choices": [[3, 16]]}, {"automaton": K.TokenAutomaton.from_allowed([1], 8)},
               {"banned_token_ids": [t for t in range(V) if t != 2], "min_tokens": 1}):
        with pytest.raises(ValueError):
            compile_constraints(SamplingParams(seed=1, **kw), V, eos)
    with pytest.raises(ValueError, match="whole vocabulary"):
        compile_constraints(SamplingParams(seed=1, banned_token_ids=list(range(V))), V, [])
    with pytest.raises(ValueError, match="EOS"):
        compile_constraints(SamplingParams(seed=1, choices=[[3]]), V, [])
    c = compile_constraints(SamplingParams(seed=1, banned_token_ids=[t for t in range(V) if t != 2]), V, eos)
    assert len(c.bias_tok) == V - 1 and c.automaton is None and c.minp_delta == NINF
    c = compile_constraints(SamplingParams(seed=1, choices=[[3, 4]]), V, eos)
    assert c.automaton == K.TokenAutomaton.from_choices([[3, 4]], V, eos)


# ------------------------------------------------------------------------------ end to end, CPU engine
CHOICES = [[10, 11, 12], [10, 11], [40], [41, 42, 43, 44], [300, 7]]
RUNS = [SamplingParams(0.0, seed=1, choices=CHOICES)] + [SamplingParams(1.5, seed=s, choices=CHOICES) for s in (3, 4, 5)]


def _engine(cfg, slots=2):
    return StageEngine(cfg, 0, cfg.num_hidden_layers, "cpu", torch.float32, has_embed=True, has_head=True,
                       source=RandomSource(cfg, SEED), max_slots=slots, max_seq=128)


def _prompt(cfg, n=7, seed=5):
    return torch.randint(3, cfg.vocab_size, (n,), generator=torch.Generator().manual_seed(seed)).tolist()


def eager_run(eng, sp, prompt, n_new, slot=1, cs=None):
    """One request on EagerSamplingDecode until EOS or n_new tokens -> (tokens, ConstraintState)."""
    cs = ConstraintState(eng, eng.max_slots, state_rows=32) if cs is None and sp.constrained else cs
    eng.reset()
    if cs is not None:
        cs.admit(slot, sp, len(prompt))
    sl, pos = eng.prefill_rows([slot], [len(prompt)])
    h = eng.forward(eng.embed(torch.tensor(prompt)), sl, pos)
    eng.advance([slot], [len(prompt)])
    kw = {} if cs is None else {"slots": [slot]}
    first = Sampler(eng, None, cs).sample(h, [len(prompt) - 1], [sp], [len(prompt)], **kw)
    g = EagerSamplingDecode(eng, 1, "full", slots=[slot], history_len=n_new, constraints=cs)
    g.set_params(0, sp)
    g.tokens.copy_(first.to(torch.int32))
    out = [int(first[0])]
    while len(out) < n_new and out[-1] not in eng.cfg.eos_ids:
        g.replay()
        out.append(int(g.tokens[0]))
    return out, cs


def _is_choice_then_eos(out, eos=2):
    return out[-1] == eos and out[:-1] in CHOICES


@pytest.mark.parametrize("sp", RUNS, ids=lambda p: f"T{p.temperature}-seed{p.seed}")
def test_eager_choices_produce_a_choice_then_eos(sp):
    cfg = tiny(layers=2)
    eng = _engine(cfg)
    out, cs = eager_run(eng, sp, _prompt(cfg), 12)
    assert _is_choice_then_eos(out), out
    assert int(cs.fault.sum()) == 0
    cs.release(1)
    assert cs.alloc.rows_free() == 32 and int(cs.astate[1]) == -1


def test_the_checker_fails_without_the_advance_step(monkeypatch):
    """Negative control: a reference that never advances the automaton keeps every row in the
    start state, and the outputs are no longer choices."""
    ref = K.logit_process_reference
    monkeypatch.setattr(K, "logit_process_reference",
                        lambda lg, V, tb, slot, tokens_in, ctr, ctr_add=0: ref(lg, V, tb, slot, None, ctr, ctr_add))
    cfg = tiny(layers=2)
    eng = _engine(cfg)
    outs = [eager_run(eng, sp, _prompt(cfg), 12)[0] for sp in RUNS]
    assert not all(_is_choice_then_eos(o) for o in outs), outs
    assert all(t in {c[0] for c in CHOICES} for o in outs for t in o)     # the start state's tokens, for ever


def _server(cfg, world=1, rank=0, batch=2, microbatches=2, **kw):
    st = plan_stages(cfg, world).stages[rank]
    return PipelineServer(cfg, RandomSource(cfg, SEED), rank, world, st.start, st.end, device="cpu", batch=batch,
                          microbatches=microbatches, max_seq=128, prefill_budget=16, dtype=torch.float32, **kw)


def test_server_choices_and_plain_neighbours():
    cfg = tiny(layers=2)
    prompts = [_prompt(cfg, n, seed=n) for n in (7, 12, 5, 9, 6)]
    plain = SamplingParams(0.8, seed=77)
    srv = _server(cfg)
    assert srv.constraints is None and srv._arena is None
    rids = [srv.submit(p, 12, sampling=sp) for p, sp in zip(prompts, RUNS)]
    rids += [srv.submit(prompts[4], 12, eos_ids=(), sampling=plain), srv.submit(prompts[3], 12, eos_ids=())]
    srv.serve(stop_when_idle=True)
    outs = [srv.requests[r].output_ids for r in rids]
    for o in outs[:4]:
        assert _is_choice_then_eos(o), o
    assert srv.constraints is not None and int(srv.constraints.fault.sum()) == 0
    assert srv._arena.rows_free() == srv.state_rows and not srv.constraints.held       # every reference returned
    assert (srv.constraints.astate == -1).all()
    # the eager twin gives the same tokens, and requests without the fields what they gave before
    eng = _engine(cfg)
    for p, sp, o in zip(prompts, RUNS, outs):
        assert eager_run(eng, sp, p, 12)[0] == o
    bare = _server(cfg)
    b = [bare.submit(prompts[4], 12, eos_ids=(), sampling=plain), bare.submit(prompts[3], 12, eos_ids=())]
    bare.serve(stop_when_idle=True)
    assert bare.constraints is None and bare._arena is None
    assert [bare.requests[r].output_ids for r in b] == outs[4:]


def test_server_refuses_what_does_not_fit_or_is_invalid():
    cfg = tiny(layers=2)
    srv = _server(cfg, state_rows=6)
    p = _prompt(cfg)
    with pytest.raises(ValueError, match="does not fit"):
        srv.submit(p, 4, sampling=SamplingParams(seed=1, choices=CHOICES))
    with pytest.raises(ValueError, match="vocabulary"):
        srv.submit(p, 4, sampling=SamplingParams(seed=1, banned_token_ids=[cfg.vocab_size]))
    rid = srv.submit(p, 6, sampling=SamplingParams(seed=1, choices=[[10, 11]]))    # 4 states fit
    srv.serve(stop_when_idle=True)
    assert srv.requests[rid].output_ids == [10, 11, 2]
    with pytest.raises(ValueError, match="single-stage"):
        _server(cfg, world=2).submit(p, 4, sampling=SamplingParams(seed=1, min_tokens=2))
    from llm_sharding_amd.runtime.speculative import EagerSpecDecode
    g = EagerSpecDecode(_engine(cfg), 1, 2, sampling=True, history_len=8, eos_ids=cfg.eos_ids)
    with pytest.raises(ValueError, match="constrained"):
        g.admit(0, [5], 4, SamplingParams(0.5, seed=1, min_p=0.2), n_prompt=1)
    g.admit(0, [5], 4, SamplingParams(0.5, seed=1), n_prompt=1)


def test_allowed_token_ids_stay_inside_the_set():
    cfg = tiny(layers=2)
    allowed = [5, 17, 99, 300, 511]
    eng = _engine(cfg)
    for sp in (SamplingParams(0.0, seed=1, allowed_token_ids=allowed), SamplingParams(1.5, seed=9, allowed_token_ids=allowed)):
        out, cs = eager_run(eng, sp, _prompt(cfg), 10)
        assert len(out) == 10 and set(out) <= set(allowed) and int(cs.fault.sum()) == 0
    assert len(set(out)) > 1
    srv = _server(cfg)
    rid = srv.submit(_prompt(cfg), 10, sampling=SamplingParams(1.5, seed=9, allowed_token_ids=allowed))
    srv.serve(stop_when_idle=True)
    assert srv.requests[rid].output_ids == out


def test_min_tokens_holds_eos_back():
    cfg = tiny(layers=2)
    eng = _engine(cfg)
    eng.head_bias = torch.zeros(cfg.head_rows)
    eng.head_bias[2] = 100.0                                       # a head that wants to end at once
    p = _prompt(cfg)
    out, _ = eager_run(eng, SamplingParams(0.7, seed=3), p, 12)
    assert out == [2]
    out, cs = eager_run(eng, SamplingParams(0.7, seed=3, min_tokens=8), p, 12)
    assert len(out) == 9 and 2 not in out[:8] and out[8] == 2
    out, _ = eager_run(eng, SamplingParams(0.0, seed=3, min_tokens=8), p, 12)
    assert len(out) == 9 and 2 not in out[:8] and out[8] == 2


def test_logprobs_describe_the_processed_row():
    cfg = tiny(layers=2)
    eng = _engine(cfg)
    sp = SamplingParams(0.0, seed=1, choices=[[10, 11]], logprobs=3)
    cs = ConstraintState(eng, 2, state_rows=8)
    cs.admit(0, sp, 7)
    p = _prompt(cfg)
    sl, pos = eng.prefill_rows([0], [7])
    h = eng.forward(eng.embed(torch.tensor(p)), sl, pos)
    tok, lp = Sampler(eng, None, cs).sample(h, [6], [sp], [7], slots=[0], return_logprobs=True)
    assert tok.tolist() == [10] and float(lp.tok_lp[0]) == 0.0 and int(lp.tok_rank[0]) == 1
    assert lp.top_id[0, :3].tolist()[0] == 10 and torch.isinf(lp.top_lp[0, 1:3]).all()
    with pytest.raises(RuntimeError, match="ConstraintState"):
        Sampler(eng).sample(h, [6], [sp], [7])


# ------------------------------------------------------------------------------ plumbing
class _FakeServer:
    def __init__(self):
        self.calls = []

    def submit(self, ids, n_new, **kw):
        self.calls.append((list(ids), n_new, kw))
        return len(self.calls) - 1


class _FakeReplies:
    def __init__(self):
        self.errors = []

    def error(self, reply_to, reason, request_id=None):
        self.errors.append(reason)


def test_submit_message_constraint_keys():
    from llm_sharding_amd.parallel.ingress import submit_message
    srv, rep = _FakeServer(), _FakeReplies()
    msg = {"input_ids": [3, 4], "logit_bias": {"5": 2.5, 9: -100}, "banned_token_ids": [7], "min_tokens": 4,
           "min_p": 0.1, "temperature": 0.9}
    assert submit_message(srv, msg, None, 8, rep) == 1
    sp = srv.calls[-1][2]["sampling"]
    assert sp.bias_entries() == [(5, 2.5), (7, NINF), (9, -100.0)] and (sp.min_tokens, sp.min_p) == (4, 0.1)
    assert submit_message(srv, {"input_ids": [3], "choices": [[4, 5], [6]]}, None, 8, rep) == 1
    assert srv.calls[-1][2]["sampling"].choices == [[4, 5], [6]]
    assert submit_message(srv, {"input_ids": [3], "allowed_token_ids": [4, 2]}, None, 8, rep) == 1
    assert submit_message(srv, {"input_ids": [3], "min_p": 2.0}, None, 8, rep) == 0
    assert rep.errors and "min_p" in rep.errors[-1]
    real = _server(tiny(layers=2), state_rows=2)
    assert submit_message(real, {"input_ids": [3], "choices": [[4, 5]]}, None, 8, rep) == 0
    assert "does not fit" in rep.errors[-1]


def test_inference_cli_constraint_flags(capsys):
    import inference
    a = inference.build_parser().parse_args(["--logit-bias", "5:1.5", "--logit-bias", "9:-inf", "--ban", "7",
                                             "--min-tokens", "3", "--min-p", "0.2", "--temperature", "0.8", "--seed", "1"])
    sp = inference.sampling_from_args(a)
    assert sp.bias_entries() == [(5, 1.5), (7, NINF), (9, NINF)] and (sp.min_tokens, sp.min_p) == (3, 0.2)
    base = ["--random", "tiny", "--device", "cpu", "--max-new-tokens", "8", "--prompt", "hello"]
    for flags in (["--min-tokens", "2"], ["--choice", "yes"], ["--ban", "7"], ["--logit-bias", "5:1"],
                  ["--min-p", "0.5", "--temperature", "0.7"]):
        for extra in (["--speculative", "2"], ["--score"], ["--hf-compare", "x"]):
            with pytest.raises(SystemExit, match="combine|greedy decode"):
                inference.main(base + flags + extra)
    with pytest.raises(SystemExit):
        inference.main(base + ["--logit-bias", "nonsense"])
    out = inference.main(base + ["--choice", "yes", "--choice", "no", "--choice", "maybe"])
    tok = inference.SyntheticByteTokenizer(512)
    want = [tok.encode(c, add_special_tokens=False) for c in ("yes", "no", "maybe")]
    assert out[-1] == 2 and out[:-1] in want
    assert "constraints:" in capsys.readouterr().out
    out = inference.main(base + ["--ban", str(out[0]), "--min-tokens", "8", "--temperature", "0.9", "--seed", "2"])
    assert len(out) == 8


# ------------------------------------------------------------------------------ threads
def _partition_ok(al) -> bool:
    """Free ranges and held ranges tile [0, state_rows) without overlap."""
    with al._lock:
        spans = sorted(list(al.free) + [(e[0], e[1].n_states) for e in al.entries.values()])
    pos = 0
    for b, n in spans:
        if b != pos or n < 1:
            return False
        pos = b + n
    return pos == al.state_rows


def test_allocator_is_safe_between_a_submitting_and_a_serving_thread():
    """One thread reserves rows (submit), another returns them (the serve loop), on the same few
    digests: the ranges always tile the arena and every reference comes back."""
    import sys
    import threading
    autos = [K.TokenAutomaton.from_choices([[3, 4 + i]], 16, [2]) for i in range(3)]      # 4 states each
    al = K.ArenaAllocator(9)                                       # two of the three fit at a time
    held, errors, n = [], [], 4000
    done = threading.Event()

    def submitter():
        try:
            for i in range(n):
                a = autos[i % 3]
                try:
                    al.acquire(a)
                    held.append(a.digest)
                except ValueError:
                    pass                                           # full: an error reply, no reference
        except Exception as e:                                     # pragma: no cover - the failure being tested
            errors.append(e)
        done.set()

    def server():
        try:
            while not done.is_set() or held:
                if held:
                    al.release(held.pop())
                    if not _partition_ok(al):
                        errors.append("ranges overlap or leak")
                        return
        except Exception as e:                                     # pragma: no cover
            errors.append(e)

    old = sys.getswitchinterval()
    sys.setswitchinterval(1e-6)
    try:
        ts = [threading.Thread(target=submitter), threading.Thread(target=server)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(60)
    finally:
        sys.setswitchinterval(old)
    assert not errors, errors[:3]
    assert not any(t.is_alive() for t in ts)
    assert al.rows_free() == 9 and not al.entries and _partition_ok(al)


def test_submitting_from_a_second_thread_while_the_server_runs():
    """The same ``choices`` over and over from an ingress thread, one request finishing as the next
    arrives: every output is a choice plus EOS and the arena ends empty."""
    import threading
    cfg = tiny(layers=2)
    srv = _server(cfg, batch=2, microbatches=1, state_rows=20)     # both tries fit: 12 + 5 states
    n, rids, errors = 24, [], []
    sent = threading.Event()

    def ingress():
        try:
            for i in range(n):
                sp = SamplingParams(1.5, seed=100 + i, choices=CHOICES if i % 3 else CHOICES[:2])
                rids.append(srv.submit(_prompt(cfg, 4 + i % 5, seed=i), 8, sampling=sp))
        except Exception as e:                                     # pragma: no cover
            errors.append(e)
        sent.set()

    t = threading.Thread(target=ingress)
    t.start()
    srv.serve(stop_when_idle=False, should_stop=sent.is_set)
    t.join(60)
    assert not errors and len(rids) == n
    for r in rids:
        assert _is_choice_then_eos(srv.requests[r].output_ids), srv.requests[r].output_ids
    assert srv._arena.rows_free() == 20 and not srv._arena.entries and not srv.constraints.held
    assert int(srv.constraints.fault.sum()) == 0 and _partition_ok(srv._arena)


def test_allocator_touches_its_tables_only_under_its_lock():
    """Deterministic twin of the thread test: every access to the digest table happens with the
    allocator's lock held (acquire, release, base and refs run on different threads in a server)."""
    al = K.ArenaAllocator(9)
    seen = []

    class Guarded(dict):
        def _chk(self):
            seen.append(al._lock.locked())

        def get(self, *a):
            self._chk()
            return dict.get(self, *a)

        def __getitem__(self, k):
            self._chk()
            return dict.__getitem__(self, k)

        def __setitem__(self, k, v):
            self._chk()
            dict.__setitem__(self, k, v)

        def __delitem__(self, k):
            self._chk()
            dict.__delitem__(self, k)

    al.entries = Guarded()
    a = K.TokenAutomaton.from_choices([[3, 4]], 16, [2])
    al.acquire(a)
    al.acquire(a)
    assert al.base(a.digest) == 0 and al.refs(a.digest) == 2
    al.release(a.digest)
    al.release(a.digest)
    assert len(seen) >= 8 and all(seen) and al.rows_free() == 9
