"""The logit stages together, CPU side: an ``EagerSamplingDecode`` with all three states and
log-probabilities against the ``ops`` references chained by hand in the written order (this file
shares no code with ``runtime.logit_stages``' order), the ordered helper over every subset, and a
one-stage ``PipelineServer`` that meets the features one request after the other, drains, re-shards
and serves again."""
import itertools
from types import SimpleNamespace

import numpy as np
import torch

import grammar_cases as GC
from llm_sharding_amd.config import tiny
from llm_sharding_amd.ops import constraints as K
from llm_sharding_amd.ops import grammar as G
from llm_sharding_amd.ops import logprobs as LP
from llm_sharding_amd.ops import penalties as P
from llm_sharding_amd.ops import sampling as S
from llm_sharding_amd.parallel.scheduler import plan_stages
from llm_sharding_amd.parallel.server import PipelineServer
from llm_sharding_amd.runtime import logit_stages as LS
from llm_sharding_amd.runtime.engine import RandomSource, StageEngine
from llm_sharding_amd.runtime.sampling import (ConstraintState, EagerSamplingDecode, GrammarState, PenaltyState,
                                               Sampler, SamplingParams)

SEED = 0            # the weights (the GPU twin uses the same)
SLOTS = [4, 1, 3, 0]
STEPS = 4
LP_ATOL = 1e-4      # the project's bound on a log-probability (csrc/sampling/logprobs.hip, Accuracy)
NUMBER, LETTERS = r"-?[0-9]{1,3}(\.[0-9]{2})?", r"[a-c]{2,5}x"


def rows(V: int) -> list:
    """One row per combination: penalty + regex + min_p + logprobs, choices + penalty, a finite bias +
    regex + logprobs=3, and a plain sampled row. The tiny model's logits span about [-1, 1], so min_p =
    0.7 at temperature 1 (a window of 0.36 under the maximum) is what makes the maximum matter."""
    return [SamplingParams(1.0, seed=5, repetition_penalty=1.3, frequency_penalty=0.25, regex=NUMBER, min_p=0.7,
                           logprobs=2),
            SamplingParams(0.9, seed=6, presence_penalty=0.5, choices=[[40, 41, 42, 43, 44, 45, 46], [40, 50, 51, 52]]),
            SamplingParams(1.2, seed=7, logit_bias={3 + ord("b"): 2.0, 3 + ord("x"): -1.5}, regex=LETTERS, logprobs=3),
            SamplingParams(0.8, seed=8, top_k=40)]


def prompts(V: int) -> list:
    g = torch.Generator().manual_seed(3)
    return [torch.randint(3, V, (n,), generator=g).tolist() for n in (5, 9, 3, 7)]


def vocab_of(cfg):
    return G.VocabBytes.from_pieces(GC.tiny_pieces(cfg.vocab_size))


def make_states(eng, cfg, params, proms, slots=SLOTS):
    """The three states over six slots with the four requests admitted."""
    pen, cs = PenaltyState(eng, 6), ConstraintState(eng, 6, state_rows=16)
    gs = GrammarState(eng, 6, vocab_of(cfg), dfa_rows=32)
    for s, sp, p in zip(slots, params, proms):
        if sp.penalized:
            pen.admit(s, p)
        cs.admit(s, sp, len(p))
        gs.admit(s, sp)
    return pen, cs, gs


def snapshot(pen, cs, gs) -> SimpleNamespace:
    """Host copies of every table of the three states."""
    cp = lambda t: t.detach().cpu().numpy().copy()  # noqa: E731
    return SimpleNamespace(state=cp(pen.state).view(np.uint16),
                           con=SimpleNamespace(**{k: cp(getattr(cs, k)) for k in K.TABLES}),
                           gram=SimpleNamespace(**{k: cp(getattr(gs, k)) for k in G.TABLES}))


def hand_chain(raw, V, snap, slots, t_in, ctr, params, swap=False) -> SimpleNamespace:
    """One step by the references, in the written order: penalise -> grammar mask -> process ->
    sample -> logprobs, from the bf16 logits ``raw``, the tables ``snap`` held before the step, the
    step's input tokens and the positions ``ctr`` the sampled tokens will occupy. ``swap``: mask and
    process change places (the wrong order)."""
    raw = raw.detach().cpu()
    f = lambda k: [getattr(p, k) for p in params]  # noqa: E731
    l1, state = P.penalize_reference(raw, V, snap.state, slots, t_in, f("repetition_penalty"), f("presence_penalty"),
                                     f("frequency_penalty"))
    if swap:  # only the processed rows: a row may have lost every column
        l2 = K.logit_process_reference(l1, V, snap.con, slots, t_in, ctr)[0]
        return SimpleNamespace(logits=G.grammar_mask_reference(l2, V, snap.gram, slots, t_in)[0])
    l2, gstate, gfault = G.grammar_mask_reference(l1, V, snap.gram, slots, t_in)
    l3, astate, fault = K.logit_process_reference(l2, V, snap.con, slots, t_in, ctr)
    tok = S.sample_reference(l3, V, f("temperature"), f("top_k"), f("top_p"), f("seed"), ctr)[0]
    lp = LP.logprobs_reference(l3, V, f("n_top"), tok)
    return SimpleNamespace(logits=l3, state=state, gstate=gstate, gfault=gfault, astate=astate, fault=fault,
                           tokens=np.asarray(tok), lp=lp)


def bits(t: torch.Tensor, V: int) -> np.ndarray:
    return t.detach().cpu().contiguous().view(torch.int16).numpy()[:, :V]


def check_tables(want, pen, cs, gs, what) -> None:
    cp = lambda t: t.detach().cpu().numpy()  # noqa: E731
    assert (cp(pen.state).view(np.uint16) == want.state).all(), what
    for k, t in (("astate", cs.astate), ("fault", cs.fault), ("gstate", gs.gstate), ("gfault", gs.gfault)):
        assert (cp(t) == getattr(want, k)).all(), (what, k)


def check_logprobs(want, lp, params, what) -> None:
    """``tok_lp`` within the project's 1e-4, ranks and the ids of the alternatives exactly."""
    asked = [i for i, p in enumerate(params) if p.logprobs is not None]
    got = [t.detach().cpu().numpy() for t in (lp.tok_lp, lp.tok_rank, lp.top_id, lp.top_lp)]
    np.testing.assert_allclose(got[0][asked], want.lp.tok_lp[asked], rtol=0, atol=LP_ATOL, err_msg=what)
    assert (got[1][asked] == want.lp.tok_rank[asked]).all(), what
    for i in asked:
        n = params[i].logprobs
        assert (got[2][i, :n] == want.lp.top_id[i, :n]).all(), what
        np.testing.assert_allclose(got[3][i, :n], want.lp.top_lp[i, :n], rtol=0, atol=LP_ATOL, err_msg=what)


def _engine(cfg, slots=6):
    return StageEngine(cfg, 0, cfg.num_hidden_layers, "cpu", torch.float32, has_embed=True, has_head=True,
                       source=RandomSource(cfg, SEED), max_slots=slots, max_seq=128)


def test_the_ordered_helper_over_every_subset():
    assert LS.STAGE_ORDER == ("penalties", "grammar", "constraints")
    assert [c.name for c in LS.STAGE_CLASSES] == list(LS.STAGE_ORDER)
    for on in itertools.product((False, True), repeat=3):
        given = {k: SimpleNamespace(name=k) if o else None for k, o in zip(("penalties", "constraints", "grammar"), on)}
        got = LS.ordered_stages(**given)
        assert [st.name for st in got] == [k for k in LS.STAGE_ORDER if given[k] is not None]
        assert all(st is given[st.name] for st in got)


def test_eager_decode_with_all_three_stages_equals_the_hand_chain():
    cfg = tiny(layers=2)
    V, eng = cfg.vocab_size, _engine(cfg)
    params, proms = rows(V), prompts(V)
    pen, cs, gs = make_states(eng, cfg, params, proms)
    eng.reset()
    sl, po = eng.prefill_rows(SLOTS, [len(p) for p in proms])
    h = eng.forward(eng.embed(torch.tensor([t for p in proms for t in p])), sl, po)
    eng.advance(SLOTS, [len(p) for p in proms])
    last = [int(i) for i in np.cumsum([len(p) for p in proms]) - 1]
    smp = Sampler(eng, pen, cs, gs)
    # the first token: the same chain without input tokens
    snap, ctr = snapshot(pen, cs, gs), [len(p) for p in proms]
    first, lp0 = smp.sample(h, last, params, ctr, slots=SLOTS, return_logprobs=True)
    want = hand_chain(smp.logits(h, last), V, snap, SLOTS, None, ctr, params)
    assert first.tolist() == want.tokens.tolist()
    check_tables(want, pen, cs, gs, "first token")
    check_logprobs(want, lp0, params, "first token")

    g = EagerSamplingDecode(eng, 4, "full", slots=SLOTS, history_len=STEPS, penalties=pen, constraints=cs, grammar=gs,
                            logprobs=True)
    for i, sp in enumerate(params):
        g.set_params(i, sp)
    g.tokens.copy_(first.to(torch.int32))
    seen, logits_of = [], g.sampler.logits
    g.sampler.logits = lambda h, rows_idx=None: seen.append(logits_of(h, rows_idx)) or seen[-1]
    order_matters = 0
    for step in range(STEPS):
        snap, t_in = snapshot(pen, cs, gs), g.tokens.tolist()
        ctr = [int(eng.seq_len[s]) + 1 for s in SLOTS]
        g.replay()
        assert len(seen) == step + 1
        want = hand_chain(seen[-1], V, snap, SLOTS, t_in, ctr, params)
        assert g.tokens.tolist() == want.tokens.tolist(), f"step {step}"
        check_tables(want, pen, cs, gs, f"step {step}")
        check_logprobs(want, g.lp, params, f"step {step}")
        assert g.history[step].tolist() == want.tokens.tolist()
        np.testing.assert_allclose(g.lp_history[step, [0, 2]].numpy(), want.lp.tok_lp[[0, 2]], rtol=0, atol=LP_ATOL)
        wrong = hand_chain(seen[-1], V, snap, SLOTS, t_in, ctr, params, swap=True)
        order_matters += int((bits(wrong.logits, V) != bits(want.logits, V)).any())
    # the precondition: min-p saw an unmasked maximum at least once, so the order was exercised
    assert order_matters >= 1
    for s, sp in zip(SLOTS, params):                       # the penalty counts: what was fed, per slot
        fed = [int(first[SLOTS.index(s)])] + g.history[:STEPS - 1, SLOTS.index(s)].tolist()
        want_counts = np.bincount(fed, minlength=V) if sp.penalized else np.zeros(V, dtype=np.int64)
        assert (pen.counts(s).numpy() == want_counts).all()


def _server(cfg, **kw):
    st = plan_stages(cfg, 1).stages[0]
    return PipelineServer(cfg, RandomSource(cfg, SEED), 0, 1, st.start, st.end, device="cpu", batch=2, microbatches=2,
                          max_seq=128, prefill_budget=16, dtype=torch.float32, vocab_bytes=vocab_of(cfg), dfa_rows=64,
                          state_rows=32, **kw)


def _result(srv, rid):
    r = srv.requests[rid]
    return r.output_ids, r.token_logprobs, r.ranks, r.top_logprobs


def test_a_server_meets_the_features_one_by_one_then_reshards():
    cfg = tiny(layers=2)
    V, NEW = cfg.vocab_size, 8
    g = torch.Generator().manual_seed(9)
    proms = [torch.randint(3, V, (n,), generator=g).tolist() for n in (7, 12, 5, 9, 6)]
    params = [SamplingParams(0.8, seed=77),
              SamplingParams(0.7, seed=3, repetition_penalty=1.4, frequency_penalty=0.3),
              SamplingParams(1.5, seed=4, regex=NUMBER),
              SamplingParams(0.9, seed=5, choices=[[40, 41, 42, 43, 44, 45], [40, 50, 51, 52, 53]]),
              SamplingParams(1.1, seed=6, logprobs=3)]
    srv = _server(cfg)
    assert (srv.penalties, srv.constraints, srv.grammar, srv.sampler) == (None, None, None, None)
    rids, overlap = [], []

    def submit_next(r, tok):  # the next request arrives while this one is still decoding
        if len(r.output_ids) == 2 and len(rids) < len(params) and r.rid == rids[-1]:
            overlap.append(r.state)
            rids.append(srv.submit(proms[len(rids)], NEW, eos_ids=(), sampling=params[len(rids)], on_token=submit_next))

    rids.append(srv.submit(proms[0], NEW, eos_ids=(), sampling=params[0], on_token=submit_next))
    srv.serve(stop_when_idle=True)
    assert len(rids) == 5 and overlap == ["decoding"] * 4
    assert srv.sampling_on and srv.logprobs_on and None not in (srv.penalties, srv.constraints, srv.grammar)
    assert (srv.sampler.penalties, srv.sampler.constraints, srv.sampler.grammar) == (srv.penalties, srv.constraints,
                                                                                    srv.grammar)
    got = [_result(srv, r) for r in rids]
    assert all(len(o[0]) == NEW for o in got) and got[4][1] is not None and got[0][1] is None
    for p, sp, o in zip(proms, params, got):               # each equals a fresh server that serves it alone
        solo = _server(cfg)
        rid = solo.submit(p, NEW, eos_ids=(), sampling=sp)
        solo.serve(stop_when_idle=True)
        assert _result(solo, rid) == o
    # drained: every row of both arenas is free again and no slot holds anything
    assert srv._arena.rows_free() == srv.state_rows and srv._garena.rows_free() == 64
    assert not srv.constraints.held and not srv.grammar.held
    assert (srv.constraints.astate == -1).all() and (srv.grammar.gstate == -1).all()
    # re-shard to the same layers: every state is rebuilt on the new engine, and serves the same
    old = (srv.eng, srv.penalties, srv.constraints, srv.grammar, srv.sampler)
    srv._reshard(srv.start, srv.end)
    assert all(new is not o for new, o in zip((srv.eng, srv.penalties, srv.constraints, srv.grammar, srv.sampler), old))
    assert all(st.eng is srv.eng for st in (srv.penalties, srv.constraints, srv.grammar, srv.sampler))
    again = [srv.submit(proms[i], NEW, eos_ids=(), sampling=params[i]) for i in (2, 3)]
    srv.serve(stop_when_idle=True)
    assert [_result(srv, r) for r in again] == [got[2], got[3]]
    assert srv._arena.rows_free() == srv.state_rows and srv._garena.rows_free() == 64
