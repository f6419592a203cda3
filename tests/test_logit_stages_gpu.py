"""The logit stages together in a captured step: a ``SamplingDecodeGraph`` with all three states
and log-probabilities against the ``ops`` references chained by hand (``test_logit_stages``'
``hand_chain``), what ``capture()`` launches and restores, and a graph built without the stages.
The vocabulary is the tiny configuration's; the kernels' own edge shapes have their own files."""
import numpy as np
import pytest
import torch

import test_logit_stages as T
from llm_sharding_amd.config import tiny
from llm_sharding_amd.ops import constraints as K
from llm_sharding_amd.ops import grammar as G
from llm_sharding_amd.ops import penalties as P
from llm_sharding_amd.runtime.engine import RandomSource, StageEngine
from llm_sharding_amd.runtime.sampling import Sampler, SamplingDecodeGraph, SamplingParams

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SLOTS, STEPS = T.SLOTS, T.STEPS


def _calls() -> tuple:
    return P.penalize_calls(), G.grammar_mask_calls(), K.logit_process_calls()


def _all_tables(pen, cs, gs) -> list:
    return ([pen.state.clone()] + [getattr(cs, k).clone() for k in K.TABLES]
            + [getattr(gs, k).clone() for k in G.TABLES])


def test_a_captured_step_with_all_three_stages_equals_the_hand_chain():
    cfg = tiny(layers=2)
    V = cfg.vocab_size
    eng = StageEngine(cfg, 0, cfg.num_hidden_layers, DEV, torch.bfloat16, has_embed=True, has_head=True,
                      source=RandomSource(cfg, T.SEED), max_slots=6, max_seq=128, max_prefill_rows=64)
    params, proms = T.rows(V), T.prompts(V)
    pen, cs, gs = T.make_states(eng, cfg, params, proms)
    eng.reset()
    sl, po = eng.prefill_rows(SLOTS, [len(p) for p in proms])
    h = eng.forward(eng.embed(torch.tensor([t for p in proms for t in p], device=DEV)), sl, po)
    eng.advance(SLOTS, [len(p) for p in proms])
    last = [sum(len(p) for p in proms[:i + 1]) - 1 for i in range(4)]
    first = Sampler(eng, pen, cs, gs).sample(h, last, params, [len(p) for p in proms], slots=SLOTS)

    calls0 = _calls()
    g = SamplingDecodeGraph(eng, 4, "full", slots=SLOTS, history_len=STEPS, penalties=pen, constraints=cs, grammar=gs,
                            logprobs=True, debug_raw=True)
    for i, sp in enumerate(params):
        g.set_params(i, sp)
    g.tokens.copy_(first.to(torch.int32))
    idx = torch.tensor(SLOTS, device=DEV)
    kept = [t[idx].clone() for t in (pen.state, cs.astate, cs.fault, gs.gstate, gs.gfault)]
    g.capture()
    torch.cuda.synchronize()
    assert _calls() == tuple(c + 2 for c in calls0)             # each stage: the warm-up run and the capture
    for t, k in zip((pen.state, cs.astate, cs.fault, gs.gstate, gs.gfault), kept):
        assert torch.equal(t[idx], k)                           # what the warm-up advanced is back

    order_matters = 0
    for step in range(STEPS):
        snap, t_in = T.snapshot(pen, cs, gs), g.tokens.cpu().tolist()
        ctr = (g.pos.cpu() + 1).tolist()
        g.replay()
        torch.cuda.synchronize()
        want = T.hand_chain(g.raw_logits, V, snap, SLOTS, t_in, ctr, params)
        assert (T.bits(g.logits, V) == T.bits(want.logits, V)).all(), f"replay {step}"
        assert torch.equal(g.logits[:, V:], g.raw_logits[:, V:])                    # columns >= V are untouched
        T.check_tables(want, pen, cs, gs, f"replay {step}")
        after = T.snapshot(pen, cs, gs)                         # every table a step does not write: as it was
        for now, before, written in ((after.con, snap.con, ("astate", "fault")),
                                     (after.gram, snap.gram, ("gstate", "gfault"))):
            for k, v in vars(before).items():
                assert k in written or np.array_equal(getattr(now, k), v), k
        assert g.tokens.cpu().tolist() == want.tokens.tolist(), f"replay {step}"
        T.check_logprobs(want, g.lp, params, f"replay {step}")
        wrong = T.hand_chain(g.raw_logits, V, snap, SLOTS, t_in, ctr, params, swap=True)
        order_matters += int((T.bits(wrong.logits, V) != T.bits(want.logits, V)).any())
    assert order_matters >= 1                                   # min-p saw an unmasked maximum: the order counted
    assert g.history.cpu()[STEPS - 1].tolist() == g.tokens.cpu().tolist()

    # a second graph over the same slots, built with none of the three: no such launch, no table touched
    calls1, tables1 = _calls(), _all_tables(pen, cs, gs)
    g2 = SamplingDecodeGraph(eng, 4, "full", slots=SLOTS)
    g2.set_params(3, SamplingParams(0.8, seed=8, top_k=40))
    g2.capture()
    g2.replay()
    torch.cuda.synchronize()
    assert _calls() == calls1 and (g2.penalties, g2.constraints, g2.grammar) == (None, None, None)
    for a, b in zip(_all_tables(pen, cs, gs), tables1):
        assert torch.equal(a, b)
