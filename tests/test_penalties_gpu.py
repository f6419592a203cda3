"""Repetition / presence / frequency penalties on the device (csrc/sampling/penalty.hip): the
kernel against the numpy reference, bitwise on logits[:, :V] and on the whole state table, on the
shared cases (tests/penalty_cases.py); the captured SamplingDecodeGraph with a PenaltyState
replay by replay; and the graph-mode server's neighbour independence and slot reuse."""
import numpy as np
import pytest
import torch

import penalty_cases as C
from sampling_cases import GAP_MIN
from llm_sharding_amd.config import tiny
from llm_sharding_amd.ops import penalties as P
from llm_sharding_amd.ops import sampling as S
from llm_sharding_amd.runtime.engine import RandomSource, StageEngine
from llm_sharding_amd.runtime.sampling import PenaltyState, Sampler, SamplingDecodeGraph, SamplingParams

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def _launch(c, rows=None, tokens=True):
    """lsa_penalize on (a selection of the rows of) a case, from the case's snapshot ->
    (logits uint16 [n, ld], state uint16 [n_slots, ld])."""
    sel = np.arange(c.rows) if rows is None else np.asarray(rows)
    lg = C.to_bf16(c.logits[sel]).to(DEV)
    st = C.to_i16(c.state).to(DEV)
    assert lg.stride(0) == c.ld and st.stride(0) == c.ld
    P.penalize(lg, c.V, sel.size, _i32(c.slot[sel]), _i32(c.tokens[sel]) if tokens else None, st,
               _f32(c.rep[sel]), _f32(c.pres[sel]), _f32(c.freq[sel]))
    torch.cuda.synchronize()
    return _bits(lg), _bits(st)


# ------------------------------------------------------------------------------ kernel vs reference
@pytest.mark.parametrize("case", C.KERNEL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_kernel_matches_reference_bitwise(case):
    c = C.make_case(*case)
    want_l, want_s = C.reference(*case)
    got_l, got_s = _launch(c)
    V = c.V
    bad = np.argwhere(got_l[:, :V] != want_l[:, :V])
    assert bad.size == 0, f"{len(bad)} logits differ, first (row, col) {bad[:4].tolist()}"
    bad = np.argwhere(got_s != want_s)
    assert bad.size == 0, f"{len(bad)} states differ, first (slot, col) {bad[:4].tolist()}"
    assert (got_l[:, V:] == C.LOGIT_PAD).all() and (got_s[:, V:] == C.STATE_PAD).all()
    # slots outside the launch keep their rows; all-off rows keep logits and state
    out = np.setdiff1d(np.arange(c.n_slots), c.slot)
    assert out.size and (got_s[out] == c.state[out]).all()
    off = np.nonzero((c.rep == 1) & (c.pres == 0) & (c.freq == 0))[0]
    assert (got_l[off] == c.logits[off]).all() and (got_s[c.slot[off]] == c.state[c.slot[off]]).all()
    if c.rows >= len(C.PARAM_MIX):
        assert off.size and set(c.tokens.tolist()) == set(C.token_choices(V))
    # the launch did something on every other row, and counted every input token
    on = np.setdiff1d(np.arange(c.rows), off)
    assert all((got_l[r, :V] != c.logits[r, :V]).any() for r in on)
    for r in on:
        t, s = int(c.tokens[r]), int(c.slot[r])
        if t >= 0:
            assert (got_s[s, t] & 0x7FFF) == min((c.state[s, t] & 0x7FFF) + 1, 0x7FFF)
            assert (got_s[s, t] & 0x8000) == (c.state[s, t] & 0x8000)
    # a second launch from the same snapshot is bitwise equal
    l2, s2 = _launch(c)
    assert (l2 == got_l).all() and (s2 == got_s).all()


def test_no_input_tokens():
    """tokens_in == null (the first token after a prefill): nothing is counted."""
    case = (4, 1003, 1008, 6)
    c = C.make_case(*case)
    want_l, want_s = P.penalize_reference(c.logits, c.V, c.state, c.slot, None, c.rep, c.pres, c.freq)
    got_l, got_s = _launch(c, tokens=False)
    assert (got_l == want_l).all() and (got_s == want_s).all() and (got_s == c.state).all()


def test_a_row_alone_equals_the_row_in_the_batch():
    case = C.KERNEL_CASES[3]
    c = C.make_case(*case)
    assert c.rows == 129
    want_l, want_s = C.reference(*case)
    for r in (1, 5, 47, 128):
        got_l, got_s = _launch(c, rows=[r])
        s = int(c.slot[r])
        assert (got_l[0] == want_l[r]).all(), f"row {r} alone differs from the row in the batch"
        assert (got_s[s] == want_s[s]).all()
        others = np.setdiff1d(np.arange(c.n_slots), [s])
        assert (got_s[others] == c.state[others]).all()


def test_argument_checks():
    c = C.make_case(4, 1003, 1008, 6)
    lg, st = C.to_bf16(c.logits).to(DEV), C.to_i16(c.state).to(DEV)
    args = (_i32(c.slot), _i32(c.tokens), st, _f32(c.rep), _f32(c.pres), _f32(c.freq))
    with pytest.raises(ValueError):
        P.penalize(lg, 2000, 4, *args)                                  # V beyond the row
    with pytest.raises(ValueError):
        P.penalize(lg, c.V, 5, *args)                                   # more rows than logits
    with pytest.raises(ValueError):
        P.penalize(lg, c.V, 4, args[0], args[1], st[:, :1000], *args[3:])  # a state row shorter than V
    with pytest.raises(ValueError):
        P.penalize(lg, c.V, 4, args[0].long(), *args[1:])
    # a slot outside the table skips its row instead of writing out of bounds
    slot = c.slot.copy()
    slot[0] = c.n_slots
    l0 = lg.clone()
    P.penalize(lg, c.V, 1, _i32(slot), args[1], st, _f32([1.3]), _f32([0.5]), _f32([0.2]))
    torch.cuda.synchronize()
    assert torch.equal(lg.view(torch.int16), l0.view(torch.int16)) and (_bits(st) == c.state).all()


# ------------------------------------------------------------------------------ graph
SLOTS = [4, 1, 3, 0]
PARAMS = [SamplingParams(0.0, seed=1, repetition_penalty=1.3),
          SamplingParams(0.8, seed=77, presence_penalty=0.5, frequency_penalty=0.3),
          SamplingParams(0.0, seed=2),
          SamplingParams(1.0, top_k=50, seed=14, repetition_penalty=0.8, presence_penalty=-0.2)]


def _tiny_engine(cfg, slots=6):
    return StageEngine(cfg, 0, cfg.num_hidden_layers, DEV, torch.bfloat16, has_embed=True, has_head=True,
                       source=RandomSource(cfg, 0), max_slots=slots, max_seq=128, max_prefill_rows=64)


def _prefill(eng, slots, prompts):
    eng.reset()
    sl, po = eng.prefill_rows(slots, [len(p) for p in prompts])
    h = eng.forward(eng.embed(torch.tensor([t for p in prompts for t in p], device=DEV)), sl, po)
    eng.advance(slots, [len(p) for p in prompts])
    return h, [int(i) for i in np.cumsum([len(p) for p in prompts]) - 1]


def test_sampling_decode_graph_with_penalties():
    cfg = tiny(layers=2)
    V, eng = cfg.vocab_size, _tiny_engine(cfg)
    g0 = torch.Generator().manual_seed(3)
    prompts = [torch.randint(3, V, (n,), generator=g0).tolist() for n in (5, 9, 3, 7)]
    h, last = _prefill(eng, SLOTS, prompts)
    pen = PenaltyState(eng, 6)
    pen.state[2].fill_(0x1234)                                   # a slot no graph row names
    for s, p, sp in zip(SLOTS, prompts, PARAMS):
        if sp.penalized:
            pen.admit(s, p)
    first = Sampler(eng, pen).sample(h, last, PARAMS, [len(p) for p in prompts], slots=SLOTS)
    calls0 = P.penalize_calls()
    g = SamplingDecodeGraph(eng, 4, "full", slots=SLOTS, history_len=6, penalties=pen, debug_raw=True)
    for i, sp in enumerate(PARAMS):
        g.set_params(i, sp)
    g.tokens.copy_(first.to(torch.int32))
    state0 = _bits(pen.state).copy()
    g.capture()
    assert P.penalize_calls() == calls0 + 2                      # the warm-up run and the capture
    assert (_bits(pen.state) == state0).all()                    # the warm-up's counts are undone
    pos0 = g.pos.cpu().tolist()
    assert pos0 == [len(p) for p in prompts]
    rep, pres, freq = ([getattr(sp, k) for sp in PARAMS]
                       for k in ("repetition_penalty", "presence_penalty", "frequency_penalty"))
    n_cmp = 0
    for step in range(6):
        t_in, prev = g.tokens.cpu().tolist(), _bits(pen.state).copy()
        g.replay()
        torch.cuda.synchronize()
        want_l, want_s = P.penalize_reference(g.raw_logits.cpu(), V, prev, SLOTS, t_in, rep, pres, freq)
        assert torch.equal(g.logits.cpu().view(torch.int16)[:, :V], want_l.view(torch.int16)[:, :V]), f"replay {step}"
        assert torch.equal(g.logits[:, V:], g.raw_logits[:, V:])
        assert (_bits(pen.state) == want_s).all(), f"replay {step}: state"
        assert torch.equal(g.logits[2], g.raw_logits[2])         # the unpenalised row
        ctr = [p + step + 1 for p in pos0]
        ref_tok, kept, gap, _ = S.sample_reference(g.logits.cpu(), V, [p.temperature for p in PARAMS],
                                                   [p.top_k for p in PARAMS], [p.top_p for p in PARAMS],
                                                   [p.seed for p in PARAMS], ctr)
        tok = g.tokens.cpu().numpy().astype(np.int64)
        assert (tok == g.history[step].cpu().numpy()).all() and kept[np.arange(4), tok].all()
        must = (gap >= GAP_MIN) | np.array([p.greedy for p in PARAMS])
        assert (tok[must] == ref_tok[must]).all(), f"replay {step}: graph {tok} reference {ref_tok}"
        n_cmp += int(must.sum())
    assert n_cmp >= 20
    assert (_bits(pen.state[2]) == 0x1234).all()
    cnt = pen.counts(SLOTS[1]).numpy()                           # the six input tokens of row 1
    want = np.bincount([int(first[1])] + g.history[:5, 1].cpu().tolist(), minlength=V)
    assert (cnt == want).all()
    # a graph built without penalties launches no penalty kernel and touches no state
    calls1, st1 = P.penalize_calls(), _bits(pen.state).copy()
    g2 = SamplingDecodeGraph(eng, 4, "full", slots=SLOTS)
    g2.set_params(1, SamplingParams(0.8, seed=77))
    g2.capture()
    g2.replay()
    torch.cuda.synchronize()
    assert P.penalize_calls() == calls1 and (_bits(pen.state) == st1).all() and g2.penalties is None
    assert not hasattr(g2, "rep")
    with pytest.raises(RuntimeError, match="PenaltyState"):
        g2.set_params(0, PARAMS[0])


def test_a_large_presence_penalty_never_repeats_a_token():
    cfg = tiny(layers=2)
    V, eng = cfg.vocab_size, _tiny_engine(cfg, slots=2)
    prompt = torch.randint(3, V, (6,), generator=torch.Generator().manual_seed(9)).tolist()
    sp = SamplingParams(0.0, seed=1, presence_penalty=1e4)
    h, last = _prefill(eng, [1], [prompt])
    pen = PenaltyState(eng, 2)
    pen.admit(1, prompt)
    first = Sampler(eng, pen).sample(h, last, [sp], [len(prompt)], slots=[1])
    g = SamplingDecodeGraph(eng, 1, "full", slots=[1], history_len=23, penalties=pen)
    g.set_params(0, sp)
    g.tokens.copy_(first.to(torch.int32))
    g.capture()
    for _ in range(23):
        g.replay()
    torch.cuda.synchronize()
    toks = [int(first[0])] + g.history[:, 0].cpu().tolist()
    assert len(toks) == 24 and len(set(toks)) == 24 and max(toks) < V
    # the same run with the penalty the other way round repeats its first token for ever
    sp = SamplingParams(0.0, seed=1, presence_penalty=-1e4)
    h, last = _prefill(eng, [1], [prompt])
    pen.admit(1, prompt)
    g.set_params(0, sp)
    g.set_positions()
    g.tokens.copy_(first.to(torch.int32))
    for _ in range(4):
        g.replay()
    torch.cuda.synchronize()
    assert g.tokens.cpu().tolist() == [int(first[0])]


# ------------------------------------------------------------------------------ server
REP = SamplingParams(0.0, seed=1, repetition_penalty=1.3)
PF = SamplingParams(0.8, seed=77, presence_penalty=0.5, frequency_penalty=0.3)


def _run(cfg, prompts, params, new=8, batch=2, microbatches=2):
    from llm_sharding_amd.parallel.server import PipelineServer
    srv = PipelineServer(cfg, RandomSource(cfg, 11), 0, 1, 0, cfg.num_hidden_layers, device=DEV, batch=batch,
                         microbatches=microbatches, max_seq=128, prefill_budget=16)
    assert srv.graph_mode and srv.penalties is None
    rids = [srv.submit(p, new, eos_ids=(), sampling=sp) for p, sp in zip(prompts, params)]
    srv.serve(stop_when_idle=True)
    return srv, [srv.requests[r].output_ids for r in rids]


def _prompts(cfg, lens):
    g = torch.Generator().manual_seed(5)
    return [torch.randint(3, cfg.vocab_size, (n,), generator=g).tolist() for n in lens]


def test_server_neighbours_and_slot_reuse():
    cfg = tiny(layers=2)
    prompts = _prompts(cfg, (7, 12, 5, 9))
    plain = SamplingParams(0.8, seed=77)
    # a plain greedy request next to penalised ones: the tokens it gets in a sampling server
    srv, out = _run(cfg, prompts[:3], [REP, PF, None])
    assert srv.sampling_on and srv.penalties is not None
    assert all(isinstance(g, SamplingDecodeGraph) and g.penalties is srv.penalties for g in srv.graphs)
    s2, bare = _run(cfg, prompts[:3], [None, plain, None])
    assert s2.sampling_on and s2.penalties is None and all(g.penalties is None for g in s2.graphs)
    assert out[2] == bare[2]
    assert all(len(o) == 8 and max(o) < cfg.vocab_size for o in out)
    cnt = srv.penalties.counts(0).numpy()                        # slot 0 held request 0: its fed tokens, at least
    fed = np.bincount(out[0][:-1], minlength=cfg.vocab_size)
    assert (cnt >= fed).all() and (cnt[out[0][:-1]] > 0).all()
    # the penalty acts: -1e4 on presence makes the first generated token win every later step
    _, stuck = _run(cfg, prompts[:1], [SamplingParams(0.0, seed=1, presence_penalty=-1e4)], new=6)
    assert stuck[0] == [stuck[0][0]] * 6
    # slot reuse: one slot, every request enters the slot a penalised request has just left
    dirty = [SamplingParams(0.9, seed=20 + i, repetition_penalty=1.5, frequency_penalty=0.4) for i in range(2)]
    _, many = _run(cfg, [prompts[3], prompts[0], prompts[1], prompts[0], prompts[2]], dirty + [PF, REP, None],
                   batch=1, microbatches=1)
    _, f_pf = _run(cfg, [prompts[1]], [PF], batch=1, microbatches=1)
    _, f_rep = _run(cfg, [prompts[0]], [REP], batch=1, microbatches=1)
    _, f_none = _run(cfg, [prompts[3], prompts[2]], [dirty[0], None], batch=1, microbatches=1)
    assert many[2] == f_pf[0] and many[3] == f_rep[0]
    assert many[4] == f_none[1]                                  # an unpenalised request after penalised ones
