"""Constrained decoding on the device (csrc/sampling/logit_process.hip): the kernel against the
numpy reference, bitwise on the logits, ``astate`` and ``fault``, on the shared cases
(tests/constraint_cases.py) and on the edges (every bias slot, a 32767-state automaton, the min-p
extremes); the captured SamplingDecodeGraph with a ConstraintState replay by replay; and captured
generation with ``choices`` on the tiny engine and the graph-mode server."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import constraint_cases as C
from llm_sharding_amd.config import tiny
from llm_sharding_amd.ops import constraints as K
from llm_sharding_amd.runtime.engine import RandomSource, StageEngine
from llm_sharding_amd.runtime.sampling import ConstraintState, Sampler, SamplingDecodeGraph, SamplingParams

pytestmark = pytest.mark.gpu
DEV = "cuda"
NINF = float("-inf")


def _bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _dev_tables(tb) -> SimpleNamespace:
    return SimpleNamespace(**{k: torch.from_numpy(np.ascontiguousarray(getattr(tb, k))).to(DEV) for k in K.TABLES})


def _launch(logits, V, tb, slot, tokens, ctr, ctr_add=0, reread=False):
    """lsa_logit_process on numpy inputs -> (logits uint16, astate, fault, arena) after the launch."""
    lg = C.to_bf16(logits).to(DEV)
    assert lg.dim() == 1 or lg.stride(0) == logits.shape[-1]
    lg = lg[None] if lg.dim() == 1 else lg
    d = _dev_tables(tb)
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)  # noqa: E731
    K.logit_process(lg, V, lg.shape[0], i32(slot), None if tokens is None else i32(tokens), i32(ctr), d, ctr_add,
                    reread=reread)
    torch.cuda.synchronize()
    return _bits(lg), d.astate.cpu().numpy(), d.fault.cpu().numpy(), d.arena.cpu().numpy()


def _same(got, want, what):
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    assert bad.size == 0, f"{len(bad)} {what} differ, first {bad[:4].tolist()}"


# ------------------------------------------------------------------------------ kernel vs reference
@pytest.mark.parametrize("case", C.KERNEL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_kernel_matches_reference_bitwise(case):
    c = C.make_case(*case)
    want_l, want_a, want_f = C.reference(*case)
    got_l, got_a, got_f, arena = _launch(c.logits, c.V, c.tables, c.slot, c.tokens, c.ctr, c.ctr_add)
    _same(got_l[:, :c.V], want_l[:, :c.V], "logits")
    _same(got_a, want_a, "automaton states")
    _same(got_f, want_f, "fault flags")
    assert (got_l[:, c.V:] == C.LOGIT_PAD).all() and (arena == c.tables.arena).all()
    off = [r for r, m in enumerate(c.modes) if m in ("off", "eos_off")]
    assert (got_l[off] == c.logits[off]).all()
    if c.rows >= len(C.MODES):
        assert set(c.modes) == set(C.MODES) and want_f.sum() >= 1 and (want_a != c.tables.astate).sum() >= 2
    # a second launch from the same snapshot is bitwise equal
    l2, a2, f2, _ = _launch(c.logits, c.V, c.tables, c.slot, c.tokens, c.ctr, c.ctr_add)
    assert (l2 == got_l).all() and (a2 == got_a).all() and (f2 == got_f).all()


@pytest.mark.parametrize("case", C.KERNEL_CASES[1:3], ids=lambda c: "x".join(map(str, c)))
def test_min_p_by_rereading_the_row_gives_the_same_bits(case):
    """Rows of up to 32768 aligned columns keep the row in registers for min-p; the path longer
    rows take (store, then re-read) must agree on them."""
    c = C.make_case(*case)
    want_l, want_a, want_f = C.reference(*case)
    got_l, got_a, got_f, _ = _launch(c.logits, c.V, c.tables, c.slot, c.tokens, c.ctr, c.ctr_add, reread=True)
    _same(got_l, want_l, "logits")
    assert (got_a == want_a).all() and (got_f == want_f).all()
    assert sum("minp" in m for m in c.modes) >= 5


def test_a_row_alone_equals_the_row_in_the_batch():
    case = C.KERNEL_CASES[2]
    c = C.make_case(*case)
    assert c.rows == 129
    want_l, want_a, want_f = C.reference(*case)
    for r in (1, 4, 9, 10, 47, 128):
        got_l, got_a, got_f, _ = _launch(c.logits[r:r + 1], c.V, c.tables, c.slot[r:r + 1], c.tokens[r:r + 1],
                                         c.ctr[r:r + 1], c.ctr_add)
        s = int(c.slot[r])
        assert (got_l[0] == want_l[r]).all(), f"row {r} ({c.modes[r]}) alone differs from the row in the batch"
        assert got_a[s] == want_a[s] and got_f[s] == want_f[s]
        others = np.setdiff1d(np.arange(got_a.size), [s])
        assert (got_a[others] == c.tables.astate[others]).all() and (got_f[others] == 0).all()


def test_no_input_tokens_and_slots_outside_the_table():
    case = C.KERNEL_CASES[1]
    c = C.make_case(*case)
    want = K.logit_process_reference(c.logits, c.V, c.tables, c.slot, None, c.ctr, c.ctr_add)
    got_l, got_a, got_f, _ = _launch(c.logits, c.V, c.tables, c.slot, None, c.ctr, c.ctr_add)
    _same(got_l, want[0], "logits")
    assert (got_a == c.tables.astate).all() and (got_f == 0).all()      # null tokens_in: nothing advances
    slot = c.slot.copy()
    slot[[1, 3]] = [c.tables.astate.size, -1]                            # outside the tables: the row is skipped
    want = K.logit_process_reference(c.logits, c.V, c.tables, slot, c.tokens, c.ctr, c.ctr_add)
    got_l, got_a, got_f, _ = _launch(c.logits, c.V, c.tables, slot, c.tokens, c.ctr, c.ctr_add)
    _same(got_l, want[0], "logits")
    _same(got_a, want[1], "automaton states")
    assert (got_l[[1, 3]] == c.logits[[1, 3]]).all()


def test_every_bias_slot_and_the_edges_of_the_row():
    V, ld = 1003, 1008
    rng = np.random.default_rng(2)
    logits = np.full((2, ld), C.LOGIT_PAD, dtype=np.uint16)
    logits[:, :V] = C.bf16_bits(4.0 * rng.standard_normal((2, V)))
    tb = C.empty_tables(3, 1, ld, eos=(2,))
    toks = np.concatenate([[0, V - 1, 1000, 1001, 4], 5 + rng.permutation(900)[:K.BIAS_MAX - 5]])   # distinct
    vals = (3.0 * rng.standard_normal(K.BIAS_MAX)).astype(np.float32)
    vals[[1, 3, 100]] = NINF
    C.set_bias(tb, 2, toks, vals)
    C.set_bias(tb, 0, [1002], [0.5])
    want = K.logit_process_reference(logits, V, tb, [2, 0], None, [7, 7])
    got_l, _, _, _ = _launch(logits, V, tb, [2, 0], None, [7, 7])
    _same(got_l, want[0], "logits")
    ch = np.nonzero(got_l[0] != logits[0])[0]
    assert set(ch) <= set(toks.tolist()) and len(ch) > 300 and {0, V - 1, 1001} <= set(ch.tolist())
    assert got_l[0, V - 1] == K.NEG_INF_BITS and np.nonzero(got_l[1] != logits[1])[0].tolist() == [1002]


def test_min_until_boundary_and_min_p_extremes():
    V, ld = 1003, 1008
    rng = np.random.default_rng(3)
    rows = 5
    logits = np.full((rows, ld), C.LOGIT_PAD, dtype=np.uint16)
    logits[:, :V] = C.bf16_bits(4.0 * rng.standard_normal((rows, V)))
    logits[3, [17, 1002]] = C.bf16_bits([30.0])[0]
    tb = C.empty_tables(rows, 1, ld, eos=(2, V - 1, 1001))
    tb.min_until[[0, 1]] = 50                     # row 0: c = 49, masked; row 1: c = 50, free
    tb.minp_delta[[2, 3, 4]] = [NINF, 0.0, -1e-6]
    ctr = np.array([48, 49, 48, 48, 48], dtype=np.int32)
    want = K.logit_process_reference(logits, V, tb, np.arange(rows), None, ctr, 1)
    got_l, _, _, _ = _launch(logits, V, tb, np.arange(rows), None, ctr, 1)
    _same(got_l, want[0], "logits")
    assert np.nonzero(got_l[0] != logits[0])[0].tolist() == [2, 1001, V - 1]
    assert (got_l[[1, 2]] == logits[[1, 2]]).all()
    keep = got_l[:, :V] != K.NEG_INF_BITS
    assert np.nonzero(keep[3])[0].tolist() == [17, 1002]
    x = K.bf16_bits_to_f32(logits[4, :V])
    assert (keep[4] == (x == x.max())).all() and (got_l[:, V:] == C.LOGIT_PAD).all()


def test_a_32767_state_automaton():
    V, S, base = 64, K.MAX_STATES, 2
    chain = C.chain_automaton(S, V)
    tb = C.empty_tables(2, base + S + 1, V)
    tb.arena[base:base + S] = chain
    tb.abase[:] = base
    tb.astate[:] = [base + S - 2, base + 40000 % S]
    tok = np.array([(S - 2) % V, (40000 % S) % V + 1], dtype=np.int32)     # the allowed one, a forbidden one
    logits = C.bf16_bits(np.random.default_rng(4).standard_normal((2, V)))
    want = K.logit_process_reference(logits, V, tb, [0, 1], tok, [3, 3])
    got_l, got_a, got_f, _ = _launch(logits, V, tb, [0, 1], tok, [3, 3])
    _same(got_l, want[0], "logits")
    assert got_a.tolist() == want[1].tolist() == [base + S - 1, base + 40000 % S]
    assert got_f.tolist() == want[2].tolist() == [0, 1]
    assert np.nonzero(got_l[0] != K.NEG_INF_BITS)[0].tolist() == [0]        # relative state 32766 loops on token 0


def test_argument_checks():
    c = C.make_case(*C.KERNEL_CASES[1])
    lg, d = C.to_bf16(c.logits).to(DEV), _dev_tables(c.tables)
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)  # noqa: E731
    slot, tok, ctr = i32(c.slot), i32(c.tokens), i32(c.ctr)
    with pytest.raises(ValueError):
        K.logit_process(lg, 2000, c.rows, slot, tok, ctr, d)                # V beyond the row
    with pytest.raises(ValueError):
        K.logit_process(lg, c.V, c.rows + 1, slot, tok, ctr, d)             # more rows than logits
    with pytest.raises(ValueError):
        K.logit_process(lg, c.V, 0, slot, tok, ctr, d)
    short = SimpleNamespace(**{**vars(d), "arena": d.arena[:, :1000]})
    with pytest.raises(ValueError):
        K.logit_process(lg, c.V, c.rows, slot, tok, ctr, short)             # an arena row shorter than V
    with pytest.raises(ValueError):
        K.logit_process(lg, c.V, c.rows, slot, tok, ctr, SimpleNamespace(**{**vars(d), "fault": None}))
    with pytest.raises(ValueError):
        K.logit_process(lg, c.V, c.rows, slot.long(), tok, ctr, d)
    assert (_bits(lg) == c.logits).all()


# ------------------------------------------------------------------------------ graph
SLOTS = [4, 1, 3, 0]
CHOICES = [[10, 11, 12], [10, 11], [40], [41, 42, 43, 44], [300, 7]]
PARAMS = [SamplingParams(0.0, seed=1, choices=CHOICES),
          SamplingParams(0.9, seed=77, logit_bias={5: 2.5, 511: -3.0}, banned_token_ids=[9], min_p=0.05, min_tokens=3),
          SamplingParams(0.0, seed=2),
          SamplingParams(1.2, top_k=50, seed=14, allowed_token_ids=[5, 17, 99, 300, 511], min_p=0.3)]


def _tiny_engine(cfg, slots=6):
    return StageEngine(cfg, 0, cfg.num_hidden_layers, DEV, torch.bfloat16, has_embed=True, has_head=True,
                       source=RandomSource(cfg, 0), max_slots=slots, max_seq=128, max_prefill_rows=64)


def _prefill(eng, slots, prompts):
    eng.reset()
    sl, po = eng.prefill_rows(slots, [len(p) for p in prompts])
    h = eng.forward(eng.embed(torch.tensor([t for p in prompts for t in p], device=DEV)), sl, po)
    eng.advance(slots, [len(p) for p in prompts])
    return h, [int(i) for i in np.cumsum([len(p) for p in prompts]) - 1]


def test_sampling_decode_graph_with_constraints():
    cfg = tiny(layers=2)
    V, eng = cfg.vocab_size, _tiny_engine(cfg)
    g0 = torch.Generator().manual_seed(3)
    prompts = [torch.randint(3, V, (n,), generator=g0).tolist() for n in (5, 9, 3, 7)]
    h, last = _prefill(eng, SLOTS, prompts)
    cs = ConstraintState(eng, 6, state_rows=16)
    for s, p, sp in zip(SLOTS, prompts, PARAMS):
        cs.admit(s, sp, len(p))
    assert cs.astate.cpu().tolist()[2] == -1 and cs.alloc.rows_free() == 16 - 12 - 1
    first = Sampler(eng, None, cs).sample(h, last, PARAMS, [len(p) for p in prompts], slots=SLOTS)
    assert int(first[0]) in (10, 40, 41, 300) and int(first[3]) in (5, 17, 99, 300, 511)
    calls0 = K.logit_process_calls()
    g = SamplingDecodeGraph(eng, 4, "full", slots=SLOTS, history_len=3, constraints=cs, debug_raw=True)
    for i, sp in enumerate(PARAMS):
        g.set_params(i, sp)
    g.tokens.copy_(first.to(torch.int32))
    a0 = cs.astate.cpu().numpy().copy()
    g.capture()
    assert K.logit_process_calls() == calls0 + 2                  # the warm-up run and the capture
    assert (cs.astate.cpu().numpy() == a0).all() and int(cs.fault.sum()) == 0   # the warm-up's advance is undone
    pos0 = g.pos.cpu().tolist()
    for step in range(3):
        t_in, pos = g.tokens.cpu().tolist(), g.pos.cpu().tolist()
        snap = SimpleNamespace(**{k: getattr(cs, k).cpu().numpy().copy() for k in K.TABLES})
        g.replay()
        torch.cuda.synchronize()
        want_l, want_a, want_f = K.logit_process_reference(g.raw_logits.cpu(), V, snap, SLOTS, t_in, pos, 1)
        assert torch.equal(g.logits.cpu().view(torch.int16)[:, :V], want_l.view(torch.int16)[:, :V]), f"replay {step}"
        assert torch.equal(g.logits[:, V:], g.raw_logits[:, V:])
        assert (cs.astate.cpu().numpy() == want_a).all() and (cs.fault.cpu().numpy() == want_f).all()
        # the eager kernel path on the same inputs gives the same row, state and flags
        d = _dev_tables(snap)
        lg = g.raw_logits.clone()
        K.logit_process(lg, V, 4, g.slot, torch.tensor(t_in, dtype=torch.int32, device=DEV),
                        torch.tensor(pos, dtype=torch.int32, device=DEV), d, ctr_add=1)
        assert torch.equal(lg.view(torch.int16), g.logits.view(torch.int16))
        assert torch.equal(d.astate, cs.astate) and torch.equal(d.fault, cs.fault)
        assert torch.equal(g.logits[2], g.raw_logits[2])          # the unconstrained row
        # exactly one advance of row 0's automaton per replay, by the token that was fed
        rel = int(snap.arena[snap.astate[4], t_in[0]])
        assert rel >= 0 and int(cs.astate[4]) == int(snap.abase[4]) + rel
        tok = g.tokens.cpu().tolist()
        assert np.isfinite(g.logits.float().cpu().numpy()[np.arange(4), tok]).all()      # never a masked token
        assert tok[3] in (5, 17, 99, 300, 511) and tok[1] != 9
        assert g.pos.cpu().tolist() == [p + step + 1 for p in pos0]
    # a graph built without constraints launches no such kernel and touches no table
    calls1, a1 = K.logit_process_calls(), cs.astate.clone()
    g2 = SamplingDecodeGraph(eng, 4, "full", slots=SLOTS)
    g2.set_params(1, SamplingParams(0.8, seed=77))
    g2.capture()
    g2.replay()
    torch.cuda.synchronize()
    assert K.logit_process_calls() == calls1 and torch.equal(cs.astate, a1) and g2.constraints is None
    with pytest.raises(RuntimeError, match="ConstraintState"):
        g2.set_params(0, PARAMS[0])


def test_captured_generation_with_choices():
    cfg = tiny(layers=2)
    V, eng = cfg.vocab_size, _tiny_engine(cfg)
    runs = [SamplingParams(0.0, seed=1, choices=CHOICES)] + [SamplingParams(1.5, seed=s, choices=CHOICES) for s in (3, 4, 5)]
    g0 = torch.Generator().manual_seed(8)
    prompts = [torch.randint(3, V, (n,), generator=g0).tolist() for n in (6, 4, 9, 5)]
    h, last = _prefill(eng, SLOTS, prompts)
    cs = ConstraintState(eng, 6, state_rows=16)
    for s, p, sp in zip(SLOTS, prompts, runs):
        cs.admit(s, sp, len(p))
    assert cs.alloc.rows_free() == 4                              # four requests share one automaton of 12 states
    first = Sampler(eng, None, cs).sample(h, last, runs, [len(p) for p in prompts], slots=SLOTS)
    g = SamplingDecodeGraph(eng, 4, "full", slots=SLOTS, history_len=6, constraints=cs)
    for i, sp in enumerate(runs):
        g.set_params(i, sp)
    g.tokens.copy_(first.to(torch.int32))
    g.capture()
    for _ in range(6):
        g.replay()
    torch.cuda.synchronize()
    hist = g.history.cpu().numpy()
    for i in range(4):
        out = [int(first[i])] + hist[:, i].tolist()
        n = out.index(2)
        assert out[:n] in CHOICES and all(t == 2 for t in out[n:]), out   # a choice, then EOS for ever
    assert int(cs.fault.sum()) == 0


def test_server_with_choices_in_graph_mode():
    from llm_sharding_amd.parallel.server import PipelineServer
    cfg = tiny(layers=2)
    srv = PipelineServer(cfg, RandomSource(cfg, 11), 0, 1, 0, cfg.num_hidden_layers, device=DEV, batch=2,
                         microbatches=2, max_seq=128, prefill_budget=16)
    assert srv.graph_mode and srv.constraints is None
    g0 = torch.Generator().manual_seed(5)
    prompts = [torch.randint(3, cfg.vocab_size, (n,), generator=g0).tolist() for n in (7, 12, 5, 9, 6)]
    params = [SamplingParams(0.0, seed=1, choices=CHOICES), SamplingParams(1.5, seed=3, choices=CHOICES), None,
              SamplingParams(1.5, seed=4, choices=CHOICES), SamplingParams(0.7, seed=5, min_tokens=6, min_p=0.1)]
    rids = [srv.submit(p, 10, sampling=sp) for p, sp in zip(prompts, params)]
    srv.serve(stop_when_idle=True)
    outs = [srv.requests[r].output_ids for r in rids]
    for i in (0, 1, 3):
        assert outs[i][-1] == 2 and outs[i][:-1] in CHOICES, outs[i]
    assert 2 not in outs[4][:6]
    assert all(isinstance(g, SamplingDecodeGraph) and g.constraints is srv.constraints for g in srv.graphs)
    assert int(srv.constraints.fault.sum()) == 0 and srv._arena.rows_free() == srv.state_rows
    assert (srv.constraints.astate == -1).all()
    # the plain greedy neighbour got what it gets in a server that never saw a constraint
    bare = PipelineServer(cfg, RandomSource(cfg, 11), 0, 1, 0, cfg.num_hidden_layers, device=DEV, batch=2,
                          microbatches=2, max_seq=128, prefill_budget=16)
    rb = [bare.submit(prompts[2], 10, sampling=None), bare.submit(prompts[0], 10, sampling=SamplingParams(0.8, seed=1))]
    bare.serve(stop_when_idle=True)
    assert bare.constraints is None and all(g.constraints is None for g in bare.graphs)
    assert bare.requests[rb[0]].output_ids == outs[2]
