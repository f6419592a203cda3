"""JSON mode on the device (csrc/sampling/pda_mask.hip): a stage step - lsa_grammar_mask, then
lsa_pda_mask - against the numpy references, bitwise on the logits, ``gstate``, ``jstate``,
``jdepth``, ``jstack`` and ``gfault``, on the shared cases (tests/pda_cases.py: an unaligned row, one
mode per row over a permuted slot table that also holds regex rows, automata on both sides of the LDS
threshold, the Llama-3 vocabulary size with 300-byte tokens); the captured SamplingDecodeGraph with
JSON rows and regex rows replay by replay; and captured generation on the tiny engine."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import grammar_cases as GC
import pda_cases as PC
from llm_sharding_amd.config import tiny
from llm_sharding_amd.ops import grammar as G
from llm_sharding_amd.ops import pda as J
from llm_sharding_amd.runtime.engine import RandomSource, StageEngine
from llm_sharding_amd.runtime.sampling import GrammarState, Sampler, SamplingDecodeGraph, SamplingParams

pytestmark = pytest.mark.gpu
DEV = "cuda"
READ_ONLY = ("arena", "accept", "offsets", "data", "gbase", "eos", "ptab", "paccept")


def _bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _dev_tables(tb) -> SimpleNamespace:
    return SimpleNamespace(**{k: torch.from_numpy(np.ascontiguousarray(getattr(tb, k))).to(DEV) for k in PC.ALL_TABLES})


def _launch(logits, V, tb, slot, tokens, shift=0, regex=True):
    """A stage step on numpy inputs -> (logits uint16, gstate, jstate, jdepth, jstack, gfault) after
    the launches; the read-only tables and the memory around the rows must come back unchanged.
    ``shift``: the row base sits that many elements behind a 16-byte boundary."""
    rows, ld = logits.shape
    buf = torch.zeros(rows * ld + 8 + shift, dtype=torch.int16, device=DEV)
    off = (-buf.data_ptr() // 2) % 8 + shift
    lg = buf[off:off + rows * ld].view(rows, ld)
    lg.copy_(torch.from_numpy(logits.view(np.int16)).to(DEV))
    lg = lg.view(torch.bfloat16)
    assert (lg.data_ptr() % 16) // 2 == shift % 8
    d = _dev_tables(tb)
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)  # noqa: E731
    sl, tk = i32(slot), None if tokens is None else i32(tokens)
    if regex:
        G.grammar_mask(lg, V, rows, sl, tk, d)
    J.pda_mask(lg, V, rows, sl, tk, d)
    torch.cuda.synchronize()
    for k in READ_ONLY:
        assert (getattr(d, k).cpu().numpy() == getattr(tb, k)).all(), f"{k} was written"
    assert int(buf[:off].abs().sum()) == 0 and int(buf[off + rows * ld:].abs().sum()) == 0
    return (_bits(lg),) + tuple(getattr(d, k).cpu().numpy() for k in PC.STATE_WORDS)


def _same(got, want, what):
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    assert bad.size == 0, f"{len(bad)} {what} differ, first {bad[:4].tolist()}"


def _check(c, want, tokens="own", shift=0):
    tok = c.tokens if isinstance(tokens, str) else tokens
    got = _launch(c.logits, c.V, c.tables, c.slot, tok, shift)
    _same(got[0][:, :c.V], want[0][:, :c.V], "logits")
    for g, w, k in zip(got[1:], want[1:], PC.STATE_WORDS):
        _same(g, w, k)
    assert (got[0][:, c.V:] == GC.LOGIT_PAD).all()
    again = _launch(c.logits, c.V, c.tables, c.slot, tok, shift)     # a second launch from the same snapshot
    assert all((a == b).all() for a, b in zip(got, again))
    return got


def test_binding_constants_and_refusals():
    assert J.lds_states() == 85 and J.block_threads() == 1024 and J.max_vocab() >= 128256
    assert J.lds_states() * 3 * 512 + 1024 <= 160 * 1024 and J.BytePDA.json().n_states <= J.lds_states()
    c = PC.small_case()
    d = _dev_tables(c.tables)
    lg = torch.zeros((1, c.V), dtype=torch.bfloat16, device=DEV)
    slot = torch.zeros(1, dtype=torch.int32, device=DEV)
    L = J._lib()
    from llm_sharding_amd.ops.hip import _p, _stream
    S = c.pda.n_states
    args = lambda **kw: [kw.get("logits", _p(lg)), c.V, kw.get("V", c.V), kw.get("rows", 1), _p(slot), 2, None,  # noqa: E731
                         kw.get("ptab", _p(d.ptab)), _p(d.paccept), kw.get("S", S), _p(d.offsets), _p(d.data),
                         d.data.numel(), _p(d.jstate), _p(d.jdepth), kw.get("jstack", _p(d.jstack)), _p(d.gfault),
                         _p(d.eos), _stream()]
    calls = J.pda_mask_calls()
    assert L.lsa_pda_mask(*args()) == 0 and J.pda_mask_calls() == calls + 1
    for bad in ({"logits": None}, {"ptab": None}, {"jstack": None}, {"V": 0}, {"rows": 32769}, {"rows": 0}, {"S": 0},
                {"S": 1024}, {"jstack": ctypes.c_void_p(d.jstack.data_ptr() + 4)}):
        assert L.lsa_pda_mask(*args(**bad)) == 1, bad                     # LSA_BAD_SHAPE
    assert J.pda_mask_calls() == calls + 1
    with pytest.raises(ValueError):
        J.pda_mask(lg, c.V, 1, slot, None, SimpleNamespace(**{**vars(d), "ptab": d.ptab[:2]}))
    with pytest.raises(ValueError):
        J.pda_mask(lg, c.V, 1, slot, None, SimpleNamespace(**{**vars(d), "jstack": d.jstack.to(torch.int32)}))
    torch.cuda.synchronize()


@pytest.mark.parametrize("shift", (3, 0, 7))
def test_one_unaligned_row(shift):
    c = PC.small_case()
    ln = np.diff(c.vocab.offsets)
    assert ln.min() == 0 and ln.max() == 20 and c.V % 8 != 0
    want = PC.cached_reference("small", c)
    assert want[5].sum() == 0 and want[2][1] != c.tables.jstate[1]
    got = _check(c, want, shift=shift)
    kept = (got[0][0, :c.V] != GC.NINF_BITS).sum()
    assert 10 < kept < c.V - 10


def test_one_mode_per_row_over_a_permuted_slot_table():
    c = PC.mixed_case()
    want = PC.cached_reference("mixed", c)
    assert set(c.modes) == set(PC.MODES) and len(c.modes) == 129
    assert (want[5] & G.FAULT_TOKEN).any() and (want[2] != c.tables.jstate).sum() >= 2
    got = _check(c, want)
    for r, m in enumerate(c.modes):
        if m == "off":
            assert (got[0][r] == c.logits[r]).all(), f"row {r} ({m}) was written"
    # the new kernel alone leaves the regex rows untouched
    alone = _launch(c.logits, c.V, c.tables, c.slot, c.tokens, regex=False)
    for r, m in enumerate(c.modes):
        if m == "regex":
            assert (alone[0][r] == c.logits[r]).all() and (got[0][r] != c.logits[r]).any()
        else:
            assert (alone[0][r] == got[0][r]).all()
    assert (alone[1] == c.tables.gstate).all()
    # null tokens_in: nothing advances
    want0 = PC.reference(c, tokens=None)
    got0 = _check(c, want0, tokens=None)
    assert all((got0[i] == getattr(c.tables, k)).all() for i, k in ((2, "jstate"), (3, "jdepth"), (4, "jstack")))
    # slots outside the table: the row is skipped
    slot = c.slot.copy()
    slot[[2, 3]] = [c.tables.jstate.size, -1]
    c2 = PC.Case(c.V, c.logits, slot, c.tokens, c.tables, c.modes, c.vocab, c.pda)
    got2 = _check(c2, PC.reference(c2))
    assert (got2[0][[2, 3]] == c.logits[[2, 3]]).all()


def test_a_row_alone_equals_the_row_in_the_batch():
    c = PC.mixed_case()
    want = PC.cached_reference("mixed", c)
    for r in (1, 2, 6, 7, 10, 11, 12, 128):
        got = _launch(c.logits[r:r + 1], c.V, c.tables, c.slot[r:r + 1], c.tokens[r:r + 1], shift=r % 8)
        s = int(c.slot[r])
        assert (got[0][0] == want[0][r]).all(), f"row {r} ({c.modes[r]}) alone differs from the row in the batch"
        assert all(got[i][s] == want[i][s] for i in range(1, 6))
        others = np.setdiff1d(np.arange(got[2].size), [s])
        assert (got[2][others] == c.tables.jstate[others]).all() and (got[5][others] == 0).all()


@pytest.mark.parametrize("S", (2, "lds", "lds+1", 1023))
def test_automata_on_both_sides_of_the_lds_threshold(S):
    S = {"lds": J.lds_states(), "lds+1": J.lds_states() + 1}.get(S, S)
    c = PC.general_case(S)
    assert c.pda.n_states == S
    want = PC.reference(c)
    assert want[5].sum() == 0 and (want[3] != c.tables.jdepth).sum() == 3
    got = _check(c, want, shift=S % 8)
    kept = (got[0][:, :c.V] != GC.NINF_BITS).sum(axis=1)
    assert (kept > 0).all() and kept[2] < kept[1]                          # at depth 64 the pushes are gone


def test_the_llama3_vocabulary_with_long_tokens():
    c = PC.wide_case()
    assert np.diff(c.vocab.offsets).max() == 300
    want = PC.reference(c)
    long_tok = c.V - 6
    assert want[5].sum() == 0 and want[2][2] != c.tables.jstate[2]             # the 300-byte token was fed
    assert want[0][1, long_tok] != GC.NINF_BITS or c.logits[1, long_tok] == GC.NINF_BITS   # and is allowed in the other row
    got = _check(c, want, shift=5)
    assert (got[0][1, :c.V] != GC.NINF_BITS).sum() > 1000


def test_a_forbidden_input_token_keeps_the_configuration():
    c = PC.mixed_case()
    rows = [r for r, m in enumerate(c.modes) if m in ("forbidden_in", "beyond_v_in", "empty_in")][:6]
    sub = PC.Case(c.V, c.logits[rows], c.slot[rows], c.tokens[rows], c.tables, tuple(c.modes[r] for r in rows), c.vocab, c.pda)
    got = _check(sub, PC.reference(sub))
    for r in rows:
        s = int(c.slot[r])
        assert got[5][s] == G.FAULT_TOKEN
        assert (got[2][s], got[3][s], got[4][s]) == (c.tables.jstate[s], c.tables.jdepth[s], c.tables.jstack[s])


def test_a_configuration_that_allows_nothing_and_one_out_of_range():
    c = PC.general_case(2)
    tb = SimpleNamespace(**vars(c.tables))
    tb.jstate, tb.jdepth = c.tables.jstate.copy(), c.tables.jdepth.copy()
    tb.eos = np.full(8, -1, dtype=np.int32)
    tb.jstate[4] = 1                                     # state 1 reads nothing, and without an EOS id nothing ends
    tb.jstate[1], tb.jdepth[3] = 2, 65
    c2 = PC.Case(c.V, c.logits, c.slot, c.tokens, tb, c.modes, c.vocab, c.pda)
    want = PC.reference(c2)
    assert want[5][4] == G.FAULT_STUCK and want[5][1] == want[5][3] == G.FAULT_STATE
    got = _check(c2, want)
    assert (got[0][[1, 3, 4]] == c.logits[[1, 3, 4]]).all()


# ------------------------------------------------------------------------------ graph
SLOTS = [4, 1, 3, 0]
JS = {"json_object": True}
PARAMS = [SamplingParams(0.0, seed=1, **JS), SamplingParams(1.3, seed=77, regex=r"[a-c]{2,5}x"),
          SamplingParams(0.9, seed=2), SamplingParams(1.2, top_k=50, seed=14, **JS)]


def _tiny_engine(cfg, slots=6):
    return StageEngine(cfg, 0, cfg.num_hidden_layers, DEV, torch.bfloat16, has_embed=True, has_head=True,
                       source=RandomSource(cfg, 0), max_slots=slots, max_seq=128, max_prefill_rows=64)


def _prefill(eng, slots, prompts):
    eng.reset()
    sl, po = eng.prefill_rows(slots, [len(p) for p in prompts])
    h = eng.forward(eng.embed(torch.tensor([t for p in prompts for t in p], device=DEV)), sl, po)
    eng.advance(slots, [len(p) for p in prompts])
    return h, [int(i) for i in np.cumsum([len(p) for p in prompts]) - 1]


def _vocab(cfg):
    return G.VocabBytes.from_pieces(GC.tiny_pieces(cfg.vocab_size))


def _snapshot(gs) -> SimpleNamespace:
    return SimpleNamespace(**{k: getattr(gs, k).cpu().numpy().copy() for k in PC.ALL_TABLES})


def _reference_step(raw, V, snap, slots, t_in):
    lg, gstate, gfault = G.grammar_mask_reference(raw, V, snap, slots, t_in)
    snap.gfault = gfault
    lg, jstate, jdepth, jstack, gfault = J.pda_mask_reference(lg, V, snap, slots, t_in)
    return lg, {"gstate": gstate, "jstate": jstate, "jdepth": jdepth, "jstack": jstack, "gfault": gfault}


def test_sampling_decode_graph_with_json_rows_and_regex_rows():
    cfg = tiny(layers=2)
    V, eng, vocab = cfg.vocab_size, _tiny_engine(cfg), _vocab(cfg)
    g0 = torch.Generator().manual_seed(3)
    prompts = [torch.randint(3, V, (n,), generator=g0).tolist() for n in (5, 9, 3, 7)]
    h, last = _prefill(eng, SLOTS, prompts)
    gs = GrammarState(eng, 6, vocab, dfa_rows=32, pda=J.BytePDA.json())
    for s, sp in zip(SLOTS, PARAMS):
        gs.admit(s, sp)
    assert gs.jstate.cpu().tolist() == [0, -1, -1, -1, 0, -1] and gs.gstate.cpu().tolist()[1] == 0
    first = Sampler(eng, None, None, gs).sample(h, last, PARAMS, [len(p) for p in prompts], slots=SLOTS)
    calls0 = J.pda_mask_calls()
    g = SamplingDecodeGraph(eng, 4, "full", slots=SLOTS, history_len=16, grammar=gs, debug_raw=True)
    for i, sp in enumerate(PARAMS):
        g.set_params(i, sp)
    g.tokens.copy_(first.to(torch.int32))
    s0 = _snapshot(gs)
    g.capture()
    assert J.pda_mask_calls() == calls0 + 2                       # the warm-up run and the capture
    for k in PC.STATE_WORDS:                                      # the warm-up's advance is undone
        assert (getattr(gs, k).cpu().numpy() == getattr(s0, k)).all(), k
    deepest = 0
    for step in range(16):
        t_in = g.tokens.cpu().tolist()
        snap = _snapshot(gs)
        g.replay()
        torch.cuda.synchronize()
        want_l, want = _reference_step(g.raw_logits.cpu(), V, snap, SLOTS, t_in)
        assert torch.equal(g.logits.cpu().view(torch.int16)[:, :V], want_l.view(torch.int16)[:, :V]), f"replay {step}"
        assert torch.equal(g.logits[:, V:], g.raw_logits[:, V:])
        for k, w in want.items():
            assert (getattr(gs, k).cpu().numpy() == w).all(), (step, k)
        deepest = max(deepest, int(want["jdepth"].max()))
        assert torch.equal(g.logits[2], g.raw_logits[2])          # the plain row
        tok = g.tokens.cpu().tolist()
        assert np.isfinite(g.logits.float().cpu().numpy()[np.arange(4), tok]).all()      # never a masked token
    assert int(gs.gfault.sum()) == 0 and deepest >= 1


def test_a_stage_with_a_pda_but_no_json_rows_equals_one_without():
    cfg = tiny(layers=2)
    V, eng, vocab = cfg.vocab_size, _tiny_engine(cfg), _vocab(cfg)
    g0 = torch.Generator().manual_seed(4)
    prompts = [torch.randint(3, V, (n,), generator=g0).tolist() for n in (5, 9, 3, 7)]
    params = [SamplingParams(0.0, seed=1), SamplingParams(1.3, seed=77, regex=r"[a-c]{2,5}x"), SamplingParams(0.9, seed=2),
              SamplingParams(0.7, top_k=20, seed=3, regex=r"(yes|no)")]
    runs = []
    for kw in ({}, {"pda": J.BytePDA.json()}):
        gs = GrammarState(eng, 6, vocab, dfa_rows=32, **kw)
        h, last = _prefill(eng, SLOTS, prompts)
        for s, sp in zip(SLOTS, params):
            gs.admit(s, sp)
        first = Sampler(eng, None, None, gs).sample(h, last, params, [len(p) for p in prompts], slots=SLOTS).to(torch.int32)
        g = SamplingDecodeGraph(eng, 4, "full", slots=SLOTS, history_len=5, grammar=gs)
        for i, sp in enumerate(params):
            g.set_params(i, sp)
        g.tokens.copy_(first)
        g.capture()
        logits = []
        for _ in range(5):
            g.replay()
            logits.append(g.logits.clone())
        torch.cuda.synchronize()
        runs.append((first.cpu(), g.history.cpu().clone(), torch.stack(logits).cpu().view(torch.int16), gs.gstate.cpu()))
        assert int(gs.gfault.sum()) == 0
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert (gs.jstate == -1).all() and int(gs.jdepth.sum()) == 0 and int(gs.jstack.sum()) == 0


def _check_output(pda, vocab, out, eos=2):
    c = (0, 0, 0)
    for i, t in enumerate(out):
        if t == eos:
            assert pda.accepting(c), out
            assert PC.ok(vocab.decode(out[:i])), vocab.decode(out[:i])
            return True
        c = pda.walk(vocab.token(t), c) if vocab.token(t) else None
        assert c is not None, (out, i)
    return False


def test_captured_generation_is_json():
    cfg = tiny(layers=2)
    V, eng, vocab, pda = cfg.vocab_size, _tiny_engine(cfg), _vocab(cfg), J.BytePDA.json()
    bias = {2: 6.0, 3 + ord("}"): 6.0, 3 + ord('"'): 3.0}
    runs = [SamplingParams(1.0, seed=1, **JS), SamplingParams(0.0, seed=3, **JS),
            SamplingParams(1.0, seed=5, logit_bias=bias, min_p=0.01, **JS),
            SamplingParams(1.0, seed=6, logit_bias=bias, repetition_penalty=1.1, logprobs=2, **JS)]
    g0 = torch.Generator().manual_seed(8)
    prompts = [torch.randint(3, V, (n,), generator=g0).tolist() for n in (6, 4, 9, 5)]
    h, last = _prefill(eng, SLOTS, prompts)
    from llm_sharding_amd.runtime.sampling import ConstraintState, PenaltyState
    gs = GrammarState(eng, 6, vocab, dfa_rows=32, pda=pda)
    cs, ps = ConstraintState(eng, 6, state_rows=1), PenaltyState(eng, 6)
    for s, p, sp in zip(SLOTS, prompts, runs):
        gs.admit(s, sp)
        cs.admit(s, sp, len(p))
        ps.admit(s, p)
    first = Sampler(eng, ps, cs, gs).sample(h, last, runs, [len(p) for p in prompts], slots=SLOTS)
    g = SamplingDecodeGraph(eng, 4, "full", slots=SLOTS, history_len=40, grammar=gs, constraints=cs, penalties=ps,
                            logprobs=True)
    for i, sp in enumerate(runs):
        g.set_params(i, sp)
    g.tokens.copy_(first.to(torch.int32))
    g.capture()
    for _ in range(40):
        g.replay()
    torch.cuda.synchronize()
    hist = g.history.cpu().numpy()
    done = [_check_output(pda, vocab, [int(first[i])] + hist[:, i].tolist()) for i in range(4)]
    assert sum(done) >= 1, done
    assert int(gs.gfault.sum()) == 0 and int(cs.fault.sum()) == 0
    assert torch.isfinite(g.lp_history[:, 3]).all()               # a chosen token is never a masked one


def test_server_with_json_in_graph_mode():
    from llm_sharding_amd.parallel.server import PipelineServer
    cfg = tiny(layers=2)
    vocab, pda = _vocab(cfg), J.BytePDA.json()
    srv = PipelineServer(cfg, RandomSource(cfg, 11), 0, 1, 0, cfg.num_hidden_layers, device=DEV, batch=2,
                         microbatches=2, max_seq=128, prefill_budget=16, vocab_bytes=vocab, dfa_rows=64)
    assert srv.graph_mode and srv.grammar is None
    g0 = torch.Generator().manual_seed(5)
    prompts = [torch.randint(3, cfg.vocab_size, (n,), generator=g0).tolist() for n in (7, 12, 5, 9)]
    bias = {2: 6.0, 3 + ord("}"): 6.0, 3 + ord('"'): 3.0}
    params = [SamplingParams(1.0, seed=1, logit_bias=bias, **JS), SamplingParams(1.5, seed=3, regex=r"(yes|no)"), None,
              SamplingParams(0.0, seed=4, **JS)]
    rids = [srv.submit(p, 30, sampling=sp) for p, sp in zip(prompts, params)]
    srv.serve(stop_when_idle=True)
    outs = [srv.requests[r].output_ids for r in rids]
    for i in (0, 3):
        _check_output(pda, vocab, outs[i])
    assert vocab.decode(outs[1][:-1]) in (b"yes", b"no") and outs[1][-1] == 2
    assert all(isinstance(g, SamplingDecodeGraph) and g.grammar is srv.grammar for g in srv.graphs)
    assert srv.grammar.pda == pda and int(srv.grammar.gfault.sum()) == 0
    assert (srv.grammar.jstate == -1).all() and (srv.grammar.gstate == -1).all()
