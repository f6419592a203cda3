"""Regex-constrained decoding on the device (csrc/sampling/grammar_mask.hip): the kernel against the
numpy reference, bitwise on the logits, ``gstate`` and ``gfault``, on the shared cases
(tests/grammar_cases.py: an unaligned row, one mode per row over a permuted slot table, DFAs on both
sides of ``LDS_STATES``, the Llama-3 vocabulary with long tokens); the captured SamplingDecodeGraph
with a GrammarState replay by replay; and captured generation under a regex on the tiny engine and
the graph-mode server."""
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import grammar_cases as GC
from llm_sharding_amd.config import tiny
from llm_sharding_amd.ops import grammar as G
from llm_sharding_amd.runtime.engine import RandomSource, StageEngine
from llm_sharding_amd.runtime.sampling import (ConstraintState, GrammarState, Sampler, SamplingDecodeGraph,
                                               SamplingParams)

pytestmark = pytest.mark.gpu
DEV = "cuda"
READ_ONLY = ("arena", "accept", "offsets", "data", "gbase", "eos")


def _bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _dev_tables(tb) -> SimpleNamespace:
    return SimpleNamespace(**{k: torch.from_numpy(np.ascontiguousarray(getattr(tb, k))).to(DEV) for k in G.TABLES})


def _launch(logits, V, tb, slot, tokens, shift=0, alt=False):
    """lsa_grammar_mask on numpy inputs -> (logits uint16, gstate, gfault) after the launch; the
    read-only tables must come back unchanged. ``shift``: the row base sits that many elements
    behind a 16-byte boundary."""
    rows, ld = logits.shape
    buf = torch.zeros(rows * ld + 8 + shift, dtype=torch.int16, device=DEV)
    off = (-buf.data_ptr() // 2) % 8 + shift
    lg = buf[off:off + rows * ld].view(rows, ld)
    lg.copy_(torch.from_numpy(logits.view(np.int16)).to(DEV))
    lg = lg.view(torch.bfloat16)
    assert (lg.data_ptr() % 16) // 2 == shift % 8
    d = _dev_tables(tb)
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)  # noqa: E731
    G.grammar_mask(lg, V, rows, i32(slot), None if tokens is None else i32(tokens), d, alt=alt)
    torch.cuda.synchronize()
    for k in READ_ONLY:
        assert (getattr(d, k).cpu().numpy() == getattr(tb, k)).all(), f"{k} was written"
    assert int(buf[:off].abs().sum()) == 0 and int(buf[off + rows * ld:].abs().sum()) == 0
    return _bits(lg), d.gstate.cpu().numpy(), d.gfault.cpu().numpy()


def _same(got, want, what):
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    assert bad.size == 0, f"{len(bad)} {what} differ, first {bad[:4].tolist()}"


def _check(c, want, tokens="own", shift=0, alt=False):
    tok = c.tokens if isinstance(tokens, str) else tokens
    got = _launch(c.logits, c.V, c.tables, c.slot, tok, shift, alt)
    _same(got[0][:, :c.V], want[0][:, :c.V], "logits")
    _same(got[1], want[1], "grammar states")
    _same(got[2], want[2], "fault flags")
    assert (got[0][:, c.V:] == GC.LOGIT_PAD).all()
    again = _launch(c.logits, c.V, c.tables, c.slot, tok, shift, alt)     # a second launch from the same snapshot
    assert all((a == b).all() for a, b in zip(got, again))
    return got


def test_binding_constants_and_refusals():
    assert G.lds_states() >= 64 and G.block_threads() % 64 == 0 and G.max_vocab() >= 128256
    assert G.lds_states(alt=True) >= 64 and G.lds_states(alt=True) != G.lds_states()
    assert max(G.lds_states(), G.lds_states(alt=True)) * 512 + 1024 <= 160 * 1024   # the staged DFA fits one CU's LDS
    c = GC.small_case()
    d = _dev_tables(c.tables)
    lg = torch.zeros((1, c.V), dtype=torch.bfloat16, device=DEV)
    slot = torch.zeros(1, dtype=torch.int32, device=DEV)
    L = G._lib()
    from llm_sharding_amd.ops.hip import _p, _stream
    args = lambda **kw: [kw.get("logits", _p(lg)), c.V, kw.get("V", c.V), kw.get("rows", 1), _p(slot), 2, None,  # noqa: E731
                         kw.get("arena", _p(d.arena)), _p(d.accept), kw.get("dfa_rows", 8), _p(d.offsets), _p(d.data),
                         d.data.numel(), _p(d.gstate), _p(d.gbase), _p(d.gfault), _p(d.eos), _stream()]
    assert L.lsa_grammar_mask(*args()) == 0
    for bad in ({"logits": None}, {"arena": None}, {"V": 0}, {"rows": 32769}, {"rows": 0}, {"dfa_rows": 0}):
        assert L.lsa_grammar_mask(*args(**bad)) == 1, bad                 # LSA_BAD_SHAPE
    with pytest.raises(ValueError):
        G.grammar_mask(lg, c.V, 1, slot, None, SimpleNamespace(**{**vars(d), "arena": d.arena[:, :128]}))
    torch.cuda.synchronize()


@pytest.mark.parametrize("shift", (3, 0, 7))
def test_one_unaligned_row(shift):
    c = GC.small_case()
    ln = np.diff(c.vocab.offsets)
    assert ln.min() == 0 and ln.max() == 20
    want = GC.cached_reference("small", c)
    assert want[2].sum() == 0 and want[1][1] != c.tables.gstate[1]
    got = _check(c, want, shift=shift)
    kept = (got[0][0, :c.V] != GC.NINF_BITS).sum()
    assert 10 < kept < c.V - 10


def test_one_mode_per_row_over_a_permuted_slot_table():
    c = GC.mixed_case()
    want = GC.cached_reference("mixed", c)
    assert set(c.modes) == set(GC.MODES) and len(c.modes) == 129
    flt = want[2]
    assert (flt & G.FAULT_TOKEN).any() and (flt & G.FAULT_STUCK).any() and (want[1] != c.tables.gstate).sum() >= 2
    got = _check(c, want)
    _check(c, want, alt=True)
    for r, m in enumerate(c.modes):
        if m in ("off", "stuck"):
            assert (got[0][r] == c.logits[r]).all(), f"row {r} ({m}) was written"
    # null tokens_in: nothing advances
    want0 = GC.reference(c, tokens=None)
    got0 = _check(c, want0, tokens=None)
    assert (got0[1] == c.tables.gstate).all()
    # slots outside the table: the row is skipped
    slot = c.slot.copy()
    slot[[1, 3]] = [c.tables.gstate.size, -1]
    c2 = GC.Case(c.V, c.logits, slot, c.tokens, c.tables, c.modes, c.vocab)
    got2 = _check(c2, GC.reference(c2))
    assert (got2[0][[1, 3]] == c.logits[[1, 3]]).all()


def test_a_row_alone_equals_the_row_in_the_batch():
    c = GC.mixed_case()
    want = GC.cached_reference("mixed", c)
    for r in (1, 2, 3, 6, 10, 11, 13, 128):
        got = _launch(c.logits[r:r + 1], c.V, c.tables, c.slot[r:r + 1], c.tokens[r:r + 1], shift=r % 8)
        s = int(c.slot[r])
        assert (got[0][0] == want[0][r]).all(), f"row {r} ({c.modes[r]}) alone differs from the row in the batch"
        assert got[1][s] == want[1][s] and got[2][s] == want[2][s]
        others = np.setdiff1d(np.arange(got[1].size), [s])
        assert (got[1][others] == c.tables.gstate[others]).all() and (got[2][others] == 0).all()


@pytest.mark.parametrize("alt", (False, True), ids=("default", "alt"))
def test_dfas_on_both_sides_of_lds_states(alt):
    """Exactly LDS_STATES, LDS_STATES + 1 and 2000 states, for the threshold of either entry; each
    case also runs through the other entry, where the threshold falls elsewhere."""
    c = GC.edge_case(G.lds_states(alt))
    want = GC.reference(c)
    assert want[2].sum() == 0 and (want[1] != c.tables.gstate).sum() == 3
    got = _check(c, want, alt=alt)
    _check(c, want, alt=not alt)
    # from the last state of [ab]{0,n} only EOS remains; from the start every token over {a, b} that fits
    for i in (2, 5, 8):
        assert ((got[0][i, :c.V] != GC.NINF_BITS).nonzero()[0] == [GC.EOS[0]]).all()
    assert (got[0][0, :c.V] != GC.NINF_BITS).sum() > 100


def test_the_llama3_vocabulary_with_long_tokens():
    c = GC.wide_case()
    assert np.diff(c.vocab.offsets).max() == 300
    want = GC.reference(c)
    assert want[2].sum() == 0 and want[1][2] == c.tables.gstate[2] + 300        # the 300-byte token was fed
    got = _check(c, want, shift=5)
    assert (got[0][1, :c.V] != GC.NINF_BITS).sum() > 1000


def test_a_state_outside_the_arena_is_flagged():
    c = GC.small_case()
    tb = SimpleNamespace(**vars(c.tables))
    tb.gstate = c.tables.gstate.copy()
    tb.gstate[1] = c.tables.arena.shape[0] + 3
    c2 = GC.Case(c.V, c.logits, c.slot, c.tokens, tb, c.modes, c.vocab)
    want = GC.reference(c2)
    assert want[2][1] == G.FAULT_STATE
    got = _check(c2, want)
    assert (got[0] == c.logits).all()


# ------------------------------------------------------------------------------ graph
SLOTS = [4, 1, 3, 0]
PATTERNS = [r"-?[0-9]{1,3}(\.[0-9]{2})?", r"[a-c]{2,5}x", None, r"(yes|no)"]
PARAMS = [SamplingParams(0.0, seed=1, regex=PATTERNS[0]), SamplingParams(1.3, seed=77, regex=PATTERNS[1]),
          SamplingParams(0.9, seed=2), SamplingParams(1.2, top_k=50, seed=14, regex=PATTERNS[3])]


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


def _matches(pattern, vocab, out, eos=2):
    n = out.index(eos) if eos in out else len(out)
    data = vocab.decode(out[:n])
    d = G.ByteDFA.from_regex(pattern)
    assert all(t == eos for t in out[n:]), out                             # EOS for ever once it ended
    assert d.walk(data) >= 0, (pattern, data)
    return n < len(out) and bool(re.fullmatch(pattern.encode(), data))


def test_sampling_decode_graph_with_a_grammar():
    cfg = tiny(layers=2)
    V, eng, vocab = cfg.vocab_size, _tiny_engine(cfg), _vocab(cfg)
    g0 = torch.Generator().manual_seed(3)
    prompts = [torch.randint(3, V, (n,), generator=g0).tolist() for n in (5, 9, 3, 7)]
    h, last = _prefill(eng, SLOTS, prompts)
    gs = GrammarState(eng, 6, vocab, dfa_rows=32)
    for s, sp in zip(SLOTS, PARAMS):
        gs.admit(s, sp)
    assert gs.gstate.cpu().tolist()[3] == -1
    first = Sampler(eng, None, None, gs).sample(h, last, PARAMS, [len(p) for p in prompts], slots=SLOTS)
    calls0 = G.grammar_mask_calls()
    g = SamplingDecodeGraph(eng, 4, "full", slots=SLOTS, history_len=4, grammar=gs, debug_raw=True)
    for i, sp in enumerate(PARAMS):
        g.set_params(i, sp)
    g.tokens.copy_(first.to(torch.int32))
    s0 = gs.gstate.cpu().numpy().copy()
    g.capture()
    assert G.grammar_mask_calls() == calls0 + 2                   # the warm-up run and the capture
    assert (gs.gstate.cpu().numpy() == s0).all() and int(gs.gfault.sum()) == 0   # the warm-up's advance is undone
    for step in range(4):
        t_in = g.tokens.cpu().tolist()
        snap = SimpleNamespace(**{k: getattr(gs, k).cpu().numpy().copy() for k in G.TABLES})
        g.replay()
        torch.cuda.synchronize()
        want_l, want_s, want_f = G.grammar_mask_reference(g.raw_logits.cpu(), V, snap, SLOTS, t_in)
        assert torch.equal(g.logits.cpu().view(torch.int16)[:, :V], want_l.view(torch.int16)[:, :V]), f"replay {step}"
        assert torch.equal(g.logits[:, V:], g.raw_logits[:, V:])
        assert (gs.gstate.cpu().numpy() == want_s).all() and (gs.gfault.cpu().numpy() == want_f).all()
        assert torch.equal(g.logits[2], g.raw_logits[2])          # the row without a regex
        tok = g.tokens.cpu().tolist()
        assert np.isfinite(g.logits.float().cpu().numpy()[np.arange(4), tok]).all()      # never a masked token
    assert int(gs.gfault.sum()) == 0
    # a graph built without grammar= launches no such kernel and touches no table
    calls1, s1 = G.grammar_mask_calls(), gs.gstate.clone()
    g2 = SamplingDecodeGraph(eng, 4, "full", slots=SLOTS)
    g2.set_params(1, SamplingParams(0.8, seed=77))
    g2.capture()
    g2.replay()
    torch.cuda.synchronize()
    assert G.grammar_mask_calls() == calls1 and torch.equal(gs.gstate, s1) and g2.grammar is None
    with pytest.raises(RuntimeError, match="GrammarState"):
        g2.set_params(0, PARAMS[0])


def test_a_graph_whose_rows_hold_no_regex_equals_one_without_grammar():
    cfg = tiny(layers=2)
    V, eng, vocab = cfg.vocab_size, _tiny_engine(cfg), _vocab(cfg)
    g0 = torch.Generator().manual_seed(4)
    prompts = [torch.randint(3, V, (n,), generator=g0).tolist() for n in (5, 9, 3, 7)]
    params = [SamplingParams(0.0, seed=1), SamplingParams(1.3, seed=77, top_p=0.9), None, SamplingParams(0.7, top_k=20, seed=3)]
    gs = GrammarState(eng, 6, vocab, dfa_rows=32)
    runs = []
    for kw in ({}, {"grammar": gs}):
        h, last = _prefill(eng, SLOTS, prompts)
        first = eng.head(h, last).to(torch.int32)
        g = SamplingDecodeGraph(eng, 4, "full", slots=SLOTS, history_len=5, **kw)
        for i, sp in enumerate(params):
            g.set_params(i, sp)
        g.tokens.copy_(first)
        g.capture()
        logits = []
        for _ in range(5):
            g.replay()
            logits.append(g.logits.clone())
        torch.cuda.synchronize()
        runs.append((g.history.cpu().clone(), torch.stack(logits).cpu().view(torch.int16)))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert (gs.gstate == -1).all() and int(gs.gfault.sum()) == 0


def test_captured_generation_under_a_regex():
    cfg = tiny(layers=2)
    V, eng, vocab = cfg.vocab_size, _tiny_engine(cfg), _vocab(cfg)
    pats = [PATTERNS[0], PATTERNS[0], PATTERNS[1], PATTERNS[3]]
    runs = [SamplingParams(0.0, seed=1, regex=pats[0]), SamplingParams(1.5, seed=3, regex=pats[1], logprobs=2),
            SamplingParams(1.5, seed=4, regex=pats[2], min_p=0.02, logit_bias={263: 2.0}),
            SamplingParams(1.5, seed=5, regex=pats[3], repetition_penalty=1.3)]
    g0 = torch.Generator().manual_seed(8)
    prompts = [torch.randint(3, V, (n,), generator=g0).tolist() for n in (6, 4, 9, 5)]
    h, last = _prefill(eng, SLOTS, prompts)
    gs = GrammarState(eng, 6, vocab, dfa_rows=32)
    cs = ConstraintState(eng, 6, state_rows=1)
    from llm_sharding_amd.runtime.sampling import PenaltyState
    ps = PenaltyState(eng, 6)
    for s, p, sp in zip(SLOTS, prompts, runs):
        gs.admit(s, sp)
        cs.admit(s, sp, len(p))
        ps.admit(s, p)
    assert gs.alloc.rows_free() == 32 - 8 - 7 - 5                 # two requests share one DFA
    first = Sampler(eng, ps, cs, gs).sample(h, last, runs, [len(p) for p in prompts], slots=SLOTS)
    g = SamplingDecodeGraph(eng, 4, "full", slots=SLOTS, history_len=10, grammar=gs, constraints=cs, penalties=ps,
                            logprobs=True)
    for i, sp in enumerate(runs):
        g.set_params(i, sp)
    g.tokens.copy_(first.to(torch.int32))
    g.capture()
    for _ in range(10):
        g.replay()
    torch.cuda.synchronize()
    hist = g.history.cpu().numpy()
    done = [_matches(pats[i], vocab, [int(first[i])] + hist[:, i].tolist()) for i in range(4)]
    assert sum(done) >= 3, done
    assert int(gs.gfault.sum()) == 0 and int(cs.fault.sum()) == 0
    assert torch.isfinite(g.lp_history[:, 1]).all()               # a chosen token is never a masked one


def test_server_with_regex_in_graph_mode():
    from llm_sharding_amd.parallel.server import PipelineServer
    cfg = tiny(layers=2)
    vocab = _vocab(cfg)
    srv = PipelineServer(cfg, RandomSource(cfg, 11), 0, 1, 0, cfg.num_hidden_layers, device=DEV, batch=2,
                         microbatches=2, max_seq=128, prefill_budget=16, vocab_bytes=vocab, dfa_rows=64)
    assert srv.graph_mode and srv.grammar is None
    g0 = torch.Generator().manual_seed(5)
    prompts = [torch.randint(3, cfg.vocab_size, (n,), generator=g0).tolist() for n in (7, 12, 5, 9, 6)]
    params = [SamplingParams(0.0, seed=1, regex=PATTERNS[0]), SamplingParams(1.5, seed=3, regex=PATTERNS[1]), None,
              SamplingParams(1.5, seed=4, regex=PATTERNS[3], min_p=0.05), SamplingParams(0.7, seed=5)]
    rids = [srv.submit(p, 12, sampling=sp) for p, sp in zip(prompts, params)]
    srv.serve(stop_when_idle=True)
    outs = [srv.requests[r].output_ids for r in rids]
    for i in (0, 1, 3):
        o = outs[i]
        assert G.ByteDFA.from_regex(params[i].regex).walk(vocab.decode(o)) >= 0, o
        if o[-1] == 2:
            assert re.fullmatch(params[i].regex.encode(), vocab.decode(o[:-1])), o
    assert sum(outs[i][-1] == 2 for i in (0, 1, 3)) >= 2
    assert all(isinstance(g, SamplingDecodeGraph) and g.grammar is srv.grammar for g in srv.graphs)
    assert int(srv.grammar.gfault.sum()) == 0 and srv._garena.rows_free() == 64 and (srv.grammar.gstate == -1).all()
    # the plain neighbours got what they get in a server that never saw a regex
    bare = PipelineServer(cfg, RandomSource(cfg, 11), 0, 1, 0, cfg.num_hidden_layers, device=DEV, batch=2,
                          microbatches=2, max_seq=128, prefill_budget=16)
    rb = [bare.submit(prompts[2], 12, sampling=None), bare.submit(prompts[4], 12, sampling=params[4])]
    bare.serve(stop_when_idle=True)
    assert bare.grammar is None and all(g.grammar is None for g in bare.graphs)
    assert bare.requests[rb[0]].output_ids == outs[2] and bare.requests[rb[1]].output_ids == outs[4]
