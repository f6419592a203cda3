#!/usr/bin/env python3
"""Cost of sampling on the device (results: profiles/sampling.md).

1. ``lsa_sample`` alone: device-event time per launch over back-to-back launches, at rows
   1 / 128 / 512 and V 32000 / 128256, for temperature only, top-k 50 and top-p 0.9, on
   bf16-rounded 2.5 * N(0, 1) logits. The bytes one streaming pass over the logits moves are
   printed next to it (the kernel re-reads the row once per pass, from L2 where it fits).
2. TPOT of a 7B-shaped ``SamplingDecodeGraph`` (temperature 0.7, top-p 0.9) against the greedy
   ``DecodeGraph`` of the same engine, at 1 and 512 rows: both graphs replayed in alternation over
   the same positions, device events around each window, median of the rounds.

3. ``--penalties`` (results: profiles/penalties.md) instead: ``lsa_penalize`` alone at 1 and 512
   rows of V = 32000 with about 200 non-zero states per row (rho 1.1, beta 0.2, an input token per
   row) next to ``lsa_sample`` (top-p 0.9) on the same shapes: back-to-back launches and 50
   launches captured in one graph (without the host's launch rate), with the bytes the kernel
   reads (2 x 2 x V per row) and the GB/s they make; and the TPOT of a 7B-shaped ``SamplingDecodeGraph``
   with penalties (temperature 0.7, top-p 0.9, rho 1.1, beta 0.2) against the same graph without.

4. ``--logprobs`` (results: profiles/logprobs.md) instead: ``lsa_logprobs`` alone at 1 and 512 rows
   of V = 32000 for ``n_top`` 0 and 20 (random targets) next to ``lsa_sample`` (top-p 0.9) on the
   same logits, back to back and 50 launches in one graph; and the TPOT of a 7B-shaped
   ``SamplingDecodeGraph`` (temperature 0.7, top-p 0.9) with ``logprobs=5`` against the same graph
   without, in alternating windows of one process.

5. ``--constraints`` (results: profiles/logit_process.md) instead: ``lsa_logit_process`` alone at 1 and
   512 rows of V = 32000 for 320 bias entries, an automaton (half the vocabulary allowed, a
   different arena row per slot) and automaton + min-p (the row kept in registers, and re-read from
   L2), 50 launches captured in one graph: once on
   logits that already carry the masks (reads only) and once with the logits restored in front of
   every launch (reads and writes; the restoring copy, captured alone, is subtracted), next to
   ``lsa_penalize`` and ``lsa_sample`` from the same process; and the TPOT of a 7B-shaped
   ``SamplingDecodeGraph`` whose rows decode under ``choices`` against the same graph without.

6. ``--grammar`` (results: profiles/grammar_mask.md, written by the run) instead: ``lsa_grammar_mask``
   alone at 1 and 512 rows of V = 32000 over a deterministic synthetic vocabulary (256 one-byte
   tokens plus ASCII strings of 2 to 12 bytes), 50 launches captured in one graph, steady (masks in
   place) and fresh (logits restored in front of every launch, the copy subtracted), for a tight
   pattern (``-?[0-9]{1,6}``), a permissive one (``[ -~]*``: every token walks to its end) and a
   permissive DFA on each side of ``LDS_STATES`` (``[ -~]{0,N}``); ``lsa_logit_process`` with the
   equivalent dense automaton in the same process; and the TPOT of a 7B-shaped
   ``SamplingDecodeGraph`` without ``grammar=``, with it and no regex row, and with every row
   under the permissive and the tight pattern.

7. ``--json`` (results: profiles/json_mask.md, written by the run) instead: ``lsa_pda_mask`` (JSON mode, the
   byte-level pushdown automaton ``BytePDA.json()``) alone at 1 and 512 rows of V = 32000 over the same
   synthetic vocabulary, 50 launches captured in one graph, every row at the start of the text
   (only ``{`` and whitespace survive) and inside a string (nearly every token walks to its end),
   in alternating windows with ``lsa_grammar_mask`` under the permissive pattern ``[ -~]*`` and with
   the same automaton padded past the LDS threshold (the L2 path); and the TPOT of a 7B-shaped
   ``SamplingDecodeGraph`` without ``grammar=``, with a ``GrammarState(pda=...)`` and no JSON row, and
   with every row inside a JSON string.

    python scripts/bench_sampling.py [--layers 32] [--skip-kernel] [--skip-tpot] [--json-out FILE]
    python scripts/bench_sampling.py --grammar [--layers 32] [--json-out FILE] [--md-out profiles/grammar_mask.md]
    python scripts/bench_sampling.py --json [--layers 32] [--json-out FILE] [--md-out profiles/json_mask.md]
    python scripts/bench_sampling.py --penalties [--layers 32] [--json-out FILE]
    python scripts/bench_sampling.py --logprobs [--layers 32] [--json-out FILE]
    python scripts/bench_sampling.py --constraints [--layers 32] [--json-out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llm_sharding_amd.config import LlamaConfig  # noqa: E402
from llm_sharding_amd.ops import constraints as K  # noqa: E402
from llm_sharding_amd.ops import grammar as G  # noqa: E402
from llm_sharding_amd.ops import logprobs as LP  # noqa: E402
from llm_sharding_amd.ops import pda as J  # noqa: E402
from llm_sharding_amd.ops import penalties as P  # noqa: E402
from llm_sharding_amd.ops import sampling as S  # noqa: E402
from llm_sharding_amd.runtime.engine import DecodeGraph, RandomSource, StageEngine  # noqa: E402
from llm_sharding_amd.runtime.sampling import (ConstraintState, GrammarState, PenaltyState,  # noqa: E402
                                               SamplingDecodeGraph, SamplingParams)

DEV = "cuda"


def _events(fn, iters: int) -> float:
    """Milliseconds per call of ``fn`` over ``iters`` back-to-back calls (device events)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def _graph_events(fn, iters: int) -> float:
    """Milliseconds per call of ``fn`` with ``iters`` calls captured in one hipGraph: the host's
    launch rate (about 16 us per call through ctypes) is out of the figure."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        for _ in range(iters):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return _events(g.replay, 3) / iters


def bench_kernel(rows: int, V: int, mode: str, iters: int = 200, graphed: bool = False) -> dict:
    g = torch.Generator(device=DEV).manual_seed(rows + V)
    lg = (2.5 * torch.randn((rows, V), generator=g, device=DEV)).to(torch.bfloat16)
    T = torch.full((rows,), 0.7, dtype=torch.float32, device=DEV)
    k = torch.full((rows,), 50 if mode == "top_k" else 0, dtype=torch.int32, device=DEV)
    p = torch.full((rows,), 0.9 if mode == "top_p" else 1.0, dtype=torch.float32, device=DEV)
    seed = torch.arange(1, rows + 1, dtype=torch.int64, device=DEV) * 7919
    ctr = torch.full((rows,), 100, dtype=torch.int32, device=DEV)
    keys = torch.zeros(rows, dtype=torch.int64, device=DEV)

    def run():
        S.sample(lg, V, rows, T, k, p, seed, ctr, keys)

    for _ in range(10):
        run()
    torch.cuda.synchronize()
    ms = statistics.median(_events(run, iters) for _ in range(5))
    out = {"rows": rows, "V": V, "mode": mode, "us": round(ms * 1e3, 2), "pass_MB": round(rows * V * 2 / 1e6, 2)}
    if graphed:
        out["graphed_us"] = round(1e3 * _graph_events(run, 50), 2)
    return out


def bench_tpot(layers: int, rows: int, rounds: int = 5, steps: int = 20) -> dict:
    cfg = LlamaConfig(num_hidden_layers=layers, vocab_size=32000, max_position_embeddings=512, name=f"7B-{layers}L")
    eng = StageEngine(cfg, 0, layers, DEV, torch.bfloat16, has_embed=True, has_head=True, source=RandomSource(cfg, 0),
                      max_slots=rows, max_seq=128, max_prefill_rows=max(rows, 128))
    greedy = DecodeGraph(eng, rows, "full").capture()
    samp = SamplingDecodeGraph(eng, rows, "full")
    for r in range(rows):
        samp.set_params(r, SamplingParams(0.7, top_p=0.9, seed=1000 + r))
    samp.capture()
    # every row starts from its own token: rows that decode identical tokens carry identical
    # activations, and the same GEMMs then run measurably faster (less switching in the MFMA
    # operands) - a greedy batch filled with one token would flatter the greedy graph
    tok0 = torch.randint(3, cfg.vocab_size, (rows,), generator=torch.Generator().manual_seed(7)).to(torch.int32).to(DEV)
    times = {"greedy": [], "sampling": []}
    for _ in range(rounds):
        for name, g in (("greedy", greedy), ("sampling", samp)):
            g.set_positions()  # both graphs walk the same positions 0 .. steps + 3
            g.tokens.copy_(tok0)
            for _ in range(3):
                g.replay()
            torch.cuda.synchronize()
            times[name].append(_events(g.replay, steps))
    tg, ts = statistics.median(times["greedy"]), statistics.median(times["sampling"])
    # where the difference goes: the lm_head with the fused argmax against the lm_head storing
    # bf16 logits, and lsa_sample on those logits (each alone, back to back)
    h = eng.buf_h[:rows]

    def head_argmax():
        eng.head_gemv(h, rows, greedy.keys)

    def head_store():
        samp.sampler.logits_into(h, rows, samp.logits)

    def draw():
        S.sample(samp.logits, cfg.vocab_size, rows, samp.temperature, samp.top_k, samp.top_p, samp.seed, samp.pos,
                 samp.keys, ctr_add=1)

    parts = {}
    for name, fn in (("head_argmax_us", head_argmax), ("head_store_us", head_store), ("lsa_sample_us", draw)):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        parts[name] = round(1e3 * statistics.median(_events(fn, 50) for _ in range(5)), 2)
    del greedy, samp, eng
    torch.cuda.empty_cache()
    return {"layers": layers, "rows": rows, "greedy_ms": round(tg, 4), "sampling_ms": round(ts, 4),
            "delta_ms": round(ts - tg, 4), "delta_pct": round(100 * (ts - tg) / tg, 2),
            "greedy_spread_ms": round(max(times["greedy"]) - min(times["greedy"]), 4),
            "sampling_spread_ms": round(max(times["sampling"]) - min(times["sampling"]), 4), **parts}


def _sparse_state(n_slots: int, width: int, V: int, nonzero: int = 200) -> torch.Tensor:
    """int16 [n_slots, width]: ``nonzero`` random columns per slot hold counts 1..5, half of them
    the prompt bit too."""
    g = torch.Generator().manual_seed(n_slots + V)
    st = torch.zeros((n_slots, width), dtype=torch.int16)
    for s in range(n_slots):
        cols = torch.randperm(V, generator=g)[:nonzero]
        val = torch.randint(1, 6, (nonzero,), generator=g).to(torch.int16)
        val[::2] += -0x8000
        st[s, cols] = val
    return st.to(DEV)


def bench_penalize(rows: int, V: int = 32000, iters: int = 200) -> dict:
    g = torch.Generator(device=DEV).manual_seed(rows + V)
    lg0 = (2.5 * torch.randn((rows, V), generator=g, device=DEV)).to(torch.bfloat16)
    lg = lg0.clone()
    st0 = _sparse_state(rows, V, V)
    st = st0.clone()
    slot = torch.arange(rows, dtype=torch.int32, device=DEV)
    tok = torch.randint(0, V, (rows,), generator=torch.Generator().manual_seed(3)).to(torch.int32).to(DEV)
    rep = torch.full((rows,), 1.1, dtype=torch.float32, device=DEV)
    pres = torch.zeros(rows, dtype=torch.float32, device=DEV)
    freq = torch.full((rows,), 0.2, dtype=torch.float32, device=DEV)

    def run():
        P.penalize(lg, V, rows, slot, tok, st, rep, pres, freq)

    for _ in range(10):
        run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(5):  # the same logits and counts in front of every window
        lg.copy_(lg0)
        st.copy_(st0)
        ms.append(_events(run, iters))
    us = statistics.median(ms) * 1e3
    lg.copy_(lg0)
    st.copy_(st0)
    gus = 1e3 * _graph_events(run, 50)
    read_mb = rows * V * 4 / 1e6
    return {"kernel": "lsa_penalize", "rows": rows, "V": V, "us": round(us, 2), "graphed_us": round(gus, 2),
            "read_MB": round(read_mb, 2), "graphed_GBps": round(read_mb / gus * 1e3, 1)}


def bench_tpot_penalties(layers: int, rows: int, rounds: int = 5, steps: int = 20) -> dict:
    cfg = LlamaConfig(num_hidden_layers=layers, vocab_size=32000, max_position_embeddings=512, name=f"7B-{layers}L")
    eng = StageEngine(cfg, 0, layers, DEV, torch.bfloat16, has_embed=True, has_head=True, source=RandomSource(cfg, 0),
                      max_slots=rows, max_seq=128, max_prefill_rows=max(rows, 128))
    pen = PenaltyState(eng, rows)
    st0 = _sparse_state(rows, cfg.head_rows, cfg.vocab_size)
    graphs = {"sampling": SamplingDecodeGraph(eng, rows, "full"),
              "penalties": SamplingDecodeGraph(eng, rows, "full", penalties=pen)}
    for r in range(rows):
        graphs["sampling"].set_params(r, SamplingParams(0.7, top_p=0.9, seed=1000 + r))
        graphs["penalties"].set_params(r, SamplingParams(0.7, top_p=0.9, seed=1000 + r, repetition_penalty=1.1,
                                                         frequency_penalty=0.2))
    for g in graphs.values():
        g.capture()
    tok0 = torch.randint(3, cfg.vocab_size, (rows,), generator=torch.Generator().manual_seed(7)).to(torch.int32).to(DEV)
    times = {k: [] for k in graphs}
    for _ in range(rounds):
        for name, g in graphs.items():
            g.set_positions()
            g.tokens.copy_(tok0)
            pen.state.copy_(st0)
            for _ in range(3):
                g.replay()
            torch.cuda.synchronize()
            times[name].append(_events(g.replay, steps))
    ts, tp = statistics.median(times["sampling"]), statistics.median(times["penalties"])
    del graphs, pen, eng
    torch.cuda.empty_cache()
    return {"layers": layers, "rows": rows, "sampling_ms": round(ts, 4), "penalties_ms": round(tp, 4),
            "delta_ms": round(tp - ts, 4), "delta_pct": round(100 * (tp - ts) / ts, 2),
            "sampling_spread_ms": round(max(times["sampling"]) - min(times["sampling"]), 4),
            "penalties_spread_ms": round(max(times["penalties"]) - min(times["penalties"]), 4)}


def bench_logprobs(rows: int, n_top: int, V: int = 32000, iters: int = 200) -> dict:
    g = torch.Generator(device=DEV).manual_seed(rows + V)
    lg = (2.5 * torch.randn((rows, V), generator=g, device=DEV)).to(torch.bfloat16)
    nt = torch.full((rows,), n_top, dtype=torch.int32, device=DEV)
    tg = torch.randint(0, V, (rows,), generator=torch.Generator().manual_seed(3)).to(torch.int32).to(DEV)
    out = LP.alloc_outputs(rows, DEV)

    def run():
        LP.logprobs(lg, V, rows, nt, tg, out)

    for _ in range(10):
        run()
    torch.cuda.synchronize()
    us = 1e3 * statistics.median(_events(run, iters) for _ in range(5))
    gus = 1e3 * _graph_events(run, 50)
    return {"kernel": "lsa_logprobs", "rows": rows, "V": V, "n_top": n_top, "us": round(us, 2),
            "graphed_us": round(gus, 2), "pass_MB": round(rows * V * 2 / 1e6, 2)}


def bench_tpot_logprobs(layers: int, rows: int, n_top: int = 5, rounds: int = 5, steps: int = 20) -> dict:
    cfg = LlamaConfig(num_hidden_layers=layers, vocab_size=32000, max_position_embeddings=512, name=f"7B-{layers}L")
    eng = StageEngine(cfg, 0, layers, DEV, torch.bfloat16, has_embed=True, has_head=True, source=RandomSource(cfg, 0),
                      max_slots=rows, max_seq=128, max_prefill_rows=max(rows, 128))
    graphs = {"sampling": SamplingDecodeGraph(eng, rows, "full"),
              "logprobs": SamplingDecodeGraph(eng, rows, "full", logprobs=True)}
    for r in range(rows):
        graphs["sampling"].set_params(r, SamplingParams(0.7, top_p=0.9, seed=1000 + r))
        graphs["logprobs"].set_params(r, SamplingParams(0.7, top_p=0.9, seed=1000 + r, logprobs=n_top))
    for g in graphs.values():
        g.capture()
    tok0 = torch.randint(3, cfg.vocab_size, (rows,), generator=torch.Generator().manual_seed(7)).to(torch.int32).to(DEV)
    times = {k: [] for k in graphs}
    for _ in range(rounds):
        for name, g in graphs.items():
            g.set_positions()
            g.tokens.copy_(tok0)
            for _ in range(3):
                g.replay()
            torch.cuda.synchronize()
            times[name].append(_events(g.replay, steps))
    ts, tl = statistics.median(times["sampling"]), statistics.median(times["logprobs"])
    del graphs, eng
    torch.cuda.empty_cache()
    return {"layers": layers, "rows": rows, "n_top": n_top, "sampling_ms": round(ts, 4), "logprobs_ms": round(tl, 4),
            "delta_ms": round(tl - ts, 4), "delta_pct": round(100 * (tl - ts) / ts, 2),
            "sampling_spread_ms": round(max(times["sampling"]) - min(times["sampling"]), 4),
            "logprobs_spread_ms": round(max(times["logprobs"]) - min(times["logprobs"]), 4)}


def bench_logit_process(rows: int, mode: str, V: int = 32000, reread: bool = False) -> dict:
    """``mode``: "bias" (320 entries), "automaton", "automaton_minp". ``reread``: the min-p pass
    re-reads the row from L2 instead of keeping it in registers."""
    from types import SimpleNamespace
    g = torch.Generator(device=DEV).manual_seed(rows + V)
    lg0 = (2.5 * torch.randn((rows, V), generator=g, device=DEV)).to(torch.bfloat16)
    lg = lg0.clone()
    cg = torch.Generator().manual_seed(rows)
    nxt = torch.randint(0, rows, (rows, V), generator=cg).to(torch.int16)
    nxt[torch.rand((rows, V), generator=cg) < 0.5] = -1
    tok = torch.stack([torch.nonzero(nxt[r] >= 0)[0, 0] for r in range(rows)])
    nxt[torch.arange(rows), tok] = torch.arange(rows, dtype=torch.int16)   # the fed token loops: slot r stays in state r
    tok = tok.to(torch.int32).to(DEV)
    auto = mode != "bias"
    tb = SimpleNamespace(
        arena=nxt.to(DEV),
        astate=(torch.arange(rows, dtype=torch.int32) if auto else torch.full((rows,), -1, dtype=torch.int32)).to(DEV),
        abase=torch.zeros(rows, dtype=torch.int32, device=DEV),
        bias_n=torch.full((rows,), 0 if auto else K.BIAS_MAX, dtype=torch.int32, device=DEV),
        bias_tok=torch.stack([torch.randperm(V, generator=cg)[:K.BIAS_MAX]
                              for _ in range(rows)]).to(torch.int32).to(DEV),
        bias_val=torch.randn((rows, K.BIAS_MAX), generator=cg).to(DEV),
        min_until=torch.zeros(rows, dtype=torch.int32, device=DEV),
        minp_delta=torch.full((rows,), 0.7 * -2.9957 if mode == "automaton_minp" else float("-inf"), device=DEV),
        fault=torch.zeros(rows, dtype=torch.int32, device=DEV),
        eos=torch.full((K.N_EOS,), -1, dtype=torch.int32, device=DEV))
    slot = torch.arange(rows, dtype=torch.int32, device=DEV)
    ctr = torch.full((rows,), 100, dtype=torch.int32, device=DEV)
    a0 = tb.astate.clone()

    def run():
        K.logit_process(lg, V, rows, slot, tok, ctr, tb, reread=reread)

    def restore():
        lg.copy_(lg0)
        tb.astate.copy_(a0)

    def restore_run():
        restore()
        run()

    for _ in range(3):
        restore_run()
    torch.cuda.synchronize()
    steady = statistics.median(1e3 * _graph_events(run, 50) for _ in range(3))       # masks in place: no stores
    both = [1e3 * _graph_events(restore_run, 50) for _ in range(5)]
    copy = [1e3 * _graph_events(restore, 50) for _ in range(5)]
    fresh = statistics.median(both) - statistics.median(copy)
    read_mb = rows * V * (4 if auto else 0) / 1e6
    return {"kernel": "lsa_logit_process", "mode": mode + ("_reread" if reread else ""), "rows": rows, "V": V, "steady_graphed_us": round(steady, 2),
            "fresh_graphed_us": round(fresh, 2), "fresh_spread_us": round(max(both) - min(both), 2),
            "restore_us": round(statistics.median(copy), 2), "read_MB": round(read_mb, 2),
            "steady_GBps": round(read_mb / steady * 1e3, 1) if auto else None}


def bench_tpot_constraints(layers: int, rows: int, rounds: int = 5, steps: int = 20) -> dict:
    cfg = LlamaConfig(num_hidden_layers=layers, vocab_size=32000, max_position_embeddings=512, name=f"7B-{layers}L")
    eng = StageEngine(cfg, 0, layers, DEV, torch.bfloat16, has_embed=True, has_head=True, source=RandomSource(cfg, 0),
                      max_slots=rows, max_seq=128, max_prefill_rows=max(rows, 128))
    # 64 choices of 48 tokens: no row reaches the end of its choice inside a window of 23 steps
    cg = torch.Generator().manual_seed(11)
    choices = [torch.randint(3, cfg.vocab_size, (48,), generator=cg).tolist() for _ in range(64)]
    cs = ConstraintState(eng, rows, state_rows=64 * 48 + 2)
    graphs = {"sampling": SamplingDecodeGraph(eng, rows, "full"),
              "choices": SamplingDecodeGraph(eng, rows, "full", constraints=cs)}
    for r in range(rows):
        graphs["sampling"].set_params(r, SamplingParams(0.7, top_p=0.9, seed=1000 + r))
        sp = SamplingParams(0.7, top_p=0.9, seed=1000 + r, choices=choices)
        cs.admit(r, sp, 1)
        graphs["choices"].set_params(r, sp)
    for g in graphs.values():
        g.capture()
    a0 = cs.astate.clone()
    tok0 = torch.randint(3, cfg.vocab_size, (rows,), generator=torch.Generator().manual_seed(7)).to(torch.int32).to(DEV)
    times = {k: [] for k in graphs}
    for _ in range(rounds):
        for name, g in graphs.items():
            g.set_positions()
            g.tokens.copy_(tok0)
            cs.astate.copy_(a0)
            for _ in range(3):
                g.replay()
            torch.cuda.synchronize()
            times[name].append(_events(g.replay, steps))
    ts, tc = statistics.median(times["sampling"]), statistics.median(times["choices"])
    del graphs, cs, eng
    torch.cuda.empty_cache()
    return {"layers": layers, "rows": rows, "sampling_ms": round(ts, 4), "choices_ms": round(tc, 4),
            "delta_ms": round(tc - ts, 4), "delta_pct": round(100 * (tc - ts) / ts, 2),
            "sampling_spread_ms": round(max(times["sampling"]) - min(times["sampling"]), 4),
            "choices_spread_ms": round(max(times["choices"]) - min(times["choices"]), 4)}


def synthetic_vocab(V: int = 32000) -> "G.VocabBytes":
    """0..2 special, 256 one-byte tokens, then ASCII strings of 2 to 12 bytes: letters, digits,
    spaces and some punctuation, seeded."""
    import numpy as np
    rng = np.random.default_rng(32000)
    alpha = np.frombuffer(b"etaoinshrdlucmfwypvbgkqjxz" * 3 + b"ETAOINSHRD0123456789012345  ..,-_:;()\"'/", dtype=np.uint8)
    pieces = [b""] * 3 + [bytes([b]) for b in range(256)]
    pieces += [rng.choice(alpha, int(rng.integers(2, 13))).tobytes() for _ in range(V - len(pieces))]
    return G.VocabBytes.from_pieces(pieces)


def _steady_fresh(run, restore) -> dict:
    def restore_run():
        restore()
        run()

    for _ in range(3):
        restore_run()
    torch.cuda.synchronize()
    steady = statistics.median(1e3 * _graph_events(run, 50) for _ in range(3))       # masks in place: no stores
    both = [1e3 * _graph_events(restore_run, 50) for _ in range(5)]
    copy = [1e3 * _graph_events(restore, 50) for _ in range(5)]
    return {"steady_graphed_us": round(steady, 2), "fresh_graphed_us": round(statistics.median(both) - statistics.median(copy), 2),
            "fresh_spread_us": round(max(both) - min(both), 2), "restore_us": round(statistics.median(copy), 2)}


def bench_grammar_mask(rows: int, pattern: str, vocab, dense: bool = True) -> list:
    """``lsa_grammar_mask`` and ``lsa_grammar_mask_alt`` (the other LDS threshold) with every row in
    the start state of ``pattern``'s DFA, and (``dense``) ``lsa_logit_process`` with the equivalent
    dense automaton, on the same logits."""
    from types import SimpleNamespace
    V = vocab.V
    g = torch.Generator(device=DEV).manual_seed(rows + V)
    lg0 = (2.5 * torch.randn((rows, V), generator=g, device=DEV)).to(torch.bfloat16)
    lg = lg0.clone()
    dfa = G.ByteDFA.from_regex(pattern)
    S = dfa.n_states
    flags = dfa.accept.astype("uint8") * G.ACCEPT
    flags[S - 1] |= G.LAST
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=DEV)  # noqa: E731
    tb = SimpleNamespace(arena=torch.from_numpy(dfa.next.copy()).to(DEV), accept=torch.from_numpy(flags).to(DEV),
                         offsets=torch.from_numpy(vocab.offsets.copy()).to(DEV), data=torch.from_numpy(vocab.data.copy()).to(DEV),
                         gstate=torch.zeros(rows, dtype=torch.int32, device=DEV),
                         gbase=torch.zeros(rows, dtype=torch.int32, device=DEV),
                         gfault=torch.zeros(rows, dtype=torch.int32, device=DEV), eos=i32([2] + [-1] * 7))
    slot = torch.arange(rows, dtype=torch.int32, device=DEV)

    def run():
        G.grammar_mask(lg, V, rows, slot, None, tb)

    def run_alt():
        G.grammar_mask(lg, V, rows, slot, None, tb, alt=True)

    def restore():
        lg.copy_(lg0)

    allowed = int((dfa.step_tokens(vocab, [0])[0] >= 0).sum())
    out = []
    for name, fn, alt in (("lsa_grammar_mask", run, False), ("lsa_grammar_mask_alt", run_alt, True)):
        path = f"lds<={G.lds_states(alt)}" if S <= G.lds_states(alt) else f"global>{G.lds_states(alt)}"
        out.append({"kernel": name, "pattern": pattern, "states": S, "path": path, "rows": rows, "V": V,
                    "allowed": allowed, **_steady_fresh(fn, restore), "table_KB": round(S * 512 / 1024, 1)})
    assert int(tb.gfault.sum()) == 0
    if dense:
        auto = dfa.to_token_automaton(vocab, [2])
        ct = SimpleNamespace(arena=torch.from_numpy(auto.next.copy()).to(DEV),
                             astate=torch.zeros(rows, dtype=torch.int32, device=DEV),
                             abase=torch.zeros(rows, dtype=torch.int32, device=DEV),
                             bias_n=torch.zeros(rows, dtype=torch.int32, device=DEV),
                             bias_tok=torch.zeros((rows, K.BIAS_MAX), dtype=torch.int32, device=DEV),
                             bias_val=torch.zeros((rows, K.BIAS_MAX), dtype=torch.float32, device=DEV),
                             min_until=torch.zeros(rows, dtype=torch.int32, device=DEV),
                             minp_delta=torch.full((rows,), float("-inf"), device=DEV),
                             fault=torch.zeros(rows, dtype=torch.int32, device=DEV), eos=i32([2] + [-1] * 7))
        ctr = torch.full((rows,), 100, dtype=torch.int32, device=DEV)

        def run_dense():
            K.logit_process(lg, V, rows, slot, None, ctr, ct)

        restore()                                 # the two kernels must produce the same row
        run()
        masked = lg.clone()
        restore()
        run_dense()
        torch.cuda.synchronize()
        assert torch.equal(masked.view(torch.int16), lg.view(torch.int16)), "dense and byte-level masks differ"
        out.append({"kernel": "lsa_logit_process", "pattern": pattern, "states": auto.n_states, "path": "dense", "rows": rows,
                    "V": V, "allowed": allowed, **_steady_fresh(run_dense, restore),
                    "table_KB": round(auto.n_states * V * 2 / 1024, 1)})
    return out


def bench_tpot_grammar(layers: int, rows: int, vocab, rounds: int = 5, steps: int = 20) -> dict:
    cfg = LlamaConfig(num_hidden_layers=layers, vocab_size=32000, max_position_embeddings=512, name=f"7B-{layers}L")
    eng = StageEngine(cfg, 0, layers, DEV, torch.bfloat16, has_embed=True, has_head=True, source=RandomSource(cfg, 0),
                      max_slots=rows, max_seq=128, max_prefill_rows=max(rows, 128))
    gs = GrammarState(eng, rows, vocab, dfa_rows=64)
    graphs = {"sampling": SamplingDecodeGraph(eng, rows, "full"),
              "grammar_idle": SamplingDecodeGraph(eng, rows, "full", grammar=gs),
              "permissive": SamplingDecodeGraph(eng, rows, "full", grammar=gs),
              "tight": SamplingDecodeGraph(eng, rows, "full", grammar=gs)}
    pats = {"permissive": "[ -~]*", "tight": "-?[0-9]{1,6}"}
    sps = {k: SamplingParams(0.7, top_p=0.9, seed=1000, regex=v) for k, v in pats.items()}
    for r in range(rows):
        for name, g in graphs.items():
            kw = {"regex": pats[name]} if name in pats else {}
            g.set_params(r, SamplingParams(0.7, top_p=0.9, seed=1000 + r, **kw))
    for g in graphs.values():
        g.capture()
    tok0 = torch.randint(3, cfg.vocab_size, (rows,), generator=torch.Generator().manual_seed(7)).to(torch.int32).to(DEV)
    times = {k: [] for k in graphs}
    for _ in range(rounds):
        for name, g in graphs.items():
            for r in range(rows):                 # every row at the start state of the graph's pattern, or none
                gs.admit(r, sps.get(name))
            g.set_positions()
            # under a pattern the first input is the one-byte token "1", which both patterns take
            g.tokens.copy_(tok0 if name not in pats else torch.full_like(tok0, 3 + ord("1")))
            for _ in range(3):
                g.replay()
            torch.cuda.synchronize()
            times[name].append(_events(g.replay, steps))
    med = {k: statistics.median(v) for k, v in times.items()}
    fault = int(gs.gfault.sum())
    del graphs, gs, eng
    torch.cuda.empty_cache()
    out = {"layers": layers, "rows": rows, "gfault": fault}
    for k, v in med.items():
        out[f"{k}_ms"] = round(v, 4)
        out[f"{k}_spread_ms"] = round(max(times[k]) - min(times[k]), 4)
        if k != "sampling":
            out[f"{k}_delta_ms"] = round(v - med["sampling"], 4)
    return out


def grammar_markdown(out: dict) -> str:
    L, T = G.lds_states(), G.block_threads()
    lines = ["# lsa_grammar_mask on MI355X", "",
             f"`python scripts/bench_sampling.py --grammar`: `LDS_STATES` = {L} (`lsa_grammar_mask_alt`, the same kernel: "
             f"{G.lds_states(alt=True)}), {T} threads per row (one workgroup). "
             "V = 32000 over the synthetic vocabulary (256 one-byte tokens plus seeded ASCII strings of 2 to 12 bytes); "
             "50 launches captured in one graph, every row in its pattern's start state. steady: the masks are already "
             "in place (reads only); fresh: the logits are restored in front of every launch and the restoring copy, "
             "captured alone, is subtracted. `lsa_logit_process` runs the equivalent dense automaton "
             "(`to_token_automaton`) on the same logits in the same process; both produced the same bits.", "",
             "| kernel | pattern | states | table | walk | rows | allowed | steady us | fresh us | fresh spread us |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for r in out["kernel"]:
        lines.append(f"| {r['kernel']} | `{r['pattern']}` | {r['states']} | {r['table_KB']} KB | {r['path']} | {r['rows']} | "
                     f"{r['allowed']} | {r['steady_graphed_us']} | {r['fresh_graphed_us']} | {r['fresh_spread_us']} |")
    if out["tpot"]:
        lines += ["", "Step time of a 7B-shaped `SamplingDecodeGraph` (temperature 0.7, top-p 0.9), alternating windows of "
                  "20 replays in one process, median of 5: without `grammar=`, with it and no regex row (every row "
                  "skipped), and with every row under the permissive and the tight pattern.", "",
                  "| layers | rows | sampling ms | grammar, no regex row ms | permissive ms | tight ms | spreads ms |",
                  "|---|---|---|---|---|---|---|"]
        for r in out["tpot"]:
            lines.append(f"| {r['layers']} | {r['rows']} | {r['sampling_ms']} | {r['grammar_idle_ms']} "
                         f"({r['grammar_idle_delta_ms']:+}) | {r['permissive_ms']} ({r['permissive_delta_ms']:+}) | "
                         f"{r['tight_ms']} ({r['tight_delta_ms']:+}) | {r['sampling_spread_ms']} / {r['grammar_idle_spread_ms']} / "
                         f"{r['permissive_spread_ms']} / {r['tight_spread_ms']} |")
    return "\n".join(lines) + "\n"


def main_grammar(a) -> dict:
    out = {"kernel": [], "tpot": [], "lds_states": G.lds_states(), "threads": G.block_threads()}
    vocab = synthetic_vocab()
    edges = sorted({G.lds_states(), G.lds_states(alt=True)})
    pats = ("-?[0-9]{1,6}", "[ -~]*") + tuple("[ -~]{0,%d}" % n for L in edges for n in (L - 1, L))
    for rows in (1, 512):
        for p in pats:
            for r in bench_grammar_mask(rows, p, vocab):
                out["kernel"].append(r)
                print(json.dumps(r), flush=True)
    if not a.skip_tpot:
        for rows in (1, 512):
            r = bench_tpot_grammar(a.layers, rows, vocab)
            out["tpot"].append(r)
            print(json.dumps(r), flush=True)
    if a.md_out:
        os.makedirs(os.path.dirname(os.path.abspath(a.md_out)), exist_ok=True)
        with open(a.md_out, "w") as f:
            f.write(grammar_markdown(out))
    return out


JSON_CONFIGS = {"start": b"", "in_string": b'{"key":"'}


def padded_pda(pda: "J.BytePDA", states: int) -> "J.BytePDA":
    """``pda`` with unreachable dead states appended up to ``states``: the same language and the same
    walks, a table past the LDS threshold."""
    import numpy as np
    nxt = np.full((3, states, 256), -1, dtype=np.int16)
    nxt[:, :pda.n_states] = pda.next
    acc = np.zeros(states, dtype=np.uint8)
    acc[:pda.n_states] = pda.accept
    return J.BytePDA(nxt, acc)


def bench_pda_mask(rows: int, vocab, rounds: int = 5) -> list:
    """``lsa_pda_mask`` with every row in one configuration of the JSON automaton, staged into LDS
    and (padded) walked from L2, and ``lsa_grammar_mask`` under ``[ -~]*``, on the same logits, in
    alternating windows of 50 captured launches; the two walks of the automaton must give the same
    bits."""
    from types import SimpleNamespace
    V = vocab.V
    g = torch.Generator(device=DEV).manual_seed(rows + V)
    lg0 = (2.5 * torch.randn((rows, V), generator=g, device=DEV)).to(torch.bfloat16)
    lg = lg0.clone()
    pda = J.BytePDA.json()
    big = padded_pda(pda, J.lds_states() + 1)
    dfa = G.ByteDFA.from_regex("[ -~]*")
    flags = dfa.accept.astype("uint8") * G.ACCEPT
    flags[dfa.n_states - 1] |= G.LAST
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=DEV)  # noqa: E731
    z = lambda dt=torch.int32: torch.zeros(rows, dtype=dt, device=DEV)  # noqa: E731
    shared = dict(offsets=torch.from_numpy(vocab.offsets.copy()).to(DEV), data=torch.from_numpy(vocab.data.copy()).to(DEV),
                  eos=i32([2] + [-1] * 7))
    rx = SimpleNamespace(arena=torch.from_numpy(dfa.next.copy()).to(DEV), accept=torch.from_numpy(flags).to(DEV),
                         gstate=z(), gbase=z(), gfault=z(), **shared)
    slot = torch.arange(rows, dtype=torch.int32, device=DEV)

    def restore():
        lg.copy_(lg0)

    out = []
    for label, prefix in JSON_CONFIGS.items():
        q, d, st = pda.walk(prefix)
        tbs = {}
        for name, p in (("lds", pda), ("l2", big)):
            tbs[name] = SimpleNamespace(ptab=torch.from_numpy(p.next.copy()).to(DEV),
                                        paccept=torch.from_numpy(p.accept.copy()).to(DEV),
                                        jstate=torch.full((rows,), q, dtype=torch.int32, device=DEV),
                                        jdepth=torch.full((rows,), d, dtype=torch.int32, device=DEV),
                                        jstack=torch.full((rows,), st, dtype=torch.int64, device=DEV), gfault=z(), **shared)
        fns = {"lsa_pda_mask lds": lambda: J.pda_mask(lg, V, rows, slot, None, tbs["lds"]),
               "lsa_pda_mask l2": lambda: J.pda_mask(lg, V, rows, slot, None, tbs["l2"]),
               "lsa_grammar_mask [ -~]*": lambda: G.grammar_mask(lg, V, rows, slot, None, rx)}
        masks = {}
        for name in ("lsa_pda_mask lds", "lsa_pda_mask l2"):
            restore()
            fns[name]()
            masks[name] = lg.clone()
        torch.cuda.synchronize()
        assert torch.equal(masks["lsa_pda_mask lds"].view(torch.int16), masks["lsa_pda_mask l2"].view(torch.int16))
        allowed = int((masks["lsa_pda_mask lds"][0] != float("-inf")).sum())
        res = {name: [] for name in fns}
        for _ in range(rounds):                    # alternating windows: one _steady_fresh per kernel and round
            for name, fn in fns.items():
                res[name].append(_steady_fresh(fn, restore))
        for name in fns:
            r = {k: round(statistics.median(x[k] for x in res[name]), 2) for k in ("steady_graphed_us", "fresh_graphed_us")}
            r["fresh_spread_us"] = round(max(x["fresh_graphed_us"] for x in res[name]) - min(x["fresh_graphed_us"] for x in res[name]), 2)
            states = dfa.n_states if "grammar" in name else (big if name.endswith("l2") else pda).n_states
            out.append({"kernel": name, "config": label if "pda" in name else "start state", "states": states, "rows": rows,
                        "V": V, "allowed": allowed if "pda" in name else int((dfa.step_tokens(vocab, [0])[0] >= 0).sum()),
                        "table_KB": round(states * (1536 if "pda" in name else 512) / 1024, 1), **r})
        assert int(tbs["lds"].gfault.sum()) == 0 and int(tbs["l2"].gfault.sum()) == 0 and int(rx.gfault.sum()) == 0
    return out


def bench_tpot_json(layers: int, rows: int, vocab, rounds: int = 5, steps: int = 20) -> dict:
    cfg = LlamaConfig(num_hidden_layers=layers, vocab_size=32000, max_position_embeddings=512, name=f"7B-{layers}L")
    eng = StageEngine(cfg, 0, layers, DEV, torch.bfloat16, has_embed=True, has_head=True, source=RandomSource(cfg, 0),
                      max_slots=rows, max_seq=128, max_prefill_rows=max(rows, 128))
    pda = J.BytePDA.json()
    gs = GrammarState(eng, rows, vocab, dfa_rows=64, pda=pda)
    graphs = {"sampling": SamplingDecodeGraph(eng, rows, "full"),
              "json_idle": SamplingDecodeGraph(eng, rows, "full", grammar=gs),
              "json": SamplingDecodeGraph(eng, rows, "full", grammar=gs)}
    for r in range(rows):
        for name, g in graphs.items():
            g.set_params(r, SamplingParams(0.7, top_p=0.9, seed=1000 + r, json_object=name == "json"))
    for g in graphs.values():
        g.capture()
    tok0 = torch.randint(3, cfg.vocab_size, (rows,), generator=torch.Generator().manual_seed(7)).to(torch.int32).to(DEV)
    q, d, st = pda.walk(JSON_CONFIGS["in_string"])
    js = SamplingParams(0.7, top_p=0.9, seed=1000, json_object=True)
    times = {k: [] for k in graphs}
    for _ in range(rounds):
        for name, g in graphs.items():
            for r in range(rows):
                gs.admit(r, js if name == "json" else None)
            if name == "json":                    # every row inside a string: nearly every token walks to its end
                gs.jstate.fill_(q)
                gs.jdepth.fill_(d)
                gs.jstack.fill_(st)
            g.set_positions()
            g.tokens.copy_(tok0 if name != "json" else torch.full_like(tok0, 3 + ord("a")))
            for _ in range(3):
                g.replay()
            torch.cuda.synchronize()
            times[name].append(_events(g.replay, steps))
    med = {k: statistics.median(v) for k, v in times.items()}
    fault = int(gs.gfault.sum())
    del graphs, gs, eng
    torch.cuda.empty_cache()
    out = {"layers": layers, "rows": rows, "gfault": fault}
    for k, v in med.items():
        out[f"{k}_ms"] = round(v, 4)
        out[f"{k}_spread_ms"] = round(max(times[k]) - min(times[k]), 4)
        if k != "sampling":
            out[f"{k}_delta_ms"] = round(v - med["sampling"], 4)
    return out


def json_markdown(out: dict) -> str:
    pda = J.BytePDA.json()
    lines = ["# lsa_pda_mask (JSON mode) on MI355X", "",
             f"`python scripts/bench_sampling.py --json`: the automaton `BytePDA.json()` (top level an object, "
             f"`max_ws` = 2) has {pda.n_states} states = {pda.n_states * 1536} bytes of LDS for its three planes "
             f"(1536 B per state; the kernel stages automata of up to {J.lds_states()} states = "
             f"{J.lds_states() * 1536} bytes, larger ones are walked from L2); `BytePDA.json(max_ws=8)` has "
             f"{J.BytePDA.json(max_ws=8).n_states} states and takes the L2 path. {J.block_threads()} threads per row (one "
             "workgroup). V = 32000 over the synthetic vocabulary (256 one-byte tokens plus seeded ASCII strings of 2 to 12 "
             "bytes); 50 launches captured in one graph, all kernels in one process in alternating windows, median of 5 "
             "rounds. steady: the masks are already in place (reads only); fresh: the logits are restored in front of every "
             "launch and the restoring copy, captured alone, is subtracted. `start`: every row at the start of the text "
             "(only `{` and whitespace survive, nearly every walk dies at its first byte); `in_string`: every row inside a "
             "string (nearly every token walks to its end). `l2`: the same automaton padded with dead states to "
             f"{J.lds_states() + 1} states, the same bits. `lsa_grammar_mask` under `[ -~]*` is the regex kernel's "
             "every-token-walks-to-its-end case.", "",
             "| kernel | configuration | states | table | rows | allowed | steady us | fresh us | fresh spread us |",
             "|---|---|---|---|---|---|---|---|---|"]
    for r in out["kernel"]:
        lines.append(f"| {r['kernel']} | {r['config']} | {r['states']} | {r['table_KB']} KB | {r['rows']} | {r['allowed']} | "
                     f"{r['steady_graphed_us']} | {r['fresh_graphed_us']} | {r['fresh_spread_us']} |")
    if out["tpot"]:
        lines += ["", "Step time of a 7B-shaped `SamplingDecodeGraph` (temperature 0.7, top-p 0.9), alternating windows of "
                  "20 replays in one process, median of 5: without `grammar=`, with a `GrammarState(pda=...)` and no JSON row "
                  "(both mask kernels skip every row), and with every row a JSON row that starts inside a string.", "",
                  "| layers | rows | sampling ms | stage, no JSON row ms | JSON rows ms | spreads ms |", "|---|---|---|---|---|---|"]
        for r in out["tpot"]:
            lines.append(f"| {r['layers']} | {r['rows']} | {r['sampling_ms']} | {r['json_idle_ms']} ({r['json_idle_delta_ms']:+}) | "
                         f"{r['json_ms']} ({r['json_delta_ms']:+}) | {r['sampling_spread_ms']} / {r['json_idle_spread_ms']} / "
                         f"{r['json_spread_ms']} |")
    return "\n".join(lines) + "\n"


def main_json(a) -> dict:
    out = {"kernel": [], "tpot": [], "lds_states": J.lds_states(), "threads": J.block_threads(),
           "json_states": J.BytePDA.json().n_states}
    vocab = synthetic_vocab()
    for rows in (1, 512):
        for r in bench_pda_mask(rows, vocab):
            out["kernel"].append(r)
            print(json.dumps(r), flush=True)
    if not a.skip_tpot:
        for rows in (1, 512):
            r = bench_tpot_json(a.layers, rows, vocab)
            out["tpot"].append(r)
            print(json.dumps(r), flush=True)
    md = a.md_out if a.md_out != "profiles/grammar_mask.md" else "profiles/json_mask.md"
    os.makedirs(os.path.dirname(os.path.abspath(md)), exist_ok=True)
    with open(md, "w") as f:
        f.write(json_markdown(out))
    return out


def main_constraints(a) -> dict:
    out = {"kernel": [], "tpot": []}
    for rows in (1, 512):
        rs = [bench_logit_process(rows, m) for m in ("bias", "automaton", "automaton_minp")]
        rs.append(bench_logit_process(rows, "automaton_minp", reread=True))
        for r in rs + [bench_penalize(rows), bench_kernel(rows, 32000, "top_p", graphed=True)]:
            out["kernel"].append(r)
            print(json.dumps(r), flush=True)
    if not a.skip_tpot:
        for rows in (1, 512):
            r = bench_tpot_constraints(a.layers, rows)
            out["tpot"].append(r)
            print(json.dumps(r), flush=True)
    return out


def main_logprobs(a) -> dict:
    out = {"kernel": [], "tpot": []}
    for rows in (1, 512):
        for r in (bench_logprobs(rows, 0), bench_logprobs(rows, 20), bench_kernel(rows, 32000, "top_p", graphed=True)):
            out["kernel"].append(r)
            print(json.dumps(r), flush=True)
    if not a.skip_tpot:
        for rows in (1, 512):
            r = bench_tpot_logprobs(a.layers, rows)
            out["tpot"].append(r)
            print(json.dumps(r), flush=True)
    return out


def main_penalties(a) -> dict:
    out = {"kernel": [], "tpot": []}
    for rows in (1, 512):
        for r in (bench_penalize(rows), bench_kernel(rows, 32000, "top_p", graphed=True)):
            out["kernel"].append(r)
            print(json.dumps(r), flush=True)
    if not a.skip_tpot:
        for rows in (1, 512):
            r = bench_tpot_penalties(a.layers, rows)
            out["tpot"].append(r)
            print(json.dumps(r), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--skip-tpot", action="store_true")
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--penalties", action="store_true", help="measure lsa_penalize and the penalised step instead")
    ap.add_argument("--logprobs", action="store_true", help="measure lsa_logprobs and the step with logprobs=5 instead")
    ap.add_argument("--constraints", action="store_true",
                    help="measure lsa_logit_process and the step under choices instead")
    ap.add_argument("--grammar", action="store_true",
                    help="measure lsa_grammar_mask, the dense automaton beside it and the step under a regex instead")
    ap.add_argument("--json", action="store_true",
                    help="measure lsa_pda_mask (JSON mode), the regex kernel beside it and the step with JSON rows instead")
    ap.add_argument("--md-out", default="profiles/grammar_mask.md",
                    help="--grammar / --json: where the table goes (--json: profiles/json_mask.md by default)")
    ap.add_argument("--json-out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sampling.py measures on the GPU: none found")
    special = a.penalties or a.logprobs or a.constraints or a.grammar or a.json
    out = (main_penalties(a) if a.penalties else main_logprobs(a) if a.logprobs else
           main_constraints(a) if a.constraints else main_grammar(a) if a.grammar else
           main_json(a) if a.json else {"kernel": [], "tpot": []})
    for V in (() if a.skip_kernel or special else (32000, 128256)):
        for rows in (1, 128, 512):
            for mode in ("temperature", "top_k", "top_p"):
                r = bench_kernel(rows, V, mode)
                out["kernel"].append(r)
                print(json.dumps(r), flush=True)
    if not a.skip_tpot and not special:
        for rows in (1, 512):
            r = bench_tpot(a.layers, rows)
            out["tpot"].append(r)
            print(json.dumps(r), flush=True)
    if a.json_out:
        os.makedirs(os.path.dirname(os.path.abspath(a.json_out)), exist_ok=True)
        with open(a.json_out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
