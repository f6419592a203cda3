#!/usr/bin/env python3
"""Cost of sampling on the device (results: profiles/sampling.md).

1. ``lsa_sample`` alone: device-event time per launch over back-to-back launches, at rows
   1 / 128 / 512 and V 32000 / 128256, for temperature only, top-k 50 and top-p 0.9, on
   bf16-rounded 2.5 * N(0, 1) logits. The bytes one streaming pass over the logits moves are
   printed next to it (the kernel re-reads the row once per pass, from L2 where it fits).
2. TPOT of a 7B-shaped ``SamplingDecodeGraph`` (temperature 0.7, top-p 0.9) against the greedy
   ``DecodeGraph`` of the same engine, at 1 and 512 rows: both graphs replayed in alternation over
   the same positions, device events around each window, median of the rounds.

    python scripts/bench_sampling.py [--layers 32] [--skip-kernel] [--skip-tpot] [--json-out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llm_sharding_amd.config import LlamaConfig  # noqa: E402
from llm_sharding_amd.ops import sampling as S  # noqa: E402
from llm_sharding_amd.runtime.engine import DecodeGraph, RandomSource, StageEngine  # noqa: E402
from llm_sharding_amd.runtime.sampling import SamplingDecodeGraph, SamplingParams  # noqa: E402

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


def bench_kernel(rows: int, V: int, mode: str, iters: int = 200) -> dict:
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
    return {"rows": rows, "V": V, "mode": mode, "us": round(ms * 1e3, 2), "pass_MB": round(rows * V * 2 / 1e6, 2)}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--skip-tpot", action="store_true")
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--json-out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sampling.py measures on the GPU: none found")
    out = {"kernel": [], "tpot": []}
    for V in (() if a.skip_kernel else (32000, 128256)):
        for rows in (1, 128, 512):
            for mode in ("temperature", "top_k", "top_p"):
                r = bench_kernel(rows, V, mode)
                out["kernel"].append(r)
                print(json.dumps(r), flush=True)
    if not a.skip_tpot:
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
