#!/usr/bin/env python3
"""Measurements behind the prefix pool (profiles/kv_fork.md). Needs a GPU; each part is one step of
scripts/gpu.sh under its own time limit:

    bash scripts/gpu.sh py scripts/bench_prefix.py kernel + py scripts/bench_prefix.py breakeven \\
        + py scripts/bench_prefix.py server + py scripts/bench_prefix.py load

  kernel     lsa_kv_fork (all four non-temporal variants) against the torch slice-copy loop of
             kv_fork_reference, same tensors, same process, alternated; 7B and 70B-stage cache
             shapes, len 128 and 2048, fan-out 1 and 8; time and GB/s of read + write
  breakeven  Llama-2-7B random-init engine: whole prefill of j + s tokens against fork(j) + an
             s-token suffix prefill at position j (s = 32, 31, 1; plain and non-temporal fork) -
             the smallest j that wins at every s is prefix_min_match
  server     PipelineServer, Llama-2-7B random-init, 2048 shared + 32 own tokens: TTFT cold / hit
  load       serve.py's load test with and without --prefix-slots (two child processes)

Every part prints one JSON line per measurement and appends it to --out (default
bench_out/bench_prefix.jsonl).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from llm_sharding_amd.ops import kvcache  # noqa: E402

DEV = "cuda:0"
HBM_COPY_TBS = 6.29  # MI355X_MICROARCH.md: measured float4 copy rate (read + write)


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(out, "a") as f:
        f.write(line + "\n")


def timed(fn, reps):
    """Device-event time of each of ``reps`` calls, in ms."""
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def summary(ts):
    return {"ms_median": statistics.median(ts), "ms_min": min(ts), "ms_max": max(ts)}


def part_kernel(a):
    shapes = {"llama2-7b (32 layers, nkv 32)": (32, 32), "llama2-70b stage (10 of 80 layers, nkv 8)": (10, 8)}
    tmax, hd, slots = 2048, 128, 10
    for name, (layers, nkv) in shapes.items():
        ks = [torch.zeros((slots, nkv, tmax, hd), dtype=torch.bfloat16, device=DEV) for _ in range(layers)]
        vs = [torch.zeros((slots, nkv, tmax, hd), dtype=torch.bfloat16, device=DEV) for _ in range(layers)]
        for t in ks + vs:
            t[0].normal_()
        for n in (128, 2048):
            for f in (1, 8):
                jobs = [(0, n, *range(1, 1 + f))]
                nbytes = 2 * layers * nkv * n * hd * 2 * (1 + f)  # every source byte read once, written f times
                cands = {"torch_loop": lambda: kvcache.kv_fork_reference(ks, vs, jobs)}
                for flags, tag in ((0, "plain"), (1, "nt_load"), (2, "nt_store"), (3, "nt_load_store")):
                    cands[f"lsa_kv_fork/{tag}"] = lambda flags=flags: kvcache.kv_fork(ks, vs, jobs, flags)
                for fn in cands.values():  # warm every candidate at this shape
                    fn()
                torch.cuda.synchronize()
                ts = {k: [] for k in cands}
                for _ in range(a.rounds):  # alternated: one call of each per round
                    for k, fn in cands.items():
                        ts[k] += timed(fn, 1)
                for k in cands:
                    s = summary(ts[k])
                    emit(a.out, {"part": "kernel", "shape": name, "len": n, "fanout": f, "what": k, "bytes": nbytes,
                                 "rounds": a.rounds, **s, "gb_s_median": nbytes / s["ms_median"] / 1e6,
                                 "share_of_copy_rate": nbytes / s["ms_median"] / 1e6 / (HBM_COPY_TBS * 1e3),
                                 "launches": 1 if k != "torch_loop" else 2 * layers * f})
        del ks, vs
        torch.cuda.empty_cache()


def _engine_7b(slots, max_seq, rows):
    from llm_sharding_amd.config import get_preset
    from llm_sharding_amd.runtime.engine import RandomSource, StageEngine
    cfg = get_preset("llama2-7b")
    return cfg, StageEngine(cfg, 0, cfg.num_hidden_layers, DEV, torch.bfloat16, has_embed=True, has_head=True,
                            source=RandomSource(cfg, 0), max_slots=slots, max_seq=max_seq, max_prefill_rows=rows)


def part_breakeven(a):
    cfg, eng = _engine_7b(3, 2048 + 64, 2048 + 64)
    g = torch.Generator().manual_seed(1)

    def prefill(slot, p0, n):
        ids = torch.randint(3, cfg.vocab_size, (n,), generator=g)
        eng.seq_len[slot] = p0
        h = eng.forward(eng.embed(ids), [slot] * n, list(range(p0, p0 + n)))
        eng.seq_len[slot] = p0 + n
        return eng.head(h, [n - 1])

    def fork(j, flags):
        kvcache.kv_fork(eng.k_cache, eng.v_cache, [(0, j, 2)], flags)

    # suffixes on both sides of a 32-row tile boundary: a prefill command's time is a step function of
    # its rows, so what a fork saves at small j depends on whether j moves the command across a step
    for suffix, js in ((32, (1, 2, 4, 8, 16, 32, 64, 128, 512, 2048)), (31, (1, 8, 16, 32, 64, 128)),
                       (1, (1, 8, 16, 32, 64, 128))):
        for j in js:
            prefill(0, 0, j)  # the pooled prefix
            cands = {"whole_prefill": lambda: prefill(1, 0, j + suffix),
                     "fork_plus_suffix/plain": lambda: (fork(j, 0), prefill(2, j, suffix)),
                     "fork_plus_suffix/nt_load_store": lambda: (fork(j, 3), prefill(2, j, suffix)),
                     "fork_only/plain": lambda: fork(j, 0)}
            for fn in cands.values():
                fn()
                fn()
            torch.cuda.synchronize()
            ts = {k: [] for k in cands}
            for _ in range(a.rounds):
                for k, fn in cands.items():
                    t0 = time.perf_counter()  # host clock to a synchronise: what the scheduler loop pays
                    fn()
                    torch.cuda.synchronize()
                    ts[k].append((time.perf_counter() - t0) * 1e3)
            for k in cands:
                emit(a.out, {"part": "breakeven", "j": j, "suffix": suffix, "what": k, "rounds": a.rounds,
                             **summary(ts[k])})


def part_server(a):
    from llm_sharding_amd.config import get_preset
    from llm_sharding_amd.parallel.server import PipelineServer
    from llm_sharding_amd.runtime.engine import RandomSource
    cfg = get_preset("llama2-7b")
    srv = PipelineServer(cfg, RandomSource(cfg, 0), 0, 1, 0, cfg.num_hidden_layers, device=DEV, batch=4,
                         microbatches=2, max_seq=2048 + 128, prefill_budget=2048, prefix_slots=2)
    g = torch.Generator().manual_seed(2)
    rnd = lambda n: torch.randint(3, cfg.vocab_size, (n,), generator=g).tolist()  # noqa: E731

    def ttft(prompt, **kw):
        rid = srv.submit(prompt, 4, eos_ids=(), **kw)
        srv.serve(stop_when_idle=True)
        return srv.requests[rid].ttft_ms

    ttft(rnd(2048) + rnd(32))  # warm the prefill shapes (2048-row chunk, 32-row chunk), no pool involved
    for rep in range(a.rounds):
        shared = rnd(2048)
        emit(a.out, {"part": "server", "rep": rep, "what": "ttft_no_pool_request", "ms": ttft(shared[:-1] + rnd(33))})
        emit(a.out, {"part": "server", "rep": rep, "what": "ttft_cold (fill 2048 + fork + 32)",
                     "ms": ttft(shared + rnd(32), cache_prefix=2048)})
        emit(a.out, {"part": "server", "rep": rep, "what": "ttft_hit (fork 2048 + 32)",
                     "ms": ttft(shared + rnd(32), cache_prefix=2048)})
    emit(a.out, {"part": "server", "what": "stats", **{k: v for k, v in srv.stats().items() if k.startswith("prefix")}})


def part_load(a):
    base = [sys.executable, os.path.join(ROOT, "serve.py"), "--model", "llama2-7b", "--requests", "64", "--prompt-len",
            "2080", "--shared-prefix-len", "2048", "--max-new-tokens", "32", "--batch", "8", "--microbatches", "2",
            "--max-seq", "2176", "--prefill-budget", "2048"]
    for rep in range(2):  # alternated
        for tag, extra in (("without_pool", []), ("prefix_slots_1", ["--prefix-slots", "1"])):
            r = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=280)
            if r.returncode != 0:  # a fault or an abort: start nothing more on the GPU
                print(r.stdout[-4000:], flush=True)
                sys.exit(r.returncode if r.returncode > 0 else 1)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
            emit(a.out, {"part": "load", "rep": rep, "what": tag, **json.loads(line)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=("kernel", "breakeven", "server", "load"))
    ap.add_argument("--rounds", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "bench_prefix.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_prefix.py measures on the GPU: none found")
    a.rounds = a.rounds or {"kernel": 20, "breakeven": 10, "server": 3, "load": 0}[a.part]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    {"kernel": part_kernel, "breakeven": part_breakeven, "server": part_server, "load": part_load}[a.part](a)


if __name__ == "__main__":
    main()
