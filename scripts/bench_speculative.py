#!/usr/bin/env python3
"""Speculative decoding on one MI355X (profiles/speculative.md): Llama-2-7B random init, one sequence.

  step     the replayed SpecDecodeGraph step at k = 1, 3, 7, 15 against the 1-row DecodeGraph step,
           context 128 and 2048, same process, alternated; c(k) = spec step / plain step
  kernels  lsa_spec_draft and lsa_spec_accept alone, 200 launches per captured graph
  e2e      tokens/s of a whole generation in script mode, the script = an earlier run's output
           corrupted at every position / every 2nd / every 3rd / nowhere

    python scripts/bench_speculative.py [--parts step,kernels,e2e] [--layers 32] [--json-out FILE]

Times are device events around windows of graph replays (no host work inside a window); every
window is warmed once, the variants of a table alternate within a round, median [min, max].
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llm_sharding_amd.config import get_preset  # noqa: E402
from llm_sharding_amd.ops import speculative as OS  # noqa: E402
from llm_sharding_amd.runtime.engine import DecodeGraph, RandomSource, StageEngine  # noqa: E402
from llm_sharding_amd.runtime.speculative import SpecDecodeGraph  # noqa: E402

DEV = "cuda:0"
MAX_SEQ = 4096
KS = (1, 3, 7, 15)


def _window(fn, n: int) -> float:
    """Milliseconds of ``n`` calls of ``fn`` (enqueue only) between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _stats(xs) -> dict:
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def _engine(layers: int) -> StageEngine:
    cfg = get_preset("llama2-7b")
    cfg.num_hidden_layers = layers
    return StageEngine(cfg, 0, layers, DEV, torch.bfloat16, has_embed=True, has_head=True, source=RandomSource(cfg, 0),
                       max_slots=1, max_seq=MAX_SEQ, max_prefill_rows=128)


def _tokens(n: int, vocab: int, seed: int) -> list:
    return np.random.default_rng(seed).integers(3, vocab, n).tolist()


# ------------------------------------------------------------------------------ step time
def part_step(eng: StageEngine, rounds: int, replays: int) -> list:
    """The K/V the rows read are whatever the cache holds (zeros): the time of a step does not
    depend on the values. A random history over 32000 tokens gives the lookup no match, so the
    context moves by one token per replay in every variant; each window restarts at the context."""
    out = []
    for ctx in (128, 2048):
        eng.seq_len[0] = ctx - 1
        hist = _tokens(ctx, eng.cfg.vocab_size, ctx)
        plain = DecodeGraph(eng, 1, "full").capture()
        graphs = {}
        for k in KS:
            g = SpecDecodeGraph(eng, 1, k)
            g.admit(0, hist, MAX_SEQ - k - ctx, n_prompt=ctx)
            graphs[k] = g.capture()

        def reset_plain():
            plain.pos.fill_(ctx - 1)

        def reset_spec(g):
            g.hlen.fill_(ctx)
            g.done.zero_()

        times = {"plain": [], **{k: [] for k in KS}}
        for r in range(rounds + 1):  # round 0 warms every graph
            reset_plain()
            t = _window(plain.replay, replays) / replays
            if r:
                times["plain"].append(t)
            for k in KS:
                reset_spec(graphs[k])
                t = _window(graphs[k].replay, replays) / replays
                if r:
                    times[k].append(t)
        base = statistics.median(times["plain"])
        row = {"part": "step", "context": ctx, "replays_per_window": replays, "rounds": rounds,
               "plain_ms": _stats(times["plain"])}
        for k in KS:
            row[f"k{k}_ms"] = _stats(times[k])
            row[f"c{k}"] = statistics.median(times[k]) / base
            row[f"accepted_per_step_k{k}"] = float((graphs[k].hlen.item() - ctx) / replays)
        out.append(row)
        print(json.dumps(row), flush=True)
    return out


# ------------------------------------------------------------------------------ kernels alone
def _graph_of(fn, launches: int):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        for _ in range(launches):
            fn()
    return g


def part_kernels(rounds: int, launches: int = 200) -> list:
    out, ld = [], 8192
    i32 = lambda *shape, fill=0: torch.full(shape, fill, dtype=torch.int32, device=DEV)  # noqa: E731
    for L in (128, 4096, ld):
        for vocab, mode in ((32000, "lookup"), (4, "lookup"), (32000, "script")):
            for n_seq, k in ((1, 3), (1, 15), (8, 15)):
                hist = torch.from_numpy(np.random.default_rng(L).integers(0, vocab, (n_seq, ld)).astype(np.int32)).to(DEV)
                hlen, tokens, pos = i32(n_seq, fill=L), i32(n_seq * (k + 1)), i32(n_seq * (k + 1))
                script = hist.clone() if mode == "script" else None
                g = _graph_of(lambda: OS.spec_draft(hist, hlen, k, ld, tokens, pos, (1, 3), script), launches)
                ts = [_window(g.replay, 1) * 1e3 / launches for _ in range(rounds + 1)][1:]
                row = {"part": "kernels", "kernel": "lsa_spec_draft", "mode": mode, "vocab": vocab, "L": L, "n_seq": n_seq,
                       "k": k, "us": _stats(ts)}
                out.append(row)
                print(json.dumps(row), flush=True)
    for n_seq, k in ((1, 3), (1, 15), (8, 15)):  # every draft accepted: k + 1 tokens appended per launch
        rows = n_seq * (k + 1)
        hist, hlen, limit, done = i32(n_seq, ld), i32(n_seq, fill=128), i32(n_seq, fill=ld), i32(n_seq)
        eos, n_acc = i32(8, fill=-1), i32(n_seq)
        tokens, cand = i32(rows, fill=5), i32(rows, fill=5)
        g = _graph_of(lambda: OS.spec_accept(hist, hlen, limit, done, eos, tokens, cand, k, ld, n_acc), launches)
        ts = []
        for _ in range(rounds + 1):
            hlen.fill_(128)
            done.zero_()
            ts.append(_window(g.replay, 1) * 1e3 / launches)
        assert int(hlen[0]) == 128 + launches * (k + 1)
        row = {"part": "kernels", "kernel": "lsa_spec_accept", "n_seq": n_seq, "k": k, "us": _stats(ts[1:])}
        out.append(row)
        print(json.dumps(row), flush=True)
    return out


# ------------------------------------------------------------------------------ end to end
def _prefill(eng: StageEngine, prompt: list) -> None:
    eng.reset()
    for c0 in range(0, len(prompt) - 1, eng.max_prefill_rows):
        chunk = prompt[c0:min(c0 + eng.max_prefill_rows, len(prompt) - 1)]
        slot, pos = eng.prefill_rows([0], [len(chunk)])
        eng.forward(eng.embed(torch.tensor(chunk, dtype=torch.int64)), slot, pos)
        eng.advance([0], [len(chunk)])


def _to_completion(g: SpecDecodeGraph, new: int) -> dict:
    """Untimed: replay in the fewest steps that can finish, looking at the device in between."""
    while not g.all_done():
        left = g.limits[0] - int(g.hlen.item())
        for _ in range(max(1, -(-left // (g.k + 1)))):
            g.replay()
    return g.results()[0]


def part_e2e(eng: StageEngine, rounds: int, ctx: int, new: int, ks) -> list:
    out = []
    prompt = _tokens(ctx, eng.cfg.vocab_size, 7)
    _prefill(eng, prompt)
    plain = DecodeGraph(eng, 1, "full").capture()

    def run_plain():
        plain.pos.fill_(ctx - 1)
        plain.tokens.fill_(prompt[-1])
        return _window(plain.replay, new)

    run_plain()
    ts = [run_plain() for _ in range(rounds)]
    row = {"part": "e2e", "variant": "plain DecodeGraph", "context": ctx, "new_tokens": new,
           "tok_per_s": _stats([new / t * 1e3 for t in ts])}
    out.append(row)
    print(json.dumps(row), flush=True)
    for k in ks:
        look = SpecDecodeGraph(eng, 1, k, history_len=new)
        look.admit(0, prompt, new, n_prompt=ctx)
        look.capture()
        ref = _to_completion(look, new)  # the lookup run whose output the scripts are built from
        g = SpecDecodeGraph(eng, 1, k, script=True, history_len=new)
        g.admit(0, prompt, new, n_prompt=ctx)
        g.capture()
        for every, label in ((1, "every position wrong"), (2, "every 2nd wrong"), (3, "every 3rd wrong"), (0, "all right")):
            script = prompt + ref["tokens"]
            if every:
                for i in range(ctx, len(script), every):
                    script[i] = (script[i] + 1) % eng.cfg.vocab_size
            g.set_script(0, script)
            ts, steps, res = [], 0, None
            for r in range(rounds + 1):
                eng.seq_len[0] = ctx - 1
                g.admit(0, prompt, new, n_prompt=ctx)
                g.step_ctr.zero_()
                g.acc_history.zero_()
                if r == 0:
                    res = _to_completion(g, new)
                    steps = len(res["accepted"])
                    continue
                ts.append(_window(g.replay, steps))
                assert g.all_done() and g.results()[0]["tokens"] == res["tokens"]
            row = {"part": "e2e", "variant": f"script, {label}", "k": k, "context": ctx, "new_tokens": new, "steps": steps,
                   "accepted_per_step": new / steps, "same_tokens_as_lookup_run": res["tokens"] == ref["tokens"],
                   "lookup_run_steps": len(ref["accepted"]), "tok_per_s": _stats([new / t * 1e3 for t in ts])}
            out.append(row)
            print(json.dumps(row), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="step,kernels,e2e")
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--replays", type=int, default=50, help="replays per timed window of part step")
    ap.add_argument("--e2e-new", type=int, default=512)
    ap.add_argument("--e2e-k", default="3,7")
    ap.add_argument("--json-out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_speculative.py measures on the GPU: no device found")
    parts, out = a.parts.split(","), []
    print(json.dumps({"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "layers": a.layers}), flush=True)
    if "kernels" in parts:
        out += part_kernels(a.rounds)
    if "step" in parts or "e2e" in parts:
        eng = _engine(a.layers)
        if "step" in parts:
            out += part_step(eng, a.rounds, a.replays)
        if "e2e" in parts:
            for ctx in (128, 2048):
                out += part_e2e(eng, max(3, a.rounds // 2), ctx, a.e2e_new, [int(k) for k in a.e2e_k.split(",")])
    if a.json_out:
        os.makedirs(os.path.dirname(os.path.abspath(a.json_out)), exist_ok=True)
        with open(a.json_out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
