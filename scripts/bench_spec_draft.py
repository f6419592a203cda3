#!/usr/bin/env python3
"""The speculative step with a draft model on one MI355X (profiles/spec_draft_model.md).

Llama-2-7B random init (32 layers, bf16), one sequence, contexts 128 and 2048, k = 3 and 7. Four
captured graphs per context and k, in one process, alternated within every round:

  plain   the 1-row DecodeGraph step
  ngram   SpecDecodeGraph with the n-gram lookup (the step as it was before draft models)
  draft   SpecDecodeGraph(draft=...): dm_begin, k draft iterations, dm_chain, then the same verification
  dm      the draft part of that step alone (dm_begin .. the last dm_chain), captured on its own

Draft models, random init: ``2l`` = two layers of the 7B's width and vocabulary; ``llama3.2-3b`` is
run only if its vocabulary is the target's (it is not: 128256 against 32000, so it is skipped).

    python scripts/bench_spec_draft.py [--layers 32] [--rounds 10] [--replays 50] [--out FILE.md] [--json-out FILE]

Times are device events around windows of graph replays (no host work inside a window); every
window is warmed once (round 0), median [min, max] over the rounds. Random-init models agree on
almost nothing, so every variant moves by one token per replay: this measures what a step COSTS.
What a trained draft gets accepted on real text is not measured (no checkpoint is available).
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
from llm_sharding_amd.runtime.engine import DecodeGraph, RandomSource, StageEngine  # noqa: E402
from llm_sharding_amd.runtime.speculative import SpecDecodeGraph  # noqa: E402

DEV = "cuda:0"
MAX_SEQ = 4096
KS = (3, 7)
CONTEXTS = (128, 2048)


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


def _fmt(s: dict) -> str:
    return f"{s['median']:.3f} [{s['min']:.3f}, {s['max']:.3f}]"


def _engine(cfg, seed: int) -> StageEngine:
    return StageEngine(cfg, 0, cfg.num_hidden_layers, DEV, torch.bfloat16, has_embed=True, has_head=True,
                       source=RandomSource(cfg, seed), max_slots=1, max_seq=MAX_SEQ, max_prefill_rows=128)


def _graph_of(fn):
    """``fn`` captured on its own (warmed once)."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        fn()
    return g


def drafts_for(target_cfg) -> tuple:
    """(name -> config of the draft models to run, name -> why one was skipped)."""
    two = get_preset("llama2-7b-2l")
    run, skipped = {"2l": two}, {}
    big = get_preset("llama3.2-3b")
    if big.vocab_size == target_cfg.vocab_size:
        run["llama3.2-3b"] = big
    else:
        skipped["llama3.2-3b"] = f"vocab_size {big.vocab_size} is not the target's {target_cfg.vocab_size}"
    return run, skipped


def measure(eng: StageEngine, name: str, draft: StageEngine, rounds: int, replays: int) -> list:
    out = []
    for ctx in CONTEXTS:
        eng.seq_len[0] = ctx - 1
        hist = np.random.default_rng(ctx).integers(3, eng.cfg.vocab_size, ctx).tolist()
        plain = DecodeGraph(eng, 1, "full").capture()
        variants = {"plain": plain}
        spec = {}
        for k in KS:
            ng = SpecDecodeGraph(eng, 1, k)
            ng.admit(0, hist, MAX_SEQ - k - ctx, n_prompt=ctx)
            dm = SpecDecodeGraph(eng, 1, k, draft=draft)
            dm.admit(0, hist, MAX_SEQ - k - ctx, n_prompt=ctx)  # prefills the draft's slot
            spec[k] = (ng.capture(), dm.capture())
            variants[f"ngram k={k}"], variants[f"draft k={k}"] = ng, dm
            variants[f"dm k={k}"] = _graph_of(dm._draft_model)

        def reset():
            plain.pos.fill_(ctx - 1)
            for ng, dm in spec.values():
                for g in (ng, dm):
                    g.hlen.fill_(ctx)
                    g.done.zero_()

        times = {v: [] for v in variants}
        moved = {}  # tokens per step of the last window of every speculative graph
        for r in range(rounds + 1):  # round 0 warms every graph
            for v, g in variants.items():
                reset()
                t = _window(g.replay, replays) / replays
                if r:
                    times[v].append(t)
                if isinstance(g, SpecDecodeGraph):
                    moved[v] = float((g.hlen.item() - ctx) / replays)
        row = {"draft": name, "draft_layers": draft.n_layers, "context": ctx, "replays_per_window": replays,
               "rounds": rounds, "ms": {v: _stats(t) for v, t in times.items()}}
        med = {v: statistics.median(t) for v, t in times.items()}
        for k in KS:
            row[f"k{k}"] = {
                "break_even_tokens_per_step": med[f"draft k={k}"] / med["plain"],
                "ngram_break_even_tokens_per_step": med[f"ngram k={k}"] / med["plain"],
                "draft_share_of_step": med[f"dm k={k}"] / med[f"draft k={k}"],
                "draft_share_by_difference": (med[f"draft k={k}"] - med[f"ngram k={k}"]) / med[f"draft k={k}"],
                "tokens_per_step_in_this_run": {"ngram": moved[f"ngram k={k}"], "draft": moved[f"draft k={k}"]}}
        out.append(row)
        print(json.dumps(row), flush=True)
    return out


def markdown(meta: dict, rows: list, skipped: dict) -> str:
    L = ["# Speculative decoding with a draft model: what a step costs", "",
         f"`scripts/bench_spec_draft.py` on one MI355X (gfx950; the runtime names the device \"{meta['device']}\"), "
         f"torch {meta['torch']}, Llama-2-7B random init ({meta['layers']} layers, bf16), one sequence, `max_seq` "
         f"{MAX_SEQ}. Times are device events around windows of {meta['replays']} graph replays with no host work "
         f"inside a window; every window is warmed once, the variants alternate within each of {meta['rounds']} "
         "rounds in one process, every window restarts at the context length; ms per step, median [min, max].", "",
         "**Random-init models agree on almost nothing, so no draft is accepted here and every variant moves by "
         "one token per replay: the tables say what a step costs, not what it yields. The acceptance of a trained "
         "draft model on real text is not measured - no checkpoint is available offline.** The break-even column is "
         "the number of tokens a step must yield on average (accepted drafts + 1) for the step to match plain "
         "decode: step / plain step.", ""]
    for name, why in skipped.items():
        L += [f"Draft `{name}` was not run: {why}.", ""]
    for name in dict.fromkeys(r["draft"] for r in rows):
        mine = [r for r in rows if r["draft"] == name]
        L += [f"## Draft `{name}` ({mine[0]['draft_layers']} layers, random init, bf16)", "",
              "| context | k | plain 1-row step | n-gram step | draft-model step | its draft part alone | draft share "
              "(alone / step) | draft share (step - n-gram step) | break-even tokens per step | n-gram break-even |",
              "|---|---|---|---|---|---|---|---|---|---|"]
        for r in mine:
            for k in KS:
                m, d = r["ms"], r[f"k{k}"]
                L.append(f"| {r['context']} | {k} | {_fmt(m['plain'])} | {_fmt(m[f'ngram k={k}'])} | "
                         f"{_fmt(m[f'draft k={k}'])} | {_fmt(m[f'dm k={k}'])} | {100 * d['draft_share_of_step']:.1f} % | "
                         f"{100 * d['draft_share_by_difference']:.1f} % | {d['break_even_tokens_per_step']:.3f} | "
                         f"{d['ngram_break_even_tokens_per_step']:.3f} |")
        acc = {(r["context"], k): r[f"k{k}"]["tokens_per_step_in_this_run"] for r in mine for k in KS}
        L += ["", "Tokens per step in these windows (random init): " +
              ", ".join(f"context {c} k={k}: n-gram {a['ngram']:.2f}, draft {a['draft']:.2f}" for (c, k), a in acc.items()) + ".",
              ""]
    return "\n".join(L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--replays", type=int, default=50, help="replays per timed window")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "spec_draft_model.md"))
    ap.add_argument("--json-out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_spec_draft.py measures on the GPU: no device found")
    cfg = get_preset("llama2-7b")
    cfg.num_hidden_layers = a.layers
    run, skipped = drafts_for(cfg)
    meta = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "layers": a.layers,
            "rounds": a.rounds, "replays": a.replays, "skipped": skipped}
    print(json.dumps(meta), flush=True)
    eng = _engine(cfg, 0)
    rows = []
    for name, dcfg in run.items():
        draft = _engine(dcfg, 1)
        rows += measure(eng, name, draft, a.rounds, a.replays)
        del draft
        torch.cuda.empty_cache()
    for path, text in ((a.out, markdown(meta, rows, skipped)), (a.json_out, json.dumps({"meta": meta, "rows": rows}, indent=1))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text + "\n")


if __name__ == "__main__":
    main()
