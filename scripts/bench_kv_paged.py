#!/usr/bin/env python3
"""Paged KV cache against the static cache on one GPU, for profiles/kv_paged.md.

--kernels: lsa_attn_decode_paged against lsa_attn_decode at the Llama-2-7B shape (32 heads, hd 128) for rows x
  context 512 x 143, 512 x 2048, 128 x 2048 and 1 x 2048, with the split count the engine picks; pages in
  allocation order and shuffled over the pool. A batch-1 window is one graph of 512 launches over 512 distinct
  slots (beyond the 256 MB Infinity Cache), so that every launch streams cold K/V; the larger shapes stream
  1 GB or more per launch. lsa_kvp_append at 1 / 128 / 512 rows, lsa_kvp_gather of a 2048-token prefix.
  Alternating windows in one process; median and (max - min) / median.
--steps: ms per decode step of random-init llama2-7b at 512 sequences and at batch 1, one captured decode
  graph per layout on ~143 tokens of context, the two alternated window by window.
--serve: serve.py's load test (child processes, one after the other) at max_seq 4096 with 128 + 128-token
  requests, two micro-batches: the static cache at 2 x 61 slots (what ``--batch 0`` sizes for a 288 GB
  device), the paged cache at 2 x 256 slots with ``--kv-pages 0``; tokens/s, p50 TPOT and the peak of requests
  in flight.
One JSON line per result; everything is also written to --out."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_kernels import timeit  # noqa: E402
from llm_sharding_amd.ops import hip, kv_paged  # noqa: E402

DEV = "cuda"
NH, NKV, HD = 32, 32, 128
PAGE = kv_paged.PAGE


def _windows(fns: dict, windows: int, reps: int = 20) -> dict:
    t = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            t[k].append(timeit(fn, reps=reps))
    return {k: (statistics.median(v), (max(v) - min(v)) / statistics.median(v)) for k, v in t.items()}


def _fill(t: torch.Tensor) -> None:
    """Fill a large tensor block by block from one generated block."""
    one = torch.randn(t[0].shape, device=DEV).to(torch.bfloat16)
    for s in range(t.shape[0]):
        t[s].copy_(one)


def _tables(slots: int, ppn: int) -> dict:
    """Block tables over a pool of slots * ppn + 1 pages: in allocation order (slot after slot) and
    shuffled over the whole pool."""
    n = slots * ppn
    order = torch.arange(1, n + 1, dtype=torch.int32).view(slots, ppn)
    g = torch.Generator().manual_seed(0)
    shuf = (torch.randperm(n, generator=g) + 1).to(torch.int32).view(slots, ppn)
    return {"order": order.to(DEV), "shuffled": shuf.to(DEV)}


def kernels(windows: int, out: list) -> None:
    for rows, ctx in ((512, 143), (512, 2048), (128, 2048), (1, 2048)):
        T = -(-(ctx + 1) // PAGE) * PAGE
        slots = rows if rows > 1 else 512  # batch 1: one launch per slot and graph, see above
        kc = torch.empty(slots, NKV, T, HD, dtype=torch.bfloat16, device=DEV)
        vc = torch.empty_like(kc)
        _fill(kc)
        _fill(vc)
        n_pages = slots * (T // PAGE) + 1
        kp = torch.empty(n_pages, NKV, PAGE, HD, dtype=torch.bfloat16, device=DEV)
        vp = torch.empty_like(kp)
        _fill(kp)
        _fill(vp)
        tabs = _tables(slots, T // PAGE)
        q = torch.randn(rows, NH * HD, device=DEV).to(torch.bfloat16)
        o = torch.zeros(rows, NH * HD, dtype=torch.bfloat16, device=DEV)
        nsplit = int(max(1, min(min(16, -(-T // 256)), -(-512 // (rows * NKV)))))
        po = torch.zeros(rows * NH * nsplit * HD, device=DEV)
        pl = torch.zeros(rows * NH * nsplit, device=DEV)
        cnt = torch.zeros(rows * NKV, dtype=torch.int32, device=DEV)
        pos = torch.full((rows,), ctx - 1, dtype=torch.int32, device=DEV)
        sl = [torch.arange(rows, dtype=torch.int32, device=DEV)] if rows > 1 else \
            [torch.tensor([i], dtype=torch.int32, device=DEV) for i in range(slots)]

        def static(i):
            hip.attn(q, kc, vc, sl[i % len(sl)], pos, rows, NH, NKV, HD, nsplit, po, pl, o, counters=cnt, min_chunk=256)

        def paged(tab):
            def f(i):
                kv_paged.attn_paged(q, kp, vp, tab, sl[i % len(sl)], pos, rows, NH, NKV, HD, nsplit, po, pl, o,
                                    counters=cnt, min_chunk=256)
            return f
        fns = {"static": static}
        for name, tab in tabs.items():
            fns[f"paged_{name}"] = paged(tab)
        r = _windows(fns, windows, reps=20 if rows > 1 else slots)
        nbytes = rows * NKV * ctx * 2 * HD * 2
        line = {"kind": "attn", "rows": rows, "context": ctx, "nsplit": nsplit, "bytes": nbytes, "windows": windows}
        for k, (us, spread) in r.items():
            line[k + "_us"], line[k + "_spread"] = round(us, 2), round(spread, 3)
            line[k + "_TBps"] = round(nbytes / us / 1e6, 3)
            if k != "static":
                line[k + "_vs_static"] = round(us / r["static"][0], 4)
        print(json.dumps(line), flush=True)
        out.append(line)
        if rows == 512 and ctx == 143:  # the append at the headline shape's cache
            for m in (1, 128, 512):
                slot = torch.arange(m, dtype=torch.int32, device=DEV)
                ps = [torch.full((m,), (7 * i) % ctx, dtype=torch.int32, device=DEV) for i in range(20)]
                r = _windows({"append": lambda i: kv_paged.kvp_append(kc, vc, kp, vp, tabs["shuffled"], slot, ps[i % 20], m)},
                             windows)
                line = {"kind": "append", "rows": m, "n_kv": NKV, "hd": HD, "append_us": round(r["append"][0], 2),
                        "append_spread": round(r["append"][1], 3)}
                print(json.dumps(line), flush=True)
                out.append(line)
        if rows == 128 and ctx == 2048:  # a chunked prefill's restore: one 2048-token prefix, and 16 of them
            for jobs in (1, 16):
                jl = [(s, 2048) for s in range(jobs)]
                r = _windows({"gather": lambda i: kv_paged.kvp_gather(kp, vp, tabs["shuffled"], kc, vc, jl)}, windows)
                gb = jobs * NKV * 2048 * HD * 2 * 2 * 2  # K and V, read and written
                line = {"kind": "gather", "jobs": jobs, "prefix": 2048, "gather_us": round(r["gather"][0], 2),
                        "gather_spread": round(r["gather"][1], 3), "TBps_read_plus_write": round(gb / r["gather"][0] / 1e6, 3)}
                print(json.dumps(line), flush=True)
                out.append(line)
        del kc, vc, kp, vp
        torch.cuda.empty_cache()


def _engine(cfg, layout, slots, max_seq, rows):
    from llm_sharding_amd.runtime.engine import RandomSource
    from llm_sharding_amd.runtime.engine_int4 import make_stage_engine
    return make_stage_engine(cfg, 0, cfg.num_hidden_layers, DEV, torch.bfloat16, has_embed=True, has_head=True,
                             source=RandomSource(cfg, 0), max_slots=slots, max_seq=max_seq, max_prefill_rows=rows,
                             kv_layout=layout, kv_pages=slots * (max_seq // PAGE) + 1 if layout == "paged" else None)


def steps(model: str, batches, windows: int, n_steps: int, ctx: int, out: list) -> None:
    from llm_sharding_amd.config import get_preset
    from llm_sharding_amd.runtime.engine import DecodeGraph
    cfg = get_preset(model)
    B = max(batches)
    graphs = {}
    max_seq = -(-(ctx + n_steps + 2) // PAGE) * PAGE
    for layout in ("static", "paged"):
        e = _engine(cfg, layout, B, max_seq, max(B, 128))
        if layout == "paged":  # shuffled pages, every slot reserved to the end of the timed window
            g = torch.Generator().manual_seed(0)
            free = e.pool._free
            e.pool._free = [free[i] for i in torch.randperm(len(free), generator=g).tolist()]
            for s in range(B):
                e.kv_reserve(s, max_seq)
        for s in range(B):
            e.seq_len[s] = ctx - n_steps // 2  # the timed steps straddle the context length
        for b in batches:
            graphs[(layout, b)] = DecodeGraph(e, b, "full", slots=list(range(b))).capture()
        print(json.dumps({"loaded": layout, "engine": type(e).__name__,
                          "weights_plus_kv_GB": round(e.memory_bytes() / 1e9, 2)}), flush=True)

    def run(g):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        g.set_positions()
        g.replay()
        torch.cuda.synchronize()
        a.record()
        for _ in range(n_steps):
            g.replay()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n_steps

    for b in batches:
        t = {layout: [] for layout in ("static", "paged")}
        for _ in range(windows):
            for layout in t:
                t[layout].append(run(graphs[(layout, b)]))
        line = {"kind": "step", "model": model, "batch": b, "context": ctx, "steps_per_window": n_steps, "windows": windows}
        for layout, v in t.items():
            line[layout + "_ms"] = round(statistics.median(v), 4)
            line[layout + "_spread"] = round((max(v) - min(v)) / statistics.median(v), 3)
        line["paged_vs_static"] = round(line["paged_ms"] / line["static_ms"], 4)
        print(json.dumps(line), flush=True)
        out.append(line)


def serve(model: str, requests: int, timeout_s: int, out: list) -> None:
    base = [sys.executable, os.path.join(ROOT, "serve.py"), "--model", model, "--max-seq", "4096", "--requests",
            str(requests), "--prompt-len", "128", "--max-new-tokens", "128", "--microbatches", "2"]
    for name, extra in (("static", ["--batch", "61"]),
                        ("paged", ["--batch", "256", "--kv-layout", "paged", "--kv-pages", "0"])):
        r = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout_s)
        res = next((json.loads(ln) for ln in reversed(r.stdout.splitlines()) if ln.startswith("{")), None)
        line = {"kind": "serve", "layout": name, "rc": r.returncode, "argv": extra}
        if res is None:
            line["tail"] = r.stdout[-2000:]
        else:
            line.update({k: res.get(k) for k in ("tok_s", "tpot_ms_p50", "tpot_ms_p90", "ttft_ms_p50", "peak_in_flight",
                                                 "slots", "microbatches", "kv_pages", "requests", "tokens", "elapsed_s")})
        print(json.dumps(line), flush=True)
        out.append(line)
        if r.returncode != 0:  # start nothing more on the GPU after a failed run
            break


def main():
    ap = argparse.ArgumentParser()
    for flag in ("--kernels", "--steps", "--serve"):
        ap.add_argument(flag, action="store_true")
    ap.add_argument("--model", default="llama2-7b")
    ap.add_argument("--batches", default="512,1")
    ap.add_argument("--context", type=int, default=143)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--n-steps", type=int, default=32)
    ap.add_argument("--requests", type=int, default=1024)
    ap.add_argument("--serve-timeout", type=int, default=400)
    ap.add_argument("--out", default="bench_kv_paged.json")
    a = ap.parse_args()
    hip.lib()
    out = []
    if a.kernels:
        kernels(a.windows, out)
    if a.steps:
        steps(a.model, [int(b) for b in a.batches.split(",")], a.windows, a.n_steps, a.context, out)
    if a.serve:
        serve(a.model, a.requests, a.serve_timeout, out)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
