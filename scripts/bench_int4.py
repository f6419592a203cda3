#!/usr/bin/env python3
"""int4 (W4A16) against fp8 and bf16 on one GPU, for profiles/int4.md.

--kernels: per Llama-2-7B projection shape and row count, the best int4 config against the best
  fp8 config (plain and cooperative) and, above one row, against dequantise + the bf16 decode
  kernel; every candidate is timed once, then the winners in alternating windows over weight
  copies that exceed the Infinity Cache (cold stream). Reports the median and the spread
  (max - min) / median of the windows.
--steps: ms per token of a random-init model (default llama2-7b) at batch 1 and 16, one captured
  decode graph per weight dtype, the dtypes alternated window by window in one process.
One JSON line per result; everything is also written to --out."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_kernels import EPIS, MODEL_HEADS, MODEL_SHAPES, timeit  # noqa: E402
from llm_sharding_amd.ops import hip, int4, packing  # noqa: E402

DEV = "cuda"


def _windows(fns: dict, windows: int) -> dict:
    """{name: (median us, spread)} over ``windows`` alternating windows (A B C A B C ...)."""
    t = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            t[k].append(timeit(fn))
    return {k: (statistics.median(v), (max(v) - min(v)) / statistics.median(v)) for k, v in t.items()}


def kernels(model: str, rows_list, windows: int, out: list) -> None:
    from llm_sharding_amd.config import llama2_7b
    from llm_sharding_amd.models.rope import rope_table
    cos, sin = rope_table(llama2_7b(), 1024, DEV)
    cws = hip.CoopWorkspace(DEV, slab_floats=1 << 25)
    for name, (N, K) in MODEL_SHAPES[model].items():
        epi = EPIS[name]
        if epi == hip.EPI_ARGMAX:
            continue
        w = torch.randn(N, K, device=DEV).mul_(0.02)
        nb = max(2, (600 << 20) // int4.int4_bytes(N, K) + 1)
        q4, s4 = int4.quantize_int4_groups(w)
        p4, s4 = int4.pack_b_int4(q4), int4.pack_scales_int4(s4)
        w4, sc4 = [p4.clone() for _ in range(nb)], [s4.clone() for _ in range(nb)]
        q8, s8 = packing.quantize_fp8_rows(w)
        nb8 = max(2, (600 << 20) // (N * K) + 1)
        w8 = [packing.pack_b_fp8(q8).view(-1).clone() for _ in range(nb8)]
        scratch = torch.empty(N * K, dtype=torch.bfloat16, device=DEV)
        del w, q4, q8
        even, norm = epi == hip.EPI_SWIGLU, epi in (hip.EPI_QKV, hip.EPI_SWIGLU)
        for M in rows_list:
            x = torch.randn(M, K, device=DEV).to(torch.bfloat16)
            o = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
            nh, nkv = MODEL_HEADS[model] if epi == hip.EPI_QKV else (1, 1)
            qb = torch.zeros(M, max(N, 128), dtype=torch.bfloat16, device=DEV)
            kc = torch.zeros(M, nkv, 1024, 128, dtype=torch.bfloat16, device=DEV)
            slot = torch.arange(M, dtype=torch.int32, device=DEV)
            pos = torch.full((M,), 100, dtype=torch.int32, device=DEV)
            if epi == hip.EPI_QKV:
                ep = hip.make_epi(out=qb, k_cache=kc, v_cache=kc, slot=slot, pos=pos, cos=cos, sin=sin, ldo=qb.shape[1],
                                  n_heads=nh, n_kv=nkv, head_dim=128, t_max=1024)
            else:
                ep = hip.make_epi(out=o, resid=o, ldo=N, ldr=N)

            def f4(cfg):
                return lambda i: int4.gemv_int4(x, w4[i % nb], sc4[i % nb], M, N, K, epi, ep, norm=norm, cfg=cfg)

            def f8(algo):
                return lambda i: hip.proj_fp8(x, w8[i % nb8], s8, M, N, K, epi, ep, norm=norm, algo=algo, ws=cws)

            def fdq(i):  # what the engine does above the native row limit: dequantise, then the bf16 kernel
                hip.gemv(x, int4.dequant_int4_packed(w4[i % nb], sc4[i % nb], scratch, N, K), M, N, K, epi, ep, norm=norm,
                         ws=cws)

            c4 = sorted((timeit(f4(c)), c) for c in int4.int4_gemv_candidates(N // 16, K, M, even))
            a8 = [("fp8", c) for c in packing.fp8_gemv_candidates(N // 16, K, M, even)] + \
                 [("coop_fp8", c) for c in packing.coop_fp8_candidates(N // 16, K, M)]
            c8 = sorted((timeit(f8(a)), a) for a in a8)
            auto = int4.int4_config(N // 16, M, even, K)
            fns = {"int4": f4(c4[0][1]), "fp8": f8(c8[0][1])}
            if auto != c4[0][1]:
                fns["int4_auto"] = f4(auto)
            if M > 1:
                fns["dequant+bf16"] = fdq
            r = _windows(fns, windows)
            b4, b8 = int4.int4_bytes(N, K), N * K + 4 * N
            line = {"shape": name, "N": N, "K": K, "M": M, "int4_cfg": list(c4[0][1]), "int4_auto_cfg": list(auto),
                    "fp8_algo": [c8[0][1][0], list(c8[0][1][1])],
                    "int4_us": round(r["int4"][0], 2), "int4_spread": round(r["int4"][1], 3),
                    "int4_TBps": round(b4 / r["int4"][0] / 1e6, 2),
                    "fp8_us": round(r["fp8"][0], 2), "fp8_spread": round(r["fp8"][1], 3),
                    "fp8_TBps": round(b8 / r["fp8"][0] / 1e6, 2),
                    "int4_sweep": [(round(t, 2),) + tuple(c) for t, c in c4]}
            for k in ("int4_auto", "dequant+bf16"):
                if k in r:
                    line[k + "_us"], line[k + "_spread"] = round(r[k][0], 2), round(r[k][1], 3)
            print(json.dumps(line), flush=True)
            out.append(line)
        del w4, sc4, w8, scratch
        torch.cuda.empty_cache()


def steps(model: str, batches, windows: int, n_steps: int, out: list) -> None:
    from llm_sharding_amd.config import get_preset
    from llm_sharding_amd.runtime.engine import DecodeGraph, RandomSource
    from llm_sharding_amd.runtime.engine_int4 import make_stage_engine
    cfg = get_preset(model)
    B = max(batches)
    graphs = {}
    for wd in ("bf16", "fp8", "int4"):
        e = make_stage_engine(cfg, 0, cfg.num_hidden_layers, DEV, torch.bfloat16, has_embed=True, has_head=True,
                        source=RandomSource(cfg, 0), max_slots=B, max_seq=256, max_prefill_rows=128, weight_dtype=wd)
        for s in range(B):
            e.seq_len[s] = 128
        for b in batches:
            graphs[(wd, b)] = DecodeGraph(e, b, "full", slots=list(range(b))).capture()
        print(json.dumps({"loaded": wd, "weights_GB": round(e.memory_bytes() / 1e9, 2)}), flush=True)

    def run(g):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        g.set_positions()  # every window starts from the same 128-token context
        g.replay()
        torch.cuda.synchronize()
        a.record()
        for _ in range(n_steps):
            g.replay()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n_steps

    for b in batches:
        t = {wd: [] for wd in ("bf16", "fp8", "int4")}
        for _ in range(windows):
            for wd in t:
                t[wd].append(run(graphs[(wd, b)]))
        line = {"model": model, "batch": b, "steps_per_window": n_steps, "windows": windows}
        for wd, v in t.items():
            line[wd + "_ms"] = round(statistics.median(v), 4)
            line[wd + "_spread"] = round((max(v) - min(v)) / statistics.median(v), 3)
        print(json.dumps(line), flush=True)
        out.append(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--steps", action="store_true")
    ap.add_argument("--model", default="llama2-7b")
    ap.add_argument("--rows", default="1,16,64")
    ap.add_argument("--batches", default="1,16")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--n-steps", type=int, default=64)
    ap.add_argument("--out", default="bench_int4.json")
    a = ap.parse_args()
    hip.lib()
    out = []
    if a.kernels:
        kernels(a.model, [int(r) for r in a.rows.split(",")], a.windows, out)
    if a.steps:
        steps(a.model, [int(b) for b in a.batches.split(",")], a.windows, a.n_steps, out)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
