#!/usr/bin/env python3
"""mxfp4 (W4A8) against int4, fp8 and bf16 on one GPU, for profiles/mx4.md.

--kernels: per Llama-2-7B projection shape and row count, the mxfp4 kernel at the chooser's config
  (and at the fastest of all candidates, each timed once first) against int4.proj_int4, hip.proj_fp8
  and dequantise + the bf16 decode kernel, in alternating windows over weight copies that exceed
  the Infinity Cache (cold stream). Reports the median and the spread (max - min) / median.
--steps: ms per token of a random-init model (default llama2-7b, optionally the first --layers
  layers) at batch 1, 16, 64 and 128, one captured decode graph per weight dtype, the dtypes
  alternated window by window in one process.
--gemm: the W4A8 GEMM (csrc/quant/gemm_mx4.hip) at 256 .. 2048 rows: the pre-pass alone, pre-pass +
  GEMM at every built config, dequantise + hip.gemm and hip.gemm on bf16 weights, with TFLOP/s.
--gemm-step: a captured 512-row decode step of --layers layers and one 2048-token prefill,
  LSA_MX4_GEMM=1 against =0, one engine each, alternated window by window.
One JSON line per result; everything is also written to --out."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_int4 import _windows  # noqa: E402
from bench_kernels import EPIS, MODEL_HEADS, MODEL_SHAPES, timeit  # noqa: E402
from llm_sharding_amd.ops import hip, int4, mx4, packing  # noqa: E402

DEV = "cuda"
DTYPES = ("bf16", "fp8", "int4", "mxfp4")


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
        nb = max(2, (600 << 20) // mx4.mx4_bytes(N, K) + 1)
        qm, em = mx4.quantize_mx4(w)
        pm, sm = mx4.pack_b_mx4(qm), mx4.pack_scales_mx4(em)
        wm, scm = [pm.clone() for _ in range(nb)], [sm.clone() for _ in range(nb)]
        q4, s4 = int4.quantize_int4_groups(w)
        p4, s4 = int4.pack_b_int4(q4), int4.pack_scales_int4(s4)
        w4, sc4 = [p4.clone() for _ in range(nb)], [s4.clone() for _ in range(nb)]
        q8, s8 = packing.quantize_fp8_rows(w)
        nb8 = max(2, (600 << 20) // (N * K) + 1)
        w8 = [packing.pack_b_fp8(q8).view(-1).clone() for _ in range(nb8)]
        scratch = torch.empty(N * K, dtype=torch.bfloat16, device=DEV)
        del w, qm, q4, q8
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

            def fm(cfg):
                return lambda i: mx4.gemv_mx4(x, wm[i % nb], scm[i % nb], M, N, K, epi, ep, norm=norm, ws=cws, cfg=cfg)

            def fdq(i):  # the engine's route above 128 rows: dequantise, then the bf16 kernel
                hip.gemv(x, mx4.dequant_mx4_packed(wm[i % nb], scm[i % nb], scratch, N, K), M, N, K, epi, ep, norm=norm, ws=cws)

            cands = [c for c in mx4.mx4_candidates(N // 16, K, M, even)
                     if mx4.mx4_slab_floats(N // 16, M, *c) <= cws.slab.numel()]
            sweep = sorted((timeit(fm(c)), c) for c in cands)
            auto = mx4.mx4_config(N // 16, K, M, even, cws.slab.numel(), cws.counters.numel())
            fns = {"mx4_auto": fm(auto), "mx4_best": fm(sweep[0][1]),
                   "int4": lambda i: int4.proj_int4(x, w4[i % nb], sc4[i % nb], M, N, K, epi, ep, norm=norm, ws=cws),
                   "fp8": lambda i: hip.proj_fp8(x, w8[i % nb8], s8, M, N, K, epi, ep, norm=norm, ws=cws),
                   "dequant+bf16": fdq}
            r = _windows(fns, windows)
            line = {"shape": name, "N": N, "K": K, "M": M, "mx4_auto_cfg": list(auto), "mx4_best_cfg": list(sweep[0][1]),
                    "mx4_best_TBps": round(mx4.mx4_bytes(N, K) / r["mx4_best"][0] / 1e6, 2),
                    "mx4_sweep": [(round(t, 2),) + tuple(c) for t, c in sweep[:6]]}
            for k, (us, spread) in r.items():
                line[k + "_us"], line[k + "_spread"] = round(us, 2), round(spread, 3)
            print(json.dumps(line), flush=True)
            out.append(line)
        del wm, scm, w4, sc4, w8, scratch
        torch.cuda.empty_cache()


def steps(model: str, batches, windows: int, n_steps: int, layers: int, out: list) -> None:
    from llm_sharding_amd.config import get_preset
    from llm_sharding_amd.runtime.engine import DecodeGraph, RandomSource
    from llm_sharding_amd.runtime.engine_int4 import make_stage_engine
    cfg = get_preset(model)
    L = layers or cfg.num_hidden_layers
    B = max(batches)
    graphs = {}
    for wd in DTYPES:
        e = make_stage_engine(cfg, 0, L, DEV, torch.bfloat16, has_embed=True, has_head=True, source=RandomSource(cfg, 0),
                              max_slots=B, max_seq=256, max_prefill_rows=128, weight_dtype=wd)
        for s in range(B):
            e.seq_len[s] = 128
        for b in batches:
            graphs[(wd, b)] = DecodeGraph(e, b, "full", slots=list(range(b))).capture()
        print(json.dumps({"loaded": wd, "layers": L, "weights_GB": round(e.memory_bytes() / 1e9, 2)}), flush=True)

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
        t = {wd: [] for wd in DTYPES}
        for _ in range(windows):
            for wd in t:
                t[wd].append(run(graphs[(wd, b)]))
        line = {"model": model, "layers": L, "batch": b, "steps_per_window": n_steps, "windows": windows}
        for wd, v in t.items():
            line[wd + "_ms"] = round(statistics.median(v), 4)
            line[wd + "_spread"] = round((max(v) - min(v)) / statistics.median(v), 3)
        print(json.dumps(line), flush=True)
        out.append(line)


def gemm(model: str, rows_list, windows: int, out: list) -> None:
    """Per projection shape and row count (STORE epilogue): the pre-pass alone, pre-pass + gemm_mx4
    at every built config against the chooser's, dequantise + hip.gemm (the default route) and
    hip.gemm on bf16 weights; TFLOP/s = 2 M N K / time."""
    cws, sk = hip.CoopWorkspace(DEV, slab_floats=1 << 27), hip.SkWorkspace(DEV)
    for name, (N, K) in MODEL_SHAPES[model].items():
        if EPIS[name] == hip.EPI_ARGMAX:
            continue
        w = torch.randn(N, K, device=DEV).mul_(0.02)
        qm, em = mx4.quantize_mx4(w)
        wm, scm = mx4.pack_b_mx4(qm), mx4.pack_scales_mx4(em)
        wb = packing.pack_b(w.to(torch.bfloat16))
        scratch = torch.empty(N * K, dtype=torch.bfloat16, device=DEV)
        del w, qm
        for M in rows_list:
            x = torch.randn(M, K, device=DEV).to(torch.bfloat16)
            o = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
            ep, epi = hip.make_epi(out=o, ldo=N), hip.EPI_STORE
            img = torch.empty(sum(mx4.a_image_bytes(M, K)), dtype=torch.uint8, device=DEV)

            def fg(cfg):
                return lambda i: mx4.gemm_mx4(*mx4.quant_act_mx8(x, M, K, img), wm, scm, M, N, K, epi, ep, ws=cws, cfg=cfg)

            cands = [c for c in mx4.mx4_gemm_candidates(M, N, K, epi) if mx4.mx4_gemm_slab_floats(M, N, c[1]) <= cws.slab.numel()]
            auto = mx4.mx4_gemm_config(M, N, K, epi, cws.slab.numel(), cws.counters.numel())
            fns = {f"mx4_bn{c[0]}_sk{c[1]}": fg(c) for c in cands}
            fns.update({"prepass": lambda i: mx4.quant_act_mx8(x, M, K, img),
                        "dequant+bf16": lambda i: hip.gemm(x, mx4.dequant_mx4_packed(wm, scm, scratch, N, K), M, N, K, epi, ep,
                                                           ws=cws, sk_ws=sk),
                        "bf16": lambda i: hip.gemm(x, wb, M, N, K, epi, ep, ws=cws, sk_ws=sk)})
            r = _windows(fns, windows)
            line = {"table": "gemm", "shape": name, "N": N, "K": K, "M": M, "auto_cfg": list(auto)}
            for k, (us, spread) in r.items():
                line[k + "_us"], line[k + "_spread"] = round(us, 2), round(spread, 3)
                if k != "prepass":
                    line[k + "_TFLOPs"] = round(2.0 * M * N * K / us / 1e6, 1)
            print(json.dumps(line), flush=True)
            out.append(line)
        del wm, scm, wb, scratch
        torch.cuda.empty_cache()


def gemm_step(model: str, layers: int, rows: int, prefill: int, windows: int, n_steps: int, out: list) -> None:
    """LSA_MX4_GEMM=1 against =0, one engine each, alternated window by window: a captured
    ``rows``-row decode step and one eager ``prefill``-token prefill forward."""
    from llm_sharding_amd.config import get_preset
    from llm_sharding_amd.runtime.engine import DecodeGraph, RandomSource
    from llm_sharding_amd.runtime.engine_int4 import make_stage_engine
    cfg = get_preset(model)
    graphs, engines = {}, {}
    for flag in ("1", "0"):  # the switch is read when the engine allocates and when the graph is captured
        os.environ["LSA_MX4_GEMM"] = flag
        e = make_stage_engine(cfg, 0, layers, DEV, torch.bfloat16, has_embed=True, has_head=True, source=RandomSource(cfg, 0),
                              max_slots=rows, max_seq=max(256, prefill), max_prefill_rows=max(rows, prefill),
                              weight_dtype="mxfp4")
        for s in range(rows):
            e.seq_len[s] = 128
        graphs[flag], engines[flag] = DecodeGraph(e, rows, "full", slots=list(range(rows))).capture(), e
    toks = torch.randint(3, cfg.vocab_size - 1, (prefill,), device=DEV)

    def run_step(flag):
        g = graphs[flag]
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

    def run_prefill(flag):
        e = engines[flag]
        os.environ["LSA_MX4_GEMM"] = flag
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e.seq_len[0] = 0
        sl, po = e.prefill_rows([0], [prefill])
        h = e.embed(toks)
        torch.cuda.synchronize()
        a.record()
        e.forward(h, sl, po)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    for table, fn in (("gemm_step", run_step), ("gemm_prefill", run_prefill)):
        t = {f: [] for f in graphs}
        for _ in range(windows + 1):  # the first window warms up
            for f in graphs:
                t[f].append(fn(f))
        line = {"table": table, "model": model, "layers": layers, "rows": rows if table == "gemm_step" else prefill,
                "windows": windows}
        for f, name in (("1", "native"), ("0", "dequant")):
            v = t[f][1:]
            line[name + "_ms"] = round(statistics.median(v), 4)
            line[name + "_spread"] = round((max(v) - min(v)) / statistics.median(v), 3)
        print(json.dumps(line), flush=True)
        out.append(line)
    del os.environ["LSA_MX4_GEMM"]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--steps", action="store_true")
    ap.add_argument("--gemm", action="store_true", help="the W4A8 GEMM's table (256..2048 rows)")
    ap.add_argument("--gemm-step", action="store_true", help="a 512-row decode step and a 2048-token prefill, LSA_MX4_GEMM=1 / 0")
    ap.add_argument("--gemm-rows", default="256,512,1024,2048")
    ap.add_argument("--model", default="llama2-7b")
    ap.add_argument("--layers", type=int, default=0, help="--steps: only the first N layers (0: all)")
    ap.add_argument("--rows", default="1,16,32,64,128")
    ap.add_argument("--batches", default="1,16,64,128")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--n-steps", type=int, default=50)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    hip.lib()
    out = []
    if a.kernels:
        kernels(a.model, [int(r) for r in a.rows.split(",")], a.windows, out)
    if a.steps:
        steps(a.model, [int(b) for b in a.batches.split(",")], a.windows, a.n_steps, a.layers, out)
    if a.gemm:
        gemm(a.model, [int(r) for r in a.gemm_rows.split(",")], a.windows, out)
    if a.gemm_step:
        gemm_step(a.model, a.layers or 4, 512, 2048, a.windows, a.n_steps, out)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
