#!/usr/bin/env python3
"""Sweep gemm_skp's plans (bm x bn x contributors 2..8 x both placements) for the residual
projections, with the epilogue the engine runs (EPI_RESID + the fused-norm ss_out partials) and
weights rotated over > 600 MB of copies so they stream from HBM as in a decode step - the same
sweep as scripts/tune_gemm_sk.py. gemm_sk's product plan of the shape is timed beside them.

One JSON line per (shape, M) on stdout with every candidate's time, and the line the winner would
have in llm_sharding_amd/ops/skp_tuning.txt. Nothing is written to the table: a plan is adopted
only after an engine A/B run of the whole step (LSA_GEMM_SKP=0 / 1, LSA_GEMM_SKP_TUNING=<table>),
since isolation wins on these two projections have vanished inside the step before.

usage: tune_gemm_skp.py [--rows 512] [--models llama2-7b,llama2-70b] [--iters N]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from llm_sharding_amd.ops import gemm_skp, hip, packing  # noqa: E402
from scripts.bench_kernels import MODEL_SHAPES  # noqa: E402
from scripts.tune_gemm_sk import timeit  # noqa: E402

DEV = "cuda"
RESIDUAL = ("o", "down")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="512")
    ap.add_argument("--models", default="llama2-7b")
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    sk_ws = hip.SkWorkspace(DEV)
    for model in a.models.split(","):
        for name, (N, K) in MODEL_SHAPES[model].items():
            if name not in RESIDUAL:
                continue
            nbuf = max(2, (600 << 20) // (N * K * 2) + 1)
            ws = [packing.pack_b(torch.randn(N, K, device=DEV).mul_(0.02).to(torch.bfloat16)) for _ in range(nbuf)]
            for M in (int(r) for r in a.rows.split(",")):
                x = torch.randn(M, K, device=DEV).to(torch.bfloat16)
                out = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
                ss = torch.zeros(M, N // 64, dtype=torch.float32, device=DEV)
                ep = hip.make_epi(out=out, resid=out, ldo=N, ldr=N, ss_out=ss)
                sk_us = round(timeit(lambda i: hip.gemm_sk(x, ws[i % nbuf], M, N, K, hip.EPI_RESID, ep, ws=sk_ws), a.iters), 2)
                res = []
                for bm in (256, 128):
                    for bn in (256, 128):
                        for C in range(2, gemm_skp.MAX_CONTRIBUTORS + 1):
                            if gemm_skp.check_plan(M, N, K, bm, bn, C) or gemm_skp.tiles(M, N, bm, bn) * C > hip.N_CU:
                                continue  # one workgroup per CU: more than 256 would run in two waves
                            if sk_ws.slab.numel() < gemm_skp.slab_floats(M, N, bm, bn, C) or \
                                    sk_ws.counters.numel() < gemm_skp.n_counters(M, N, bm, bn):
                                continue
                            for tm in (0, 1):
                                us = timeit(lambda i: gemm_skp.gemm_skp(x, ws[i % nbuf], M, N, K, hip.EPI_RESID, ep, bm=bm, bn=bn,
                                                                        contributors=C, tile_major=tm, ws=sk_ws), a.iters)
                                res.append((round(us, 2), bm, bn, C, tm))
                res.sort()
                best = res[0] if res else None
                print(json.dumps({"model": model, "shape": name, "N": N, "K": K, "M": M, "gemm_sk_plan": hip.gemm_sk_plan(M, N, K),
                                  "gemm_sk_us": sk_us, "best_us": best and best[0],
                                  "table_line": best and f"{M} {N} {K} {best[1]} {best[2]} {best[3]} {best[4]}",
                                  "all": res}), flush=True)
            del ws
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
