#!/usr/bin/env python3
"""FP8 KV cache against the bf16 cache on one GPU, for profiles/kv8.md.

--kernels: lsa_attn_decode_kv8 against lsa_attn_decode at the Llama-2-7B shape (32 heads, hd 128) for rows x context
  512 x 143, 512 x 2048, 128 x 2048, 1 x 128 and 1 x 2048, with the split count the engine picks;
  a batch-1 window is one graph of 512 launches over 512 distinct slots (0.5 GB of codes or more per
  replay, beyond the 256 MB Infinity Cache), so that every launch streams cold K/V. lsa_kv8_append at
  1, 128 and 512 rows. Alternating windows in one process; median and (max - min) / median.
--steps: ms per decode step of random-init llama2-7b at 512 sequences and at batch 1, one captured
  decode graph per kv_dtype on ~143 tokens of context, the two alternated window by window.
--bench: run_decode_benchmark(kv_dtype=...) once per dtype at 512 sequences with its batch-1 latency
  pass (the public path, end to end: PipelineStage, prefill, captured decode).
--quality: logits rel_err and greedy-token agreement over 64 teacher-forced steps, the fp8-KV engine
  against the bf16 engine on the same random-init weights; the same two figures for fp8 WEIGHTS
  (bf16 KV) as a yardstick of what a random-init 32-layer model does to a small perturbation.
One JSON line per result; everything is also written to --out."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_kernels import timeit  # noqa: E402
from llm_sharding_amd.ops import hip, kv8, packing  # noqa: E402

DEV = "cuda"
NH, NKV, HD = 32, 32, 128


def _windows(fns: dict, windows: int, reps: int = 20) -> dict:
    t = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            t[k].append(timeit(fn, reps=reps))
    return {k: (statistics.median(v), (max(v) - min(v)) / statistics.median(v)) for k, v in t.items()}


def _fill(t: torch.Tensor, make) -> None:
    """Fill a large cache tensor slot by slot from one generated slot."""
    one = make(t[0].shape)
    for s in range(t.shape[0]):
        t[s].copy_(one)


def kernels(windows: int, out: list) -> None:
    for rows, ctx in ((512, 143), (512, 2048), (128, 2048), (1, 128), (1, 2048)):
        T = -(-(ctx + 1) // 64) * 64
        slots = rows if rows > 1 else 512  # batch 1: one launch per slot and graph, see above
        kc = torch.empty(slots, NKV, T, HD, dtype=torch.bfloat16, device=DEV)
        vc = torch.empty_like(kc)
        _fill(kc, lambda sh: torch.randn(sh, device=DEV).to(torch.bfloat16))
        _fill(vc, lambda sh: torch.randn(sh, device=DEV).to(torch.bfloat16))
        k8 = torch.empty(slots, NKV, T, HD, dtype=torch.uint8, device=DEV)
        v8 = torch.empty_like(k8)
        ks = torch.full((slots, NKV, T), 2.0 ** -6, device=DEV)
        vs = torch.full((slots, NKV, T), 2.0 ** -6, device=DEV)
        # finite codes of both signs up to 240 (no NaN code): the timing does not depend on the values
        _fill(k8, lambda sh: torch.randint(0, 0x78, sh, device=DEV, dtype=torch.uint8) | (torch.randint(0, 2, sh, device=DEV, dtype=torch.uint8) << 7))
        _fill(v8, lambda sh: torch.randint(0, 0x78, sh, device=DEV, dtype=torch.uint8) | (torch.randint(0, 2, sh, device=DEV, dtype=torch.uint8) << 7))
        q = torch.randn(rows, NH * HD, device=DEV).to(torch.bfloat16)
        o = torch.zeros(rows, NH * HD, dtype=torch.bfloat16, device=DEV)
        nsplit = int(max(1, min(min(16, -(-T // 256)), -(-512 // (rows * NKV)))))
        po = torch.zeros(rows * NH * nsplit * HD, device=DEV)
        pl = torch.zeros(rows * NH * nsplit, device=DEV)
        cnt = torch.zeros(rows * NKV, dtype=torch.int32, device=DEV)
        pos = torch.full((rows,), ctx - 1, dtype=torch.int32, device=DEV)
        sl = [torch.arange(rows, dtype=torch.int32, device=DEV)] if rows > 1 else \
            [torch.tensor([i], dtype=torch.int32, device=DEV) for i in range(slots)]

        def f16(i):
            hip.attn(q, kc, vc, sl[i % len(sl)], pos, rows, NH, NKV, HD, nsplit, po, pl, o, counters=cnt, min_chunk=256)

        def f8(i):
            kv8.attn_kv8(q, k8, v8, ks, vs, sl[i % len(sl)], pos, rows, NH, NKV, HD, nsplit, po, pl, o, counters=cnt,
                         min_chunk=256)
        r = _windows({"bf16": f16, "kv8": f8}, windows, reps=20 if rows > 1 else slots)
        b16 = rows * NKV * ctx * 2 * HD * 2
        b8 = rows * NKV * ctx * (2 * HD + 8)
        line = {"kind": "attn", "rows": rows, "context": ctx, "nsplit": nsplit, "bytes_bf16": b16, "bytes_kv8": b8,
                "windows": windows}
        for k, (us, spread) in r.items():
            line[k + "_us"], line[k + "_spread"] = round(us, 2), round(spread, 3)
            line[k + "_TBps"] = round((b16 if k == "bf16" else b8) / us / 1e6, 3)
        line["ratio"] = round(r["bf16"][0] / r["kv8"][0], 3)
        print(json.dumps(line), flush=True)
        out.append(line)
        if rows == 512 and ctx == 143:  # the append at the headline shape's cache
            for m in (1, 128, 512):
                slot = torch.arange(m, dtype=torch.int32, device=DEV)
                ps = [torch.full((m,), (7 * i) % ctx, dtype=torch.int32, device=DEV) for i in range(20)]
                r = _windows({"append": lambda i: kv8.kv8_append(kc, vc, k8, v8, ks, vs, slot, ps[i % 20], m)}, windows)
                line = {"kind": "append", "rows": m, "n_kv": NKV, "hd": HD, "append_us": round(r["append"][0], 2),
                        "append_spread": round(r["append"][1], 3)}
                print(json.dumps(line), flush=True)
                out.append(line)
        del kc, vc, k8, v8, ks, vs
        torch.cuda.empty_cache()


def _engine(cfg, kvd, slots, max_seq, rows):
    from llm_sharding_amd.runtime.engine import RandomSource
    from llm_sharding_amd.runtime.engine_int4 import make_stage_engine
    return make_stage_engine(cfg, 0, cfg.num_hidden_layers, DEV, torch.bfloat16, has_embed=True, has_head=True,
                             source=RandomSource(cfg, 0), max_slots=slots, max_seq=max_seq, max_prefill_rows=rows,
                             kv_dtype=kvd)


def steps(model: str, batches, windows: int, n_steps: int, ctx: int, out: list) -> None:
    from llm_sharding_amd.config import get_preset
    from llm_sharding_amd.runtime.engine import DecodeGraph
    cfg = get_preset(model)
    B = max(batches)
    graphs = {}
    for kvd in ("bf16", "fp8"):
        e = _engine(cfg, kvd, B, -(-(ctx + n_steps + 2) // 64) * 64, max(B, 128))
        for s in range(B):
            e.seq_len[s] = ctx - n_steps // 2  # the timed steps straddle the context length
        for b in batches:
            graphs[(kvd, b)] = DecodeGraph(e, b, "full", slots=list(range(b))).capture()
        print(json.dumps({"loaded": kvd, "weights_plus_kv_GB": round(e.memory_bytes() / 1e9, 2)}), flush=True)

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
        t = {kvd: [] for kvd in ("bf16", "fp8")}
        for _ in range(windows):
            for kvd in t:
                t[kvd].append(run(graphs[(kvd, b)]))
        line = {"kind": "step", "model": model, "batch": b, "context": ctx, "steps_per_window": n_steps, "windows": windows}
        for kvd, v in t.items():
            line[kvd + "_ms"] = round(statistics.median(v), 4)
            line[kvd + "_spread"] = round((max(v) - min(v)) / statistics.median(v), 3)
        line["ratio"] = round(line["bf16_ms"] / line["fp8_ms"], 3)
        print(json.dumps(line), flush=True)
        out.append(line)


def bench(model: str, batch: int, n_steps: int, out: list) -> None:
    from llm_sharding_amd.parallel.pipeline import run_decode_benchmark
    for kvd in ("bf16", "fp8"):
        r = run_decode_benchmark(model=model, n_gpus=1, steps=n_steps, warmup=4, batch=batch, prompt_len=128,
                                 verbose=False, kv_dtype=kvd, latency_steps=n_steps)
        line = {"kind": "run_decode_benchmark", "model": model, "batch": batch, "kv_dtype": kvd}
        line.update({k: v for k, v in (r or {}).items() if isinstance(v, (int, float, str))})
        print(json.dumps(line), flush=True)
        out.append(line)
        torch.cuda.empty_cache()


def quality(model: str, out: list, n_seq: int = 4, prompt: int = 128, n_steps: int = 64) -> None:
    from llm_sharding_amd.config import get_preset
    from llm_sharding_amd.runtime.engine import RandomSource
    from llm_sharding_amd.runtime.engine_int4 import make_stage_engine
    from llm_sharding_amd.utils.numerics import rel_err
    cfg = get_preset(model)
    kw = dict(has_embed=True, has_head=True, max_slots=n_seq, max_seq=256, max_prefill_rows=n_seq * prompt)
    engs = {"bf16": _engine(cfg, "bf16", n_seq, 256, n_seq * prompt), "kv_fp8": _engine(cfg, "fp8", n_seq, 256, n_seq * prompt),
            "weights_fp8": make_stage_engine(cfg, 0, cfg.num_hidden_layers, DEV, torch.bfloat16, source=RandomSource(cfg, 0),
                                             weight_dtype="fp8", **kw)}
    lm = packing.unpack_b(engs["bf16"].lm_head).float()  # (the final norm's weight is folded in)

    def logits(h):
        x = h.float()
        return (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + cfg.rms_norm_eps)) @ lm.t()
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(3, cfg.vocab_size, (n_seq * prompt,), generator=g).to(DEV)
    sl = list(range(n_seq))
    hs = {}
    for k, e in engs.items():
        slot, pos = e.prefill_rows(sl, [prompt] * n_seq)
        h = e.forward(e.embed(ids), slot, pos)
        e.advance(sl, [prompt] * n_seq)
        hs[k] = h[prompt - 1::prompt].clone()
    agree = {k: 0 for k in engs if k != "bf16"}
    errs = {k: [] for k in agree}
    for _ in range(n_steps):
        lg = {k: logits(h) for k, h in hs.items()}
        t16 = lg["bf16"].argmax(-1)
        for k in agree:
            errs[k].append(float(rel_err(lg[k], lg["bf16"])))
            agree[k] += int((lg[k].argmax(-1) == t16).sum())
        for k, e in engs.items():  # every engine is fed the bf16 engine's token
            slot, pos = e.prefill_rows(sl, [1] * n_seq)
            hs[k] = e.forward(e.embed(t16), slot, pos).clone()
            e.advance(sl, [1] * n_seq)
    for k in agree:
        line = {"kind": "quality", "against": "bf16", "engine": k, "model": model, "sequences": n_seq, "prompt": prompt,
                "steps": n_steps, "greedy_agreement": round(agree[k] / (n_steps * n_seq), 4),
                "logits_rel_err_median": round(statistics.median(errs[k]), 5), "logits_rel_err_max": round(max(errs[k]), 5)}
        print(json.dumps(line), flush=True)
        out.append(line)


def main():
    ap = argparse.ArgumentParser()
    for flag in ("--kernels", "--steps", "--bench", "--quality"):
        ap.add_argument(flag, action="store_true")
    ap.add_argument("--model", default="llama2-7b")
    ap.add_argument("--batches", default="512,1")
    ap.add_argument("--context", type=int, default=143)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--n-steps", type=int, default=32)
    ap.add_argument("--out", default="bench_kv8.json")
    a = ap.parse_args()
    hip.lib()
    out = []
    if a.kernels:
        kernels(a.windows, out)
    if a.steps:
        steps(a.model, [int(b) for b in a.batches.split(",")], a.windows, a.n_steps, a.context, out)
    if a.bench:
        bench(a.model, 512, a.n_steps, out)
    if a.quality:
        quality(a.model, out)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
