#!/usr/bin/env python3
"""Continuous-batching server over the layer-sharded pipeline, one process per GPU.

    # 8 MI355X, Llama-2-7B shards (or --random for random-init weights of that architecture)
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 --master-port 29500 \\
        serve.py --shards shards/Llama-2-7b-chat-hf_bfloat16 --port 40700
    # client (any host): reference-style user_request message on the ingress port
    python -c "from llm_sharding_amd.utils.node_worker import send_user_request; \\
               send_user_request('127.0.0.1', 40700, text='Write a poem about the blue sky.')"

    # self-contained load test: N synthetic requests, prints a JSON stats line and exits
    python serve.py --model llama2-7b --requests 256 --prompt-len 128 --max-new-tokens 128

All runtime knobs are RuntimeConfig fields (``--batch --microbatches --max-seq --prefill-budget
--no-use-graph --no-causal --trace-dir --log-level ...``).

Rank 0 (embedding stage) is the ingress: it accepts ``{"command": "user_request", "text" |
"input_ids", "max_new_tokens", "reply_to"}`` messages (the reference's control-port JSON /
our LSAM framing, see ``utils/node_worker.send_user_request``) on ``--port``, streams every
finished request to stdout and, if ``reply_to`` is given, pushes ``{"request_id",
"output_ids", "text", "ttft_ms", "tpot_ms"}`` back to that address. ``{"command":
"shutdown"}`` drains the queue and stops every rank. Optional ``temperature``, ``top_k``,
``top_p`` and ``seed`` keys of a request sample on the device instead of greedy decode (one
pipeline stage only), and ``repetition_penalty``, ``presence_penalty`` and ``frequency_penalty``
keys penalise repeated tokens on the device (also at temperature 0; one stage only); a
``logprobs`` key (0..20) adds a ``"logprobs"`` dict to the reply: per-token ``token_logprobs``,
``ranks`` and that many ``top_logprobs`` alternatives (one stage only); ``logit_bias``,
``banned_token_ids``, ``min_tokens``, ``min_p``, ``allowed_token_ids`` and ``choices`` keys constrain
the output on the device (one stage only; ``--state-rows`` sizes the automaton arena); a ``regex``
key makes the output's bytes fully match a pattern (one stage only; ``--dfa-rows`` sizes the
byte-level DFA arena; ``--regex PATTERN`` does the same for every request of the load test); a
``json_object: true`` or ``response_format: {"type": "json_object"}`` key makes the output one JSON
object (one stage only; ``--json`` does the same for the load test, ``--json-max-ws`` bounds the
whitespace runs);
``--temperature --top-k --top-p --repetition-penalty --presence-penalty --frequency-penalty
--logprobs --min-p --min-tokens`` do the same for the synthetic load test (request i seeded with
``--seed`` + i).
``--prefix-slots P`` adds a pool of P KV slots for shared prompt prefixes: a request's
``cache_prefix`` key declares its leading tokens worth keeping, every request forks the longest
pooled match instead of prefilling it, and an ``n`` key asks for that many samples of one prompt
behind one prefill (the reply then carries a ``"choices"`` list). ``--shared-prefix-len L`` gives
the load test's requests the same first L tokens, declared; ``--n N`` makes each of them N samples.
"""
import argparse
import json
import os
import sys
import threading
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from llm_sharding_amd.parallel.scheduler import plan_stages  # noqa: E402
from llm_sharding_amd.parallel.server import PipelineServer  # noqa: E402
from llm_sharding_amd.utils.log import get_logger  # noqa: E402
from llm_sharding_amd.utils.runtime_config import RuntimeConfig  # noqa: E402


def _ingress(srv, port, tok, stop_evt, default_new):
    from llm_sharding_amd.parallel.ingress import Replies, run_ingress
    from llm_sharding_amd.parallel.transport import PullSocket
    sock = PullSocket(f"tcp://*:{port}")
    print(f"[INFO] ingress listening on tcp://*:{sock.port}", flush=True)
    replies = Replies(tok)
    try:
        run_ingress(srv, sock, tok, stop_evt, default_new, replies)
    finally:
        sock.close()
        replies.close()


def main():
    ap = argparse.ArgumentParser(description="continuous-batching pipeline server (one process per GPU)")
    RuntimeConfig.add_arguments(ap)
    ap.add_argument("--random", default="", help="alias of --model: random-init weights of a preset")
    ap.add_argument("--requests", type=int, default=0, help="synthetic load test: N requests, then exit")
    ap.add_argument("--prompt-len", type=int, default=128)
    ap.add_argument("--temperature", type=float, default=0.0, help="load test: sample instead of greedy decode "
                                                                   "(request i uses seed --seed + i; one stage only)")
    ap.add_argument("--top-k", type=int, default=0)
    ap.add_argument("--top-p", type=float, default=1.0)
    ap.add_argument("--repetition-penalty", type=float, default=1.0, help="load test: HF's repetition_penalty "
                                                                          "(1: off; one stage only)")
    ap.add_argument("--presence-penalty", type=float, default=0.0)
    ap.add_argument("--frequency-penalty", type=float, default=0.0)
    ap.add_argument("--logprobs", type=int, default=None, metavar="N",
                    help="load test: collect per-token log-probabilities and N (0..20) alternatives (one stage only)")
    ap.add_argument("--min-p", type=float, default=None,
                    help="load test: drop tokens with p < min_p * p_max (needs --temperature; one stage only)")
    ap.add_argument("--min-tokens", type=int, default=0, help="load test: no EOS before this many tokens (one stage only)")
    ap.add_argument("--state-rows", type=int, default=256,
                    help="rows of the automaton arena of constrained requests (one per automaton state; allocated "
                         "with the first constrained request: 16 MB at V = 32000, 66 MB at V = 128256 for 256)")
    ap.add_argument("--regex", default=None, metavar="PATTERN",
                    help="load test: every request's output, as bytes, fully matches PATTERN (one stage only)")
    ap.add_argument("--json", action="store_true",
                    help="load test: every request's output is one JSON object (one stage only; not with --regex)")
    ap.add_argument("--json-max-ws", type=int, default=2, metavar="N",
                    help="json_object requests: the longest whitespace run between JSON tokens, 0..8")
    ap.add_argument("--dfa-rows", type=int, default=4096, metavar="N",
                    help="rows of the byte-level DFA arena of requests with a regex (one per DFA state, 512 B each "
                         "whatever the vocabulary; allocated with the first such request)")
    ap.add_argument("--prefix-slots", type=int, default=0, metavar="P",
                    help="KV slots of the prefix pool (0: no prefix caching, no parallel samples)")
    ap.add_argument("--shared-prefix-len", type=int, default=0, metavar="L",
                    help="load test: every request starts with the same L tokens and declares them")
    ap.add_argument("--n", type=int, default=1, metavar="N", help="load test: N samples per prompt (submit_n)")
    ap.add_argument("--kv-dtype", default="bf16", choices=("bf16", "fp8"),
                    help="KV cache format: fp8 = e4m3 codes + one power-of-two scale per cached vector "
                         "(8448 instead of 16384 bytes per Llama-2-7B token and layer; no --prefix-slots)")
    ap.add_argument("--kv-layout", default="static", choices=("static", "paged"),
                    help="KV cache layout: paged = a pool of 64-token pages behind a block table; a request holds the "
                         "pages of prompt + max_new_tokens instead of a max_seq slot (bf16 KV; no --prefix-slots, no --n)")
    ap.add_argument("--kv-pages", type=int, default=0, metavar="N",
                    help="with --kv-layout paged: pages in every stage's pool (0: sized from the free HBM)")
    argv = sys.argv[1:]
    for i in range(len(argv) - 1):  # a pattern that starts with '-' is no option
        if argv[i] == "--regex":
            argv[i:i + 2] = ["--regex=" + argv[i + 1]]
            break
    a = ap.parse_args(argv)
    if a.random:
        a.model = a.random
    rc = RuntimeConfig.from_args(a)
    if rc.trace_dir:
        os.environ["LSA_TRACE"] = rc.trace_dir
    os.environ.setdefault("LSA_LOG_LEVEL", rc.log_level)
    log = get_logger("serve")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    dev = rc.torch_device(local)
    gpu = dev.type == "cuda"
    if gpu:
        torch.cuda.set_device(dev)
    ctrl = None
    if world > 1:
        import torch.distributed as dist
        if gpu:
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group("gloo")
        ctrl = dist.new_group(backend="gloo")
    cfg, source = rc.model_and_source()
    M = rc.microbatches or max(2, world)
    paged = a.kv_layout == "paged"
    if a.kv_pages and not paged:
        raise SystemExit("[ERROR] --kv-pages needs --kv-layout paged")
    if paged and rc.batch == 0:
        raise SystemExit("[ERROR] --kv-layout paged sizes its pages from the HBM (--kv-pages 0), not its slots: "
                         "give --batch")
    if rc.batch == 0:  # size the KV cache from this GPU's HBM
        from llm_sharding_amd.parallel.scheduler import scratch_bytes, size_kv_slots
        mem = torch.cuda.get_device_properties(dev).total_memory if gpu else 64e9
        # activations / workspaces of every concurrently replayed scratch set, plus 8 GB slack
        reserve = 8e9 + scratch_bytes(cfg, rc.prefill_budget, sets=max(1, rc.streams))
        # (the KV budget moves layer boundaries: iterated to a fixed point, priced by the cache format)
        rc.batch, _ = size_kv_slots(cfg, world, rc.max_seq, mem, reserve, M, a.prefix_slots, a.kv_dtype)
        log.info(f"KV cache sized from {mem / 1e9:.0f} GB HBM: {rc.batch} slots x {M} micro-batches")
    if paged:
        from llm_sharding_amd.parallel.scheduler import scratch_bytes, size_kv_pages
        kv_pages = a.kv_pages
        if kv_pages:
            plan = plan_stages(cfg, world, kv_tokens=rc.max_seq * rc.batch * M, kv_layout="paged", kv_pages=kv_pages)
        else:  # what fits every stage next to its weights, its staging layer and its scratch (a fixed point:
            # the page budget moves the layer boundaries)
            mem = torch.cuda.get_device_properties(dev).total_memory if gpu else 64e9
            reserve = 8e9 + scratch_bytes(cfg, rc.prefill_budget, sets=max(1, rc.streams))
            kv_pages, plan = size_kv_pages(cfg, world, rc.batch * M, rc.max_seq, mem, reserve)
            log.info(f"paged KV cache sized from {mem / 1e9:.0f} GB HBM: {kv_pages} pages of 64 tokens per stage")
    else:
        kv_pages = None
        plan = plan_stages(cfg, world, kv_tokens=rc.max_seq * (rc.batch * M + a.prefix_slots), kv_dtype=a.kv_dtype)
    st = plan.stages[rank]
    if rank == 0:
        log.info(f"{cfg.name}: {world} stage(s) {plan.ranges()}, {M} x {rc.batch} slots")
    # the tokenizer of the shards (the synthetic byte tokenizer for random weights) and, on a
    # single-stage server, the byte strings of its vocabulary: what a request with a regex needs
    tok = vocab_bytes = None
    if rank == 0:
        from llm_sharding_amd.models.tokenizer import SyntheticByteTokenizer, load_tokenizer
        try:
            tok = load_tokenizer(rc.shards) if rc.shards else None
        except Exception as e:  # noqa: BLE001
            log.warning(f"no tokenizer: {e}")
        if world == 1:
            from llm_sharding_amd.ops.grammar import VocabBytes
            try:
                vocab_bytes = VocabBytes.from_tokenizer(tok if tok is not None else SyntheticByteTokenizer(cfg.vocab_size),
                                                        cfg.vocab_size)
            except Exception as e:  # noqa: BLE001 - requests with a regex are then refused one by one
                log.warning(f"no byte strings of the vocabulary: {e}")
    srv = PipelineServer(cfg, source, rank, world, st.start, st.end, dev, batch=rc.batch, microbatches=M,
                         max_seq=rc.max_seq, prefill_budget=rc.prefill_budget, use_graph=rc.use_graph,
                         dtype=rc.torch_dtype(dev) if gpu else torch.float32, ctrl_group=ctrl, causal=rc.causal,
                         streams=rc.streams, prefix_slots=a.prefix_slots, state_rows=a.state_rows,
                         vocab_bytes=vocab_bytes, dfa_rows=a.dfa_rows, kv_dtype=a.kv_dtype, json_max_ws=a.json_max_ws,
                         kv_layout=a.kv_layout, kv_pages=kv_pages)
    if rank != 0:
        srv.serve()
    elif a.requests:
        g = torch.Generator().manual_seed(rc.seed + 1)
        shared = torch.randint(3, cfg.vocab_size, (min(a.shared_prefix_len, a.prompt_len),), generator=g).tolist()
        for i in range(a.requests):
            ids = shared + torch.randint(3, cfg.vocab_size, (a.prompt_len - len(shared),), generator=g).tolist()
            pen = (a.repetition_penalty, a.presence_penalty, a.frequency_penalty)
            kw = {}
            if (a.temperature > 0 or pen != (1.0, 0.0, 0.0) or a.logprobs is not None or a.min_p is not None
                    or a.min_tokens or a.regex is not None or a.json):
                from llm_sharding_amd.runtime.sampling import SamplingParams
                kw["sampling"] = SamplingParams(a.temperature, a.top_k, a.top_p, rc.seed + i * a.n, *pen,
                                                logprobs=a.logprobs, min_p=a.min_p, min_tokens=a.min_tokens,
                                                regex=a.regex, json_object=a.json)
            if a.n > 1:
                srv.submit_n(ids, a.n, rc.max_new_tokens, eos_ids=(), **kw)
            elif shared and a.prefix_slots:
                srv.submit(ids, rc.max_new_tokens, eos_ids=(), cache_prefix=len(shared), **kw)
            else:
                srv.submit(ids, rc.max_new_tokens, eos_ids=(), **kw)
        t0 = time.perf_counter()
        srv.t_start = t0
        srv.serve(stop_when_idle=True)
        s = srv.stats()
        s.update({"metric": "serving_output_tokens_per_sec", "n_gpus": world, "model": cfg.name,
                  "requests": a.requests * a.n, "prompt_len": a.prompt_len, "max_new_tokens": rc.max_new_tokens,
                  "prefix_slots": a.prefix_slots, "shared_prefix_len": len(shared), "n": a.n,
                  "slots": rc.batch * M, "microbatches": M, "kv_layout": a.kv_layout, "kv_pages": kv_pages})
        print(json.dumps(s), flush=True)
    else:
        stop_evt = threading.Event()
        th = threading.Thread(target=_ingress, args=(srv, rc.port, tok, stop_evt, rc.max_new_tokens), daemon=True)
        th.start()
        srv.serve(stop_when_idle=False, should_stop=stop_evt.is_set)
        th.join(timeout=5)
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
