#!/usr/bin/env python3
"""Single-process generation (reference inference.py, which calls HF generate): the whole model
on one device through the MI355X engine (hipGraph decode on GPU). Greedy by default;
``--temperature T [--top-k K] [--top-p P] [--seed S]`` samples on the device instead (the
``do_sample / top_p / temperature`` switches of the reference's generate call), reproducibly:
the seed in use is printed, and the same seed gives the same tokens.
``--repetition-penalty R`` (the reference's commented-out ``repetition_penalty=1.2``),
``--presence-penalty A`` and ``--frequency-penalty B`` penalise repeated tokens on the device, with
or without a temperature (temperature 0: the arg-max of the penalised logits).
``--logprobs N`` (0..20) prints each generated token's log-probability, rank and N most likely
alternatives (of the penalised logits at temperature 1, before top-k / top-p); ``--score`` prints the
prompt's own per-token log-probabilities, mean NLL and perplexity instead of generating.
``--logit-bias ID:VAL`` and ``--ban ID`` (both repeatable), ``--min-tokens N``, ``--min-p P`` and
``--choice TEXT`` (repeatable: the output is exactly one of the texts' token sequences, then EOS)
constrain the output on the device (``ops.constraints``); not together with ``--speculative``,
``--score`` or ``--hf-compare``.
``--speculative K [--spec-ngram MIN,MAX]`` decodes speculatively: K tokens drafted from the sequence's
own history (the longest n-gram match of MIN..MAX tokens) are verified in one step of K + 1 rows; the
output is the plain output, greedy or sampled, in fewer steps when the text repeats itself.
``--speculative K --draft-shards DIR`` (or ``--draft-random PRESET`` beside ``--random``) drafts with a
second, smaller model of the same vocabulary instead (``--spec-ngram`` is ignored then).

    python inference.py --shards DIR [--prompt "..."] [--max-new-tokens 128]
    python inference.py --random llama2-7b --max-new-tokens 64     # random-init weights
    python inference.py --shards DIR --hf-compare HF_DIR           # + the reference's own path
    python inference.py --shards DIR --temperature 0.7 --top-p 0.9 --seed 1
    python inference.py --random llama2-7b --repetition-penalty 1.2
    python inference.py --shards DIR --logprobs 5
    python inference.py --shards DIR --score --prompt "..."
    python inference.py --shards DIR --choice " yes" --choice " no" --choice " maybe"
    python inference.py --shards DIR --temperature 0.8 --min-p 0.05 --min-tokens 16 --ban 13
    python inference.py --shards DIR --speculative 3 [--temperature 0.7 --top-p 0.9 --seed 1]
    python inference.py --shards DIR --speculative 3 --draft-shards SMALL_DIR
    python inference.py --random llama2-7b --speculative 3 --draft-random llama2-7b-2l

``--hf-compare HF_DIR`` also runs what the reference's inference.py runs
(/root/reference/inference.py:16-45: transformers' AutoModelForCausalLM + greedy generate) on the
HF checkpoint the shards were cut from, in fp32 on the CPU, and reports where the two greedy
decodes agree (tests/test_llama_hf_parity.py pins the same parity in the test suite).
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from llm_sharding_amd.config import LlamaConfig, get_preset  # noqa: E402
from llm_sharding_amd.models.tokenizer import SyntheticByteTokenizer, load_tokenizer  # noqa: E402
from llm_sharding_amd.runtime.engine import DecodeGraph, RandomSource, ShardFolderSource  # noqa: E402
from llm_sharding_amd.runtime.engine_int4 import make_stage_engine  # noqa: E402


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shards", default="")
    ap.add_argument("--random", default="", help="preset name for random-init weights (no checkpoint)")
    ap.add_argument("--prompt", default="Write a poem about the blue sky.")
    ap.add_argument("--max-new-tokens", type=int, default=128)
    ap.add_argument("--device", default="cuda:0" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--kv-dtype", default="bf16", choices=("bf16", "fp8"),
                    help="KV cache format: fp8 = e4m3 codes + one power-of-two scale per cached vector (GPU)")
    ap.add_argument("--kv-layout", default="static", choices=("static", "paged"),
                    help="KV cache layout: paged = a pool of 64-token pages behind a block table (GPU); the request "
                         "reserves prompt + --max-new-tokens at admission")
    ap.add_argument("--kv-pages", type=int, default=0,
                    help="with --kv-layout paged: pages in the pool (0: one sequence of max_seq tokens, plus the null page)")
    ap.add_argument("--weight-dtype", default="bf16", choices=("bf16", "fp8", "int4"),
                    help="projection weights on the GPU: bf16, fp8 (OCP e4m3, per-row scales, fp8 lm_head) or int4 "
                         "(symmetric group-128, bf16 lm_head); ignored on the CPU")
    ap.add_argument("--hf-compare", default="", help="HF checkpoint dir: also run transformers' greedy generate "
                                                     "(the reference inference.py's path, fp32 CPU) and compare tokens")
    ap.add_argument("--temperature", type=float, default=0.0, help="0 (default): greedy decode")
    ap.add_argument("--top-k", type=int, default=0, help="keep the k most likely tokens (0: off)")
    ap.add_argument("--top-p", type=float, default=1.0, help="keep the smallest set of mass >= p (1: off)")
    ap.add_argument("--seed", type=int, default=None, help="64-bit sampling seed (default: drawn and printed)")
    ap.add_argument("--repetition-penalty", type=float, default=1.0,
                    help="> 1 damps tokens of the prompt and the output so far (HF's repetition_penalty; 1: off)")
    ap.add_argument("--presence-penalty", type=float, default=0.0,
                    help="subtracted from the logit of every token generated so far (0: off)")
    ap.add_argument("--frequency-penalty", type=float, default=0.0,
                    help="subtracted once per time a token has been generated (0: off)")
    ap.add_argument("--logprobs", type=int, default=None, metavar="N",
                    help="print each generated token's log-probability, rank and N (0..20) alternatives")
    ap.add_argument("--score", action="store_true",
                    help="score the prompt instead of generating: per-token log-probabilities, mean NLL, perplexity")
    ap.add_argument("--logit-bias", action="append", default=[], metavar="ID:VAL",
                    help="add VAL (finite, or -inf) to token ID's logit; repeatable")
    ap.add_argument("--ban", action="append", type=int, default=[], metavar="ID",
                    help="never produce token ID; repeatable")
    ap.add_argument("--min-tokens", type=int, default=0, help="no EOS before this many generated tokens (0: off)")
    ap.add_argument("--min-p", type=float, default=None,
                    help="drop tokens with p < min_p * p_max at the temperature in use (HF's min_p; needs a "
                         "temperature)")
    ap.add_argument("--choice", action="append", default=[], metavar="TEXT",
                    help="the output is exactly one of the given texts (tokenised without special tokens), then EOS; "
                         "repeatable")
    ap.add_argument("--json", action="store_true",
                    help="the output is one JSON object (RFC 8259, whitespace runs of at most 2 bytes, nesting up to "
                         "64), then EOS: a byte-level pushdown automaton masked on the device; not with --regex")
    ap.add_argument("--regex", default=None, metavar="PATTERN",
                    help="the output, as bytes, fully matches PATTERN (a byte-level DFA walked over the vocabulary's "
                         "byte strings on the device), then EOS")
    ap.add_argument("--speculative", type=int, default=0, metavar="K",
                    help="speculative decoding: verify K (1..15) n-gram drafts per step (0: off)")
    ap.add_argument("--spec-ngram", default="1,3", metavar="MIN,MAX",
                    help="n-gram lengths (1 <= MIN <= MAX <= 8) of the draft lookup")
    ap.add_argument("--draft-shards", default="", metavar="DIR",
                    help="with --speculative: draft with the model in DIR (same vocabulary) instead of the n-gram "
                         "lookup; --spec-ngram is ignored then")
    ap.add_argument("--draft-random", default="", metavar="PRESET",
                    help="with --speculative: a random-init draft model (seed 1) of preset PRESET, beside --random")
    ap.add_argument("--draft-weight-dtype", default="bf16", choices=("bf16", "fp8", "int4"),
                    help="the draft model's projection weights on the GPU")
    return ap


def draft_engine_from_args(a, eng):
    """--draft-shards / --draft-random (``speculative_from_args`` has checked them against the other
    flags): None without either, else the draft model whole on one stage of ``eng``'s device, with
    its sequence length and one slot."""
    if not (a.draft_shards or a.draft_random):
        return None
    if a.draft_shards:
        cfg = LlamaConfig.from_pretrained(a.draft_shards)
        src = ShardFolderSource(a.draft_shards, cfg)
    else:
        cfg = get_preset(a.draft_random)
        src = RandomSource(cfg, 1)
    if cfg.vocab_size != eng.cfg.vocab_size:
        raise SystemExit(f"[ERROR] the draft model's vocab_size {cfg.vocab_size} is not the target's {eng.cfg.vocab_size}")
    if cfg.max_position_embeddings < eng.max_seq:
        raise SystemExit(f"[ERROR] the draft model's {cfg.max_position_embeddings} positions are fewer than the "
                         f"target's max_seq {eng.max_seq}")
    return make_stage_engine(cfg, 0, cfg.num_hidden_layers, a.device, eng.dtype, has_embed=True, has_head=True,
                             source=src, max_seq=eng.max_seq, weight_dtype=a.draft_weight_dtype)


def speculative_from_args(a, sp):
    """--speculative / --spec-ngram: None without the flag, else (k, (nmin, nmax)); exits on a value
    out of range or a flag speculation does not combine with."""
    if a.draft_shards and a.draft_random:
        raise SystemExit("[ERROR] --draft-shards and --draft-random are two draft models: pass one")
    if a.speculative == 0:
        if a.draft_shards or a.draft_random:
            raise SystemExit("[ERROR] --draft-shards / --draft-random need --speculative K")
        return None
    from llm_sharding_amd.ops.speculative import MAX_K, MAX_NGRAM
    if not 1 <= a.speculative <= MAX_K:
        raise SystemExit(f"[ERROR] --speculative K must be in [1, {MAX_K}]")
    try:
        nmin, nmax = (int(x) for x in a.spec_ngram.split(","))
    except ValueError:
        raise SystemExit("[ERROR] --spec-ngram takes MIN,MAX")
    if not 1 <= nmin <= nmax <= MAX_NGRAM:
        raise SystemExit(f"[ERROR] --spec-ngram needs 1 <= MIN <= MAX <= {MAX_NGRAM}")
    if a.score or a.hf_compare:
        raise SystemExit("[ERROR] --speculative does not combine with --score or --hf-compare")
    if sp is not None and (sp.penalized or sp.logprobs is not None):
        raise SystemExit("[ERROR] --speculative does not combine with the penalty flags or --logprobs "
                         "(their state is sequential per token)")
    if constraint_flags(a):
        raise SystemExit("[ERROR] --speculative does not combine with --logit-bias, --ban, --min-tokens, --min-p or "
                         "--choice (the constraint state is sequential per token)")
    if a.regex is not None:
        raise SystemExit("[ERROR] --speculative does not combine with --regex (the DFA state is sequential per token)")
    if a.json:
        raise SystemExit("[ERROR] --speculative does not combine with --json (the automaton's state and stack are "
                         "sequential per token)")
    return a.speculative, (nmin, nmax)


def constraint_flags(a) -> bool:
    return bool(a.logit_bias or a.ban or a.min_tokens or a.min_p is not None or a.choice)


def sampling_from_args(a, choices=None):
    """The run's SamplingParams; None for the greedy default (temperature 0, no penalty, no
    logprobs, no constraint). ``choices``: the token sequences of ``--choice``."""
    from llm_sharding_amd.runtime.sampling import SamplingParams
    pen = (a.repetition_penalty, a.presence_penalty, a.frequency_penalty)
    if (a.temperature == 0.0 and a.top_k == 0 and a.top_p == 1.0 and a.seed is None and pen == (1.0, 0.0, 0.0)
            and a.logprobs is None and not constraint_flags(a) and a.regex is None and not a.json):
        return None
    bias = {}
    for item in a.logit_bias:
        k, sep, v = item.partition(":")
        try:
            bias[int(k)] = float(v)
        except ValueError:
            raise SystemExit(f"[ERROR] --logit-bias takes ID:VAL, got {item!r}")
    try:
        sp = SamplingParams(a.temperature, a.top_k, a.top_p, a.seed, *pen, logprobs=a.logprobs, logit_bias=bias or None,
                            banned_token_ids=a.ban or None, min_tokens=a.min_tokens, min_p=a.min_p, choices=choices,
                            regex=a.regex, json_object=a.json)
    except ValueError as e:
        if constraint_flags(a) or a.regex is not None or a.json:
            raise SystemExit(f"[ERROR] {e}")
        raise
    return None if sp.plain else sp


def join_regex_arg(argv):
    """``--regex PATTERN`` as ``--regex=PATTERN``: argparse would take a pattern that starts with
    '-' (``-?[0-9]+``) for an option."""
    argv = list(sys.argv[1:] if argv is None else argv)
    for i in range(len(argv) - 1):
        if argv[i] == "--regex":
            argv[i:i + 2] = ["--regex=" + argv[i + 1]]
            break
    return argv


def main(argv=None):
    a = build_parser().parse_args(join_regex_arg(argv))
    sp = sampling_from_args(a)
    spec = speculative_from_args(a, sp)
    if sp is not None and a.hf_compare:
        raise SystemExit("[ERROR] --hf-compare checks the greedy decode: drop the sampling and penalty flags")
    if (constraint_flags(a) or a.regex is not None or a.json) and (a.score or a.hf_compare):
        raise SystemExit("[ERROR] --score and --hf-compare do not combine with --logit-bias, --ban, --min-tokens, "
                         "--min-p, --choice, --regex or --json")
    if a.shards:
        cfg = LlamaConfig.from_pretrained(a.shards)
        src, tok = ShardFolderSource(a.shards, cfg), load_tokenizer(a.shards)
    else:
        cfg = get_preset(a.random or "tiny")
        src, tok = RandomSource(cfg), SyntheticByteTokenizer(cfg.vocab_size)
    dt = torch.bfloat16 if a.device.startswith("cuda") else torch.float32
    max_seq = min(cfg.max_position_embeddings, 4096)
    kv_pages = None
    if a.kv_layout == "paged":
        if spec is not None:
            raise SystemExit("[ERROR] --speculative does not combine with --kv-layout paged yet (the speculative "
                             "graph's admission does not reserve pages)")
        kv_pages = a.kv_pages or max_seq // 64 + 1
    elif a.kv_pages:
        raise SystemExit("[ERROR] --kv-pages needs --kv-layout paged")
    t0 = time.perf_counter()
    eng = make_stage_engine(cfg, 0, cfg.num_hidden_layers, a.device, dt, has_embed=True, has_head=True, source=src,
                            max_seq=max_seq, weight_dtype=a.weight_dtype, kv_dtype=a.kv_dtype, kv_layout=a.kv_layout,
                            kv_pages=kv_pages)
    ids = tok(a.prompt, return_tensors="pt")["input_ids"][0]
    if getattr(eng, "paged", False):  # admission: the whole request's pages, before any graph replays
        eng.kv_reserve(0, min(eng.max_seq, ids.numel() + a.max_new_tokens))
    if a.choice:
        sp = sampling_from_args(a, [tok.encode(c, add_special_tokens=False) for c in a.choice])
    print(f"[INFO] loaded in {time.perf_counter() - t0:.1f}s; prompt tokens {ids.numel()}")
    if a.score:
        return score(eng, tok, ids.tolist())
    draft = draft_engine_from_args(a, eng)
    slot, pos = eng.prefill_rows([0], [ids.numel()])
    h = eng.forward(eng.embed(ids.to(a.device)), slot, pos)
    eng.advance([0], [ids.numel()])
    if spec is not None:
        out, dt_s, st = speculative_tokens(eng, h, ids.tolist(), a.max_new_tokens, spec[0], spec[1], sp, cfg.eos_ids,
                                           draft=draft)
        out = report(a, cfg, tok, ids, out, dt_s)
        if draft is not None:
            print(f"[INFO] speculative k={spec[0]} draft model {draft.cfg.name} ({draft.n_layers} layers, "
                  f"{a.draft_weight_dtype}): {st['tokens']} tokens in {st['steps']} steps, "
                  f"{st['tokens'] / max(1, st['steps']):.2f} tokens per step")
            return out
        print(f"[INFO] speculative k={spec[0]} n-gram {spec[1][0]}..{spec[1][1]}: {st['tokens']} tokens in {st['steps']} "
              f"steps, {st['tokens'] / max(1, st['steps']):.2f} tokens per step, a draft matched in {st['matched']} steps")
        return out
    if sp is not None:
        lp = {}
        out, dt_s = sample_tokens(eng, h, ids.numel(), a.max_new_tokens, sp, prompt_ids=ids.tolist(), lp_out=lp,
                                  tok=tok)
        out = report(a, cfg, tok, ids, out, dt_s)
        if sp.grammar is not None:
            report_regex(sp, tok, cfg, out)
        if sp.json_object:
            report_json(tok, cfg, out)
        if lp:
            print_logprobs(tok, out, lp)
        return out
    first = eng.head(h, [ids.numel() - 1])
    out = [int(first[0])]
    t1 = time.perf_counter()
    if eng.gpu:
        g = DecodeGraph(eng, 1, "full", history_len=a.max_new_tokens)
        g.tokens.copy_(first.to(torch.int32))
        g.capture()
        for _ in range(a.max_new_tokens - 1):
            g.replay()
        torch.cuda.synchronize()
        out += g.history[:a.max_new_tokens - 1, 0].tolist()
    else:
        cur = first
        for _ in range(a.max_new_tokens - 1):
            slot, pos = eng.prefill_rows([0], [1])
            h = eng.forward(eng.embed(cur), slot, pos)
            eng.advance([0], [1])
            cur = eng.head(h)
            out.append(int(cur[0]))
    dt_s = time.perf_counter() - t1
    return report(a, cfg, tok, ids, out, dt_s)


def score(eng, tok, ids: list):
    """--score: log p(ids[t + 1] | ids[..t]) of the prompt, its mean NLL and perplexity. Returns
    the per-token log-probabilities (a list of len(ids) - 1 floats)."""
    import math
    from llm_sharding_amd.runtime.sampling import score_prompt
    res = score_prompt(eng, ids)
    lps = res.tok_lp.tolist()
    for t, lp, rk in zip(ids[1:], lps, res.tok_rank.tolist()):
        print(f"  {t:>7d} {tok.decode([t])!r:<16} logprob {lp:10.4f}  rank {rk}")
    nll = -sum(lps) / len(lps)
    print(f"[INFO] scored {len(lps)} tokens: mean NLL {nll:.6f}  perplexity {math.exp(nll):.6f}")
    return lps


def print_logprobs(tok, out: list, lp: dict) -> None:
    """--logprobs: one line per generated token."""
    for i, t in enumerate(out):
        alts = "  ".join(f"{j}:{v:.3f}" for j, v in lp["top"][i])
        print(f"  {t:>7d} {tok.decode([t])!r:<16} logprob {lp['lp'][i]:10.4f}  rank {lp['rank'][i]}"
              + (f"  top [{alts}]" if alts else ""))


def speculative_tokens(eng, h, ids: list, n_new: int, k: int, ngram: tuple, sp, eos_ids, draft=None) -> tuple:
    """Speculative continuation of the prefilled sequence in slot 0 (``h``: the prefill's final
    hidden): the first token from the head (``Sampler.sample`` when sampling), the rest from a
    captured ``SpecDecodeGraph`` on the GPU (the eager twin on the CPU), replayed until the sequence
    is done. ``draft``: a draft engine instead of the n-gram lookup (its slot 0 is prefilled by
    ``admit``). Returns (tokens, seconds, {steps, tokens, matched})."""
    from llm_sharding_amd.runtime.sampling import Sampler
    from llm_sharding_amd.runtime.speculative import EagerSpecDecode, SpecDecodeGraph
    if sp is None:
        first = eng.head(h, [len(ids) - 1])
    else:
        print(f"[INFO] sampling: temperature {sp.temperature} top_k {sp.top_k} top_p {sp.top_p} seed {sp.seed}")
        first = Sampler(eng).sample(h, [len(ids) - 1], [sp], [len(ids)])
    t1 = time.perf_counter()
    g = (SpecDecodeGraph if eng.gpu else EagerSpecDecode)(eng, 1, k, ngram=ngram, sampling=sp is not None,
                                                          history_len=max(1, n_new), eos_ids=eos_ids, draft=draft)
    try:
        g.admit(0, ids + [int(first[0])], n_new, sp)
    except ValueError as e:
        raise SystemExit(f"[ERROR] {e}")
    g.capture()
    left = n_new - 1
    while left > 0 and not g.all_done():  # the fewest steps that can finish, then one look at the device
        for _ in range(-(-left // (k + 1))):
            g.replay()
        r = g.results()[0]
        left = n_new - len(r["tokens"])
    dt_s = time.perf_counter() - t1
    r = g.results()[0]
    return r["tokens"], dt_s, {"steps": len(r["accepted"]), "tokens": sum(r["accepted"]), "matched": r["matched"]}


def report_regex(sp, tok, cfg, out: list) -> None:
    """--regex: the generated bytes and whether they match (an output cut by --max-new-tokens is a
    live prefix of a match)."""
    from llm_sharding_amd.ops.grammar import VocabBytes
    data = VocabBytes.from_tokenizer(tok, cfg.vocab_size).decode([t for t in out if t not in cfg.eos_ids])
    full = sp.grammar.accepts(data)
    print(f"[INFO] regex {sp.regex!r}: output {data!r} " + ("matches" if full else
          ("is a prefix of a match (cut by --max-new-tokens)" if sp.grammar.walk(data) >= 0 else "DOES NOT MATCH")))


def report_json(tok, cfg, out: list) -> None:
    """--json: the generated bytes and whether they parse (an output cut by --max-new-tokens is a
    live prefix of a JSON object)."""
    import json
    from llm_sharding_amd.ops.grammar import VocabBytes
    from llm_sharding_amd.ops.pda import BytePDA
    data = VocabBytes.from_tokenizer(tok, cfg.vocab_size).decode([t for t in out if t not in cfg.eos_ids])
    try:
        parsed = isinstance(json.loads(data.decode("utf-8")), dict)
    except ValueError:
        parsed = False
    print(f"[INFO] json: output {data!r} " + ("parses as a JSON object" if parsed else
          ("is a live prefix of a JSON object (cut by --max-new-tokens)" if BytePDA.json().alive(data) else "DOES NOT PARSE")))


def sample_tokens(eng, h, n_prompt: int, n_new: int, sp, prompt_ids=None, lp_out=None, tok=None) -> tuple:
    """Sampled continuation of the prefilled sequence in slot 0 (``h``: the prefill's final
    hidden): the first token from ``Sampler.sample``, the rest from a captured
    ``SamplingDecodeGraph`` on the GPU (the eager twin on the CPU). With a penalty the
    sequence's token statistics (``PenaltyState``, ``prompt_ids`` marked) ride along, with a
    constraint its ``ConstraintState``, with a regex or ``json_object`` its ``GrammarState`` over the byte strings of
    ``tok``'s vocabulary (``runtime.logit_stages``). With ``sp.logprobs`` the tokens'
    log-probabilities, ranks and alternatives go into the dict ``lp_out`` (``lp``, ``rank``, ``top``:
    per token a list of (id, logprob))."""
    from llm_sharding_amd.ops.grammar import VocabBytes
    from llm_sharding_amd.ops.pda import BytePDA
    from llm_sharding_amd.runtime.logit_stages import STAGE_CLASSES
    from llm_sharding_amd.runtime.sampling import EagerSamplingDecode, Sampler, SamplingDecodeGraph
    print(f"[INFO] sampling: temperature {sp.temperature} top_k {sp.top_k} top_p {sp.top_p} seed {sp.seed}")
    build = {  # a one-slot state per stage the request asks for, and the line that reports it
        "penalties": lambda cls: (cls(eng, 1), f"penalties: repetition {sp.repetition_penalty} presence "
                                  f"{sp.presence_penalty} frequency {sp.frequency_penalty}"),
        "constraints": lambda cls: (cls(eng, 1, state_rows=max(1, sum(len(c) for c in sp.choices or ()) + 2)),
                                    f"constraints: {len(sp.bias_entries())} bias entries, min_tokens {sp.min_tokens}, "
                                    f"min_p {sp.min_p}, {len(sp.choices or ())} choices"),
        "grammar": lambda cls: (
            (cls(eng, 1, VocabBytes.from_tokenizer(tok, eng.cfg.vocab_size), dfa_rows=1, pda=BytePDA.json()),
             f"json: a byte-level pushdown automaton of {BytePDA.json().n_states} states") if sp.json_object else
            (cls(eng, 1, VocabBytes.from_tokenizer(tok, eng.cfg.vocab_size), dfa_rows=sp.grammar.n_states),
             f"regex {sp.regex!r}: a byte-level DFA of {sp.grammar.n_states} states")),
    }
    kw = {}
    for cls in STAGE_CLASSES:
        if cls.wants(sp):
            try:
                kw[cls.name], line = build[cls.name](cls)
                kw[cls.name].enter(0, sp, prompt_ids)
            except ValueError as e:
                raise SystemExit(f"[ERROR] {e}")
            print(f"[INFO] {line}")
    want_lp = sp.logprobs is not None
    first = Sampler(eng, **kw).sample(h, [n_prompt - 1], [sp], [n_prompt], slots=[0] if kw else None,
                                      return_logprobs=want_lp)
    steps = []
    if want_lp:
        first, lp0 = first
        steps.append((lp0.tok_rank[0].clone(), lp0.top_id[0].clone(), lp0.top_lp[0].clone()))
        kw["logprobs"] = True
    t1 = time.perf_counter()
    g = (SamplingDecodeGraph if eng.gpu else EagerSamplingDecode)(eng, 1, "full", history_len=max(1, n_new - 1), **kw)
    g.set_params(0, sp)
    g.tokens.copy_(first.to(torch.int32))
    g.capture()
    for _ in range(n_new - 1):
        g.replay()
        if want_lp:  # device-side copies, no host wait per token
            steps.append((g.lp.tok_rank[0].clone(), g.lp.top_id[0].clone(), g.lp.top_lp[0].clone()))
    if eng.gpu:
        torch.cuda.synchronize()
    dt_s = time.perf_counter() - t1
    if want_lp and lp_out is not None:
        lp_out["lp"] = [float(lp0.tok_lp[0])] + g.lp_history[:n_new - 1, 0].tolist()
        lp_out["rank"] = [int(r) for r, _, _ in steps]
        lp_out["top"] = [list(zip(i[:sp.logprobs].tolist(), v[:sp.logprobs].tolist())) for _, i, v in steps]
    return [int(first[0])] + g.history[:n_new - 1, 0].tolist(), dt_s


def report(a, cfg, tok, ids, out, dt_s):
    eos = [i for i, t in enumerate(out) if t in cfg.eos_ids]
    if eos:
        out = out[:eos[0] + 1]
    print(tok.decode(ids.tolist() + out, skip_special_tokens=True))
    print(f"[INFO] {len(out)} new tokens, {max(1, len(out) - 1) / max(dt_s, 1e-9):.1f} tok/s decode")
    if a.hf_compare:
        hf = hf_greedy(a.hf_compare, ids, len(out))
        same = next((i for i, (x, y) in enumerate(zip(out, hf)) if x != y), len(out))
        print(f"[INFO] HF greedy (transformers, fp32 CPU) agrees on the first {same}/{len(out)} tokens"
              + ("" if same == len(out) else f"; first divergence at token {same}: ours {out[same]}, HF {hf[same]}"))
    return out


def hf_greedy(hf_dir: str, ids: torch.Tensor, n_new: int) -> list:
    """The reference's single-process path: AutoModelForCausalLM.from_pretrained + greedy
    generate (/root/reference/inference.py:16-45), here fp32 on the CPU as the oracle."""
    from transformers import AutoModelForCausalLM
    m = AutoModelForCausalLM.from_pretrained(hf_dir, dtype=torch.float32).eval()
    with torch.no_grad():
        g = m.generate(ids[None].cpu(), max_new_tokens=n_new, min_new_tokens=n_new, do_sample=False)
    return g[0, ids.numel():].tolist()


if __name__ == "__main__":
    main()
