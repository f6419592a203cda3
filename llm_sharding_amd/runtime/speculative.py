"""Speculative decoding on top of :class:`StageEngine`: ``k`` drafted tokens per sequence are
verified in one decode step of ``k + 1`` rows, and the step keeps every token the model agrees with
plus the model's own next one. Greedy decode, :class:`DecodeGraph` and the sampling graphs are
untouched: everything here is an extra path that exists only when a caller asks for it.

The step is ``draft -> embed -> layers -> head -> accept`` (``ops.speculative`` has the two
contracts). The ``k + 1`` rows of a sequence share its KV slot at consecutive positions: the QKV
epilogue appends every row's K/V before attention launches and every decode attention kernel is
causal by position, so row ``j`` sees exactly the tokens before it - a causal verification pass.
The static cache is addressed by position: cells written for rejected drafts lie beyond every later
row's position until the next step overwrites them, so rolling back costs nothing.

Acceptance is plain token equality, also when sampling: ``lsa_sample``'s noise is a pure function
of (seed, position, vocabulary index) and row ``j`` samples with the counter ``pos_j + 1``, exactly
as the non-speculative graph does. A row whose inputs are the tokens the plain decode would have
fed produces the token the plain decode would have produced, so no rejection-sampling correction
exists: the output is the plain output, token for token (given the same kernel numerics).

* :class:`SpecDecodeGraph` - the captured step; all state on the device, replayed with no host
  work per step.
* :class:`EagerSpecDecode` - the same interface over ``eng.embed / forward / head`` and the numpy
  references: what CPU engines run, and the graph's twin in tests on a GPU engine.
* :func:`generate_speculative` - prefill and speculative steps to completion.

**A draft model** (``draft=``): the drafts come from a second, smaller :class:`StageEngine` of the
same vocabulary, run greedily inside the same step (``ops.speculative``, **Draft model**):

    ``dm_begin -> [draft embed -> layers -> head -> argmax_finalize -> dm_chain] x k -> embed -> ..``

Iteration 0 feeds the draft two rows per sequence (the last two known tokens: at most one of the
draft's cells is missing after a step that accepted every draft), the others one. Acceptance stays
token equality against the target's own (greedy or sampled) token, so whatever the draft proposes
the output is the target's plain output; a better draft only makes the steps fewer. The draft's
static cache is addressed by position like the target's: nothing is rolled back.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from ..ops import sampling as S
from ..ops import speculative as OS
from .engine import StageEngine
from .sampling import GREEDY, Sampler, SamplingParams, _check_full_head, device_params


class _SpecState:
    """What both implementations share: validation, admission, results. State arrays are numpy on
    the host (``EagerSpecDecode``) or torch on the device (``SpecDecodeGraph``); a sequence that has
    not been admitted is parked as a finished one at the far end of its slot (``hlen = max_seq - k``:
    its rows rewrite cells no admitted sequence can ever rely on, since ``limit + k <= max_seq``)."""

    def __init__(self, eng: StageEngine, n_seq: int, k: int, slots, ngram, script: bool, sampling: bool,
                 history_len: int, eos_ids, draft: Optional[StageEngine] = None):
        _check_full_head(eng)
        if not eng.has_embed:
            raise RuntimeError("[ERROR] speculative decoding needs the stage that owns the embedding")
        self.eng, self.n_seq, self.k = eng, int(n_seq), int(k)
        self.max_seq = self.ld = eng.max_seq
        self.ngram = (int(ngram[0]), int(ngram[1]))
        OS.check_shape(self.n_seq, self.k, self.ld, self.max_seq, self.ngram)
        self.rows = self.n_seq * (self.k + 1)
        if self.rows > eng.DECODE_MAX_ROWS or OS.MAX_ROWS != eng.DECODE_MAX_ROWS:
            raise ValueError(f"speculative: {self.rows} rows exceed the decode path's {eng.DECODE_MAX_ROWS}")
        self.slots = list(range(self.n_seq)) if slots is None else [int(s) for s in slots]
        if len(self.slots) != self.n_seq or len(set(self.slots)) != self.n_seq:
            raise ValueError(f"speculative: {self.n_seq} sequences need {self.n_seq} distinct slots, got {self.slots}")
        if any(not 0 <= s < eng.max_slots for s in self.slots):
            raise ValueError(f"speculative: slots {self.slots} outside the engine's {eng.max_slots}")
        self.slot_rows = [s for s in self.slots for _ in range(self.k + 1)]
        self.use_script, self.sampling = bool(script), bool(sampling)
        self.history_len = int(history_len)
        self.eos_np = OS.eos_array(eos_ids)
        self.params = [GREEDY] * self.n_seq
        self.prompt_len = [0] * self.n_seq
        self.limits = [0] * self.n_seq
        self.draft = draft
        if draft is not None:
            self._check_draft(draft)

    def _check_draft(self, d: StageEngine) -> None:
        """The refusals of a draft engine, each naming what does not fit."""
        eng = self.eng
        if self.use_script:
            raise ValueError("speculative: draft= and script=True are two draft sources: pass one of them")
        if d is eng:
            raise ValueError("speculative: the draft must be an engine of its own (its KV cache holds the draft "
                             "model's K/V), not the target engine itself")
        if d.start != 0 or d.end != d.cfg.num_hidden_layers:
            raise ValueError(f"speculative: the draft must hold all its layers on one stage, this one holds "
                             f"[{d.start}, {d.end}) of {d.cfg.num_hidden_layers}")
        if not d.has_embed or d.embed_w is None:
            raise ValueError("speculative: the draft engine has no embedding")
        if d.lm_head is None:
            raise ValueError("speculative: the draft engine has no lm_head")
        if (d.head_v0, d.head_v1) != (0, d.cfg.head_rows):
            raise ValueError(f"speculative: the draft needs its whole lm_head, this one holds vocabulary rows "
                             f"[{d.head_v0}, {d.head_v1}) of {d.cfg.head_rows} (head_cols)")
        if d.cfg.vocab_size != eng.cfg.vocab_size:
            raise ValueError(f"speculative: the draft's vocab_size {d.cfg.vocab_size} is not the target's "
                             f"{eng.cfg.vocab_size}")
        if d.max_seq < self.max_seq:
            raise ValueError(f"speculative: the draft's max_seq {d.max_seq} is below the target's {self.max_seq}")
        if any(s >= d.max_slots for s in self.slots):
            raise ValueError(f"speculative: slots {self.slots} outside the draft engine's {d.max_slots}")
        if d.device != eng.device:
            raise ValueError(f"speculative: the draft is on {d.device}, the target on {eng.device}")

    def _prefill_draft(self, slot: int, toks: np.ndarray) -> None:
        """The draft engine's slot from scratch: K/V of ``toks`` at positions ``0 .. len - 1``."""
        d = self.draft
        d.reset([slot])
        for c0 in range(0, int(toks.size), d.max_prefill_rows):
            chunk = toks[c0:c0 + d.max_prefill_rows]
            srow, pos = d.prefill_rows([slot], [int(chunk.size)])
            d.forward(d.embed(torch.from_numpy(chunk.astype(np.int64))), srow, pos)
            d.advance([slot], [int(chunk.size)])

    # the two implementations write one sequence's state
    def _put(self, i: int, hist_row: np.ndarray, hlen: int, limit: int, done: int) -> None:
        raise NotImplementedError

    def host_state(self) -> dict:
        """numpy copies of hist, hlen, done, acc_history, steps, match_ctr."""
        raise NotImplementedError

    def _check_tokens(self, tokens, what: str) -> np.ndarray:
        t = np.asarray([int(x) for x in tokens], dtype=np.int64)
        if t.size and (t.min() < 0 or t.max() >= self.eng.cfg.vocab_size):
            raise ValueError(f"speculative: {what} token outside the vocabulary")
        return t.astype(np.int32)

    def admit(self, i: int, tokens, max_new_tokens: int, params: Optional[SamplingParams] = None,
              n_prompt: Optional[int] = None) -> None:
        """Sequence ``i`` starts with the known ``tokens``, all but the last of them in the
        sequence's KV slot (``eng.seq_len[slot] == len(tokens) - 1``). By default ``tokens`` is the
        prompt plus the first generated token, as a prefill and its head leave them; ``n_prompt``
        (default ``len(tokens) - 1``) says how many of them are the prompt - ``len(tokens)`` for a
        prompt prefilled up to its last token, whose first new token the first step produces.
        At most ``max_new_tokens`` tokens follow the prompt: ``limit = n_prompt + max_new_tokens``.
        With a draft engine its slot is prefilled here with all but the last of ``tokens``."""
        if not 0 <= i < self.n_seq:
            raise ValueError(f"speculative: sequence {i} outside [0, {self.n_seq})")
        toks = self._check_tokens(tokens, "a prompt")
        n, new = int(toks.size), int(max_new_tokens)
        n_prompt = n - 1 if n_prompt is None else int(n_prompt)
        if n < 1 or new < 1 or not 1 <= n_prompt <= n or n_prompt < n - 1:
            raise ValueError("speculative: admit takes a prompt of >= 1 token, at most one generated token behind "
                             "it, and max_new_tokens >= 1")
        slot = self.slots[i]
        if self.eng.seq_len[slot] != n - 1:
            raise ValueError(f"speculative: slot {slot} holds {self.eng.seq_len[slot]} positions, not the {n - 1} "
                             "tokens before the last known one")
        limit = n_prompt + new
        if limit + self.k > self.max_seq:
            raise ValueError(f"speculative: prompt {n_prompt} + max_new_tokens {new} + k {self.k} exceeds max_seq "
                             f"{self.max_seq} (the k + 1 rows of a step need their positions inside the slot)")
        p = GREEDY if params is None else params
        if p.penalized or p.logprobs is not None:
            raise ValueError("speculative: penalties and logprobs are sequential per slot and not supported "
                             "together with speculation")
        if p.constrained:
            raise ValueError("speculative: constrained decoding (logit_bias, banned_token_ids, min_tokens, min_p, "
                             "allowed_token_ids, choices, automaton) keeps sequential state per slot and is not "
                             "supported together with speculation")
        if p.grammar is not None:
            raise ValueError("speculative: a regex keeps sequential state per slot (the DFA state after every token) "
                             "and is not supported together with speculation")
        if p.json_object:
            raise ValueError("speculative: json_object keeps sequential state per slot (the automaton's state and "
                             "stack after every token) and is not supported together with speculation")
        if not p.greedy and not self.sampling:
            raise ValueError("speculative: a sampled sequence needs sampling=True")
        row = np.zeros(self.ld, dtype=np.int32)
        row[:n] = toks
        done = int(limit == n or (n > n_prompt and int(toks[-1]) in {int(t) for t in self.eos_np if t >= 0}))
        self.params[i], self.prompt_len[i], self.limits[i] = p, n_prompt, limit
        if self.draft is not None:
            self._prefill_draft(slot, toks[:n - 1])
        self._put(i, row, n, limit, done)

    def set_script(self, i: int, tokens) -> None:
        """Script mode: ``tokens[p]`` is the proposal for absolute position ``p`` of sequence ``i``
        (positions beyond the list propose token 0)."""
        if not self.use_script:
            raise RuntimeError("speculative: built without script=True")
        toks = self._check_tokens(tokens, "a script")[:self.ld]
        row = np.zeros(self.ld, dtype=np.int32)
        row[:toks.size] = toks
        self._put_script(i, row)

    def results(self) -> list:
        """Per sequence: ``tokens`` (the generated ones, ``hist[P:hlen]``), ``done``, ``accepted``
        (the accepted count of each of its steps, as far as the history reaches) and ``matched``
        (in how many of its steps the draft came from a match)."""
        st = self.host_state()
        steps = min(int(st["steps"]), self.history_len)
        out = []
        for i in range(self.n_seq):
            acc = [int(m) for m in st["acc_history"][:steps, i] if m > 0] if self.history_len else []
            out.append({"tokens": st["hist"][i, self.prompt_len[i]:int(st["hlen"][i])].tolist(),
                        "done": bool(st["done"][i]), "accepted": acc, "matched": int(st["match_ctr"][i])})
        return out

    def all_done(self) -> bool:
        return bool(self.host_state()["done"].all())

    def sync_positions(self) -> None:
        hlen = self.host_state()["hlen"]
        for i, s in enumerate(self.slots):
            if self.prompt_len[i]:  # parked sequences leave their slot's length alone
                self.eng.seq_len[s] = int(hlen[i]) - 1
                if self.draft is not None:  # the cells the invariant vouches for
                    self.draft.seq_len[s] = max(0, int(hlen[i]) - 2)


class SpecDecodeGraph(_SpecState):
    """The captured speculative step of ``n_seq`` sequences x ``k`` drafts (``rows = n_seq * (k + 1)
    <= DECODE_MAX_ROWS``, mode "full": one stage with the whole lm_head):

        ``lsa_spec_draft`` -> ``embed`` -> layers -> head -> ``lsa_spec_accept``

    with the greedy head (fused arg-max keys -> ``argmax_finalize`` into ``cand``) or, with
    ``sampling=True``, bf16 logits -> ``lsa_sample`` (counter ``pos + 1``) -> ``argmax_finalize``;
    the logits buffer (``rows x head_rows`` bf16) exists only then. ``ngram = (nmin, nmax)``:
    lookup drafts; ``script=True``: drafts from :meth:`set_script` (the hook for an external draft
    source). ``history_len``: steps of accepted counts kept on the device. Admit the sequences, then
    :meth:`capture`, then :meth:`replay` any number of times without a host sync; replays after
    every sequence is done change nothing but scratch.

    ``draft=``: a whole model on one stage (all layers, embedding, the whole lm_head; any
    ``weight_dtype``) with the target's ``vocab_size``, ``max_seq`` at least the target's and the
    graph's slot ids; ``lsa_spec_draft`` is replaced by ``lsa_spec_dm_begin`` and ``k`` greedy draft
    iterations on the same stream (module docstring), on two scratch sets of the draft engine's own
    (2 rows and 1 row per sequence). ``ngram`` is ignored then; ``script=True`` is refused."""

    DRAFT_SCRATCH = ("spec-draft-2", "spec-draft-1")  # StageEngine.decode_scratch keys of the draft engine

    def __init__(self, eng: StageEngine, n_seq: int, k: int, slots: Optional[list] = None, ngram=(1, 3),
                 script: bool = False, sampling: bool = False, history_len: int = 0, eos_ids=(),
                 draft: Optional[StageEngine] = None):
        from ..ops import hip
        if not eng.gpu:
            raise RuntimeError("SpecDecodeGraph needs a GPU stage (EagerSpecDecode runs on the CPU)")
        super().__init__(eng, n_seq, k, slots, ngram, script, sampling, history_len, eos_ids, draft)
        dev, n, rows = eng.device, self.n_seq, self.rows
        i32 = lambda *shape, fill=0: torch.full(shape, fill, dtype=torch.int32, device=dev)  # noqa: E731
        park = self.max_seq - self.k
        self.hist = i32(n, self.ld)
        self.hlen, self.limit, self.done = i32(n, fill=park), i32(n, fill=park), i32(n, fill=1)
        self.eos = torch.from_numpy(self.eos_np).to(dev)
        self.script = i32(n, self.ld) if self.use_script else None
        self.tokens, self.pos, self.cand = i32(rows), i32(rows), i32(rows)
        self.slot = torch.tensor(self.slot_rows, dtype=torch.int32, device=dev)
        self.keys = torch.zeros(rows, dtype=torch.int64, device=dev)
        self.n_acc, self.matched, self.match_ctr = i32(n), i32(n), i32(n)
        self.acc_history = i32(self.history_len, n) if self.history_len else None
        self.step_ctr = i32(1)
        self.logits = None
        if self.sampling:
            self.sampler = Sampler(eng)
            self.logits = torch.zeros((rows, eng.cfg.head_rows), dtype=torch.bfloat16, device=dev)
            for name, v in device_params([GREEDY] * rows, dev).items():
                setattr(self, name, v)
        self.graph = None
        self._hip = hip
        if draft is not None:
            self.slots_t = torch.tensor(self.slots, dtype=torch.int32, device=dev)
            self.d_tokens, self.d_pos, self.d_slot = i32(2 * n), i32(2 * n), i32(2 * n)
            self.d_slot.copy_(self.slots_t.repeat_interleave(2))  # what lsa_spec_dm_begin rewrites every step
            self.d_tokens1, self.d_pos1, self.d_amax = i32(n), i32(n), i32(n)
            self.d_last = torch.arange(1, 2 * n, 2, dtype=torch.int32, device=dev)  # each pair's second row
            self.d_keys = torch.zeros(n, dtype=torch.int64, device=dev)
            for key in self.DRAFT_SCRATCH:
                draft.decode_scratch(key)  # allocated before any capture

    def _put(self, i, hist_row, hlen, limit, done) -> None:
        self.hist[i].copy_(torch.from_numpy(hist_row))
        self.hlen[i], self.limit[i], self.done[i] = hlen, limit, done
        if self.sampling:
            p, r = self.params[i], slice(i * (self.k + 1), (i + 1) * (self.k + 1))
            self.temperature[r], self.top_k[r], self.top_p[r] = p.temperature, p.top_k, p.top_p
            self.seed[r] = S.seed_to_i64(p.seed)

    def _put_script(self, i, row) -> None:
        self.script[i].copy_(torch.from_numpy(row))

    def host_state(self) -> dict:
        return {"hist": self.hist.cpu().numpy(), "hlen": self.hlen.cpu().numpy(), "done": self.done.cpu().numpy(),
                "acc_history": None if self.acc_history is None else self.acc_history.cpu().numpy(),
                "steps": int(self.step_ctr.item()), "match_ctr": self.match_ctr.cpu().numpy()}

    def _step(self) -> None:
        hip, eng, rows, k = self._hip, self.eng, self.rows, self.k
        if self.draft is not None:
            self._draft_model()
        else:
            OS.spec_draft(self.hist, self.hlen, k, self.max_seq, self.tokens, self.pos, self.ngram, self.script,
                          self.matched, self.done, self.match_ctr)
        h = eng.buf_h[:rows]
        hip.embed(self.tokens, eng.embed_w, h)
        eng._forward_hip(h, self.slot, self.pos, None, rows, nsplit=eng.decode_nsplit(rows))
        if self.sampling:
            self.sampler.logits_into(h, rows, self.logits)
            S.sample(self.logits, eng.cfg.vocab_size, rows, self.temperature, self.top_k, self.top_p, self.seed,
                     self.pos, self.keys, ctr_add=1)
        else:
            eng.head_gemv(h, rows, self.keys)
        hip.argmax_finalize(self.keys, rows, self.cand, None)  # pos=None: positions are the draft kernel's
        OS.spec_accept(self.hist, self.hlen, self.limit, self.done, self.eos, self.tokens, self.cand, k, self.max_seq,
                       self.n_acc, self.acc_history, self.step_ctr)

    def _draft_model(self) -> None:
        """``dm_begin -> [draft embed -> layers -> head -> argmax_finalize -> dm_chain] x k``: the
        target's ``tokens`` / ``pos`` filled from the draft engine's greedy continuation."""
        hip, d, n, k = self._hip, self.draft, self.n_seq, self.k
        OS.spec_dm_begin(self.hist, self.hlen, self.slots_t, k, self.max_seq, d.max_seq, self.d_tokens, self.d_pos,
                         self.d_slot, self.tokens, self.pos, self.matched, self.done, self.match_ctr)
        for j in range(k):
            rows = 2 * n if j == 0 else n
            with d.use_scratch(self.DRAFT_SCRATCH[min(j, 1)]):
                h = d.buf_h[:rows]
                if j == 0:
                    hip.embed(self.d_tokens, d.embed_w, h)
                    d._forward_hip(h, self.d_slot, self.d_pos, None, rows, nsplit=d.decode_nsplit(rows))
                    d.head_gemv(h, n, self.d_keys, a_rows=self.d_last)
                else:
                    hip.embed(self.d_tokens1, d.embed_w, h)
                    d._forward_hip(h, self.slots_t, self.d_pos1, None, rows, nsplit=d.decode_nsplit(rows))
                    d.head_gemv(h, n, self.d_keys)
            hip.argmax_finalize(self.d_keys, n, self.d_amax, None)  # greedy, no position increment
            OS.spec_dm_chain(self.d_amax, self.hlen, self.hist.stride(0), k, j, self.max_seq, d.max_seq, self.tokens,
                             self.d_tokens1, self.d_pos1)

    _STATE = ("hist", "hlen", "limit", "done", "n_acc", "matched", "match_ctr")

    def capture(self, warmup: bool = True) -> "SpecDecodeGraph":
        """Capture the step. The warm-up run (if any) is undone: every piece of device state is
        restored (the K/V cells it wrote lie at positions ``>= hlen - 1``, which the first replay
        rewrites)."""
        saved = {a: getattr(self, a).clone() for a in self._STATE}
        dev = self.eng.device
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            if warmup:
                self._step()
        torch.cuda.current_stream(dev).wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            self._step()
        self.graph = g
        for a, v in saved.items():
            getattr(self, a).copy_(v)
        self.keys.zero_()
        if self.draft is not None:
            self.d_keys.zero_()
        self.step_ctr.zero_()
        if self.acc_history is not None:
            self.acc_history.zero_()
        return self

    def replay(self) -> None:
        self.graph.replay()


class EagerSpecDecode(_SpecState):
    """:class:`SpecDecodeGraph`'s interface without a graph: the numpy references around
    ``eng.embed`` / ``eng.forward`` / ``eng.head`` (``Sampler.sample`` with ``positions = pos + 1``
    for sampled sequences). CPU engines run this; on a GPU engine it issues the same forward and
    head launches as the graph and serves as its twin in tests. ``draft=``: as for the graph;
    ``ops.speculative.draft_model_reference`` around the draft engine's ``embed / forward / head``
    (``ngram`` is ignored then)."""

    def __init__(self, eng: StageEngine, n_seq: int, k: int, slots: Optional[list] = None, ngram=(1, 3),
                 script: bool = False, sampling: bool = False, history_len: int = 0, eos_ids=(),
                 draft: Optional[StageEngine] = None):
        super().__init__(eng, n_seq, k, slots, ngram, script, sampling, history_len, eos_ids, draft)
        n, park = self.n_seq, self.max_seq - self.k
        self.hist = np.zeros((n, self.ld), dtype=np.int32)
        self.hlen, self.limit = np.full(n, park, dtype=np.int32), np.full(n, park, dtype=np.int32)
        self.done = np.ones(n, dtype=np.int32)
        self.script = np.zeros((n, self.ld), dtype=np.int32) if self.use_script else None
        self.n_acc, self.matched, self.match_ctr = (np.zeros(n, dtype=np.int32) for _ in range(3))
        self.acc_history = np.zeros((self.history_len, n), dtype=np.int32) if self.history_len else None
        self.step_ctr = np.zeros(1, dtype=np.int32)
        self.sampler = Sampler(eng) if self.sampling else None
        self.tokens = self.pos = self.cand = None

    def _put(self, i, hist_row, hlen, limit, done) -> None:
        self.hist[i] = hist_row
        self.hlen[i], self.limit[i], self.done[i] = hlen, limit, done

    def _put_script(self, i, row) -> None:
        self.script[i] = row

    def host_state(self) -> dict:
        return {"hist": self.hist, "hlen": self.hlen, "done": self.done, "acc_history": self.acc_history,
                "steps": int(self.step_ctr[0]), "match_ctr": self.match_ctr}

    def capture(self, warmup: bool = True) -> "EagerSpecDecode":
        return self

    def _draft_rows(self, tokens, pos, slot, out_rows) -> np.ndarray:
        """One draft iteration: the draft engine's greedy token of every row of ``out_rows``."""
        d = self.draft
        h = d.forward(d.embed(torch.from_numpy(tokens)), slot.tolist(), pos.tolist())
        return d.head(h, [int(r) for r in out_rows]).cpu().numpy().astype(np.int32)

    def replay(self) -> None:
        eng, k = self.eng, self.k
        if self.draft is not None:
            self.tokens, self.pos, self.matched, _ = OS.draft_model_reference(
                self.hist, self.hlen, k, self.max_seq, self.draft.max_seq, self._draft_rows, self.slots, self.done,
                self.match_ctr)
        else:
            self.tokens, self.pos, self.matched = OS.draft_reference(
                self.hist, self.hlen, k, self.max_seq, self.ngram, self.script, self.done, self.match_ctr)
        h = eng.embed(torch.from_numpy(self.tokens))
        h = eng.forward(h, self.slot_rows, self.pos.tolist())
        if self.sampling:
            rows_params = [p for p in self.params for _ in range(k + 1)]
            cand = self.sampler.sample(h, None, rows_params, [int(p) + 1 for p in self.pos])
        else:
            cand = eng.head(h)
        self.cand = cand.cpu().numpy().astype(np.int32)
        self.n_acc = OS.accept_reference(self.hist, self.hlen, self.limit, self.done, self.eos_np, self.tokens,
                                         self.cand, k, self.max_seq, self.acc_history, self.step_ctr)


def generate_speculative(eng: StageEngine, prompts: Sequence[Sequence[int]], max_new_tokens: int, k: int = 3,
                         sampling=None, eos_ids=None, ngram=(1, 3), script=None,
                         draft: Optional[StageEngine] = None) -> tuple:
    """Prefill ``prompts`` (up to their last token) into slots ``0 .. n - 1`` of ``eng`` and decode
    speculatively - the first step feeds the last prompt token - until every sequence has
    ``max_new_tokens`` tokens or has produced an id of ``eos_ids`` (None: no stop ids).
    ``sampling``: None, one :class:`SamplingParams` or one per prompt. ``script``: one token list
    per prompt, indexed by absolute position - drafts come from it instead of the lookup.
    ``draft``: a draft engine (:class:`SpecDecodeGraph`) - drafts come from its greedy continuation,
    ``ngram`` is ignored, ``matched_fraction`` is 1 and a ``script`` beside it is refused; its slots
    ``0 .. n - 1`` are prefilled here. The
    default ``k = 3`` is the largest measured ``k`` whose step stays within 3 % of the 1-row step at
    contexts 128 and 2048 (profiles/speculative.md).

    Returns ``(outputs, stats)``: the generated tokens per prompt, and ``steps`` (of the longest
    running sequence), ``tokens``, ``mean_accepted`` (tokens per step and sequence),
    ``matched_fraction`` (share of those steps whose draft came from a match) and ``accepted``
    (the per-step counts per sequence)."""
    n, new = len(prompts), int(max_new_tokens)
    if n < 1 or n > eng.max_slots:
        raise ValueError(f"generate_speculative: {n} prompts for {eng.max_slots} slots")
    params = list(sampling) if isinstance(sampling, (list, tuple)) else [sampling] * n
    params = [GREEDY if p is None else p for p in params]
    if len(params) != n:
        raise ValueError(f"generate_speculative: {len(params)} sampling parameters for {n} prompts")
    sampled = any(not p.greedy for p in params)
    cls = SpecDecodeGraph if eng.gpu else EagerSpecDecode
    g = cls(eng, n, k, ngram=ngram, script=script is not None, sampling=sampled, history_len=max(1, new),
            eos_ids=eos_ids or (), draft=draft)
    prompts = [[int(t) for t in p] for p in prompts]
    if any(len(p) < 1 for p in prompts):
        raise ValueError("generate_speculative: an empty prompt")
    for i, p in enumerate(prompts):  # refuse before any work
        if len(p) + new + g.k > eng.max_seq:
            raise ValueError(f"speculative: prompt {len(p)} + max_new_tokens {new} + k {g.k} exceeds max_seq {eng.max_seq}")
    eng.reset(list(range(n)))
    for i, p in enumerate(prompts):  # all but the last prompt token: the first step feeds that one
        for c0 in range(0, len(p) - 1, eng.max_prefill_rows):
            chunk = p[c0:min(c0 + eng.max_prefill_rows, len(p) - 1)]
            slot, pos = eng.prefill_rows([i], [len(chunk)])
            eng.forward(eng.embed(torch.tensor(chunk, dtype=torch.int64)), slot, pos)
            eng.advance([i], [len(chunk)])
        g.admit(i, p, new, params[i], n_prompt=len(p))
        if script is not None:
            g.set_script(i, script[i])
    g.capture()
    while True:
        st = g.host_state()
        if st["done"].all():
            break
        # the fewest steps that can finish the longest remaining sequence, then look again
        remaining = max(g.limits[i] - int(st["hlen"][i]) for i in range(n) if not st["done"][i])
        for _ in range(max(1, -(-remaining // (g.k + 1)))):
            g.replay()
    g.sync_positions()
    res = g.results()
    seq_steps = sum(len(r["accepted"]) for r in res)
    tokens = sum(sum(r["accepted"]) for r in res)
    stats = {"steps": max(len(r["accepted"]) for r in res), "tokens": tokens, "mean_accepted": tokens / max(1, seq_steps),
             "matched_fraction": sum(r["matched"] for r in res) / max(1, seq_steps),
             "accepted": [r["accepted"] for r in res]}
    return [r["tokens"] for r in res], stats


__all__ = ["SpecDecodeGraph", "EagerSpecDecode", "generate_speculative"]
