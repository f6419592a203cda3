"""Seeded temperature / top-k / top-p sampling on top of :class:`StageEngine`.

Greedy decode (``StageEngine.head``, ``DecodeGraph``) is untouched: everything here is an extra
path that exists only when a request asks for it.

* :class:`SamplingParams` - one request's ``temperature / top_k / top_p / seed``.
* :class:`Sampler` - bf16 logits of selected rows through the existing lm_head kernels
  (``EPI_STORE``) and one sampled token per row (``ops.sampling.sample``; the fp64 reference on
  a CPU engine). Used for the first token after a prefill.
* :class:`SamplingDecodeGraph` - a :class:`DecodeGraph` whose step ends in logits ->
  ``lsa_sample`` -> ``argmax_finalize`` instead of the fused argmax, with per-row parameters on
  the device (:meth:`SamplingDecodeGraph.set_params` between replays).
* :class:`EagerSamplingDecode` - the same interface for CPU engines.
* :class:`PenaltyState` - the per-slot token statistics of the repetition / presence / frequency
  penalties (``ops.penalties``); it exists only once a request asks for a penalty, and a graph or
  Sampler built without it runs exactly the code above.
* :class:`ConstraintState` - the automaton arena and the per-slot tables of constrained decoding
  (``ops.constraints``: logit bias, banned tokens, ``min_tokens``, min-p, token automata); it
  exists only once a request asks for one of them, and a graph or Sampler built without it runs
  exactly the code above. The order is penalise -> process -> sample -> logprobs.
* :class:`GrammarState` - the byte-level DFA arena, the vocabulary's byte strings and the per-slot
  states of regex-constrained decoding (``ops.grammar``, ``SamplingParams.regex``); it exists only
  once a request carries a regex, and a graph or Sampler built without it runs exactly the code
  above. With it the order is penalise -> grammar mask -> process -> sample -> logprobs: min-p sees
  the masked row.
* Log-probabilities (``SamplingParams.logprobs``, ``ops.logprobs``): :meth:`Sampler.logprobs`,
  ``SamplingDecodeGraph(..., logprobs=True)`` (one ``lsa_logprobs`` launch behind
  ``argmax_finalize``; a graph built without it captures exactly the step above) and
  :func:`score_prompt`. The numbers describe the bf16 row ``lsa_sample`` reads: after the
  penalties, before temperature and the top-k / top-p filters.

A request's tokens depend only on its own logits, seed and positions (the noise is a pure
function of seed, position and vocabulary index), not on the row, slot or batch it runs in.
"""
from __future__ import annotations

import math
import numbers
import os
from dataclasses import dataclass
from typing import Any, Optional, Sequence

import numpy as np
import torch

from ..ops import constraints as K
from ..ops import grammar as G
from ..ops import logprobs as LP
from ..ops import penalties as P
from ..ops import sampling as S
from .engine import DecodeGraph, EagerDecode, StageEngine


@dataclass
class SamplingParams:
    """``temperature == 0`` is greedy (the filters are then ignored). ``top_k == 0`` and
    ``top_p == 1`` switch the filters off. ``seed=None`` draws 64 bits from ``os.urandom`` and
    stores them, so any run can be replayed from ``params.seed``. ``repetition_penalty`` (HF's,
    over prompt + generated tokens; 1 = off), ``presence_penalty`` and ``frequency_penalty``
    (OpenAI / vLLM's, over generated tokens; 0 = off) edit the logits before the filters and the
    draw - also at temperature 0, which then takes the arg-max of the penalised logits.
    ``logprobs`` (None = off): ``0`` returns the chosen token's log-probability and rank, ``1..20``
    also that many most likely alternatives - of the penalised logits at temperature 1, before the
    top-k / top-p filters.

    Constrained decoding (``ops.constraints``; every field off by default): ``logit_bias`` (token ->
    a finite value or ``-inf``, added to the logit) and ``banned_token_ids`` (a bias of ``-inf``)
    share 320 entries; ``min_tokens`` masks every EOS id of the configuration until that many
    tokens have been generated; ``min_p`` in (0, 1] masks tokens with ``p_i < min_p * p_max`` at
    the request's temperature (ignored at temperature 0); ``allowed_token_ids`` (only these tokens
    - include EOS if the output may end), ``choices`` (the output is exactly one of these token-id
    sequences, then EOS) and ``automaton`` (an explicit :class:`ops.constraints.TokenAutomaton`,
    the hook of an external regex / grammar compiler) exclude one another, and ``banned_token_ids``,
    a ``-inf`` bias and ``min_tokens``: the automaton decides what may appear and when the output
    ends, so a row can never lose every column.

    ``regex`` (``ops.grammar``): the output, as bytes, fully matches this pattern - compiled here
    into a byte-level DFA (:attr:`grammar`), so a syntax error surfaces at construction. It excludes
    ``allowed_token_ids``, ``choices``, ``automaton``, ``banned_token_ids``, a ``-inf`` bias and
    ``min_tokens`` for the same reason; a finite ``logit_bias``, ``min_p``, the penalties, top-k /
    top-p and ``logprobs`` combine with it."""
    temperature: float = 0.0
    top_k: int = 0
    top_p: float = 1.0
    seed: Optional[int] = None
    repetition_penalty: float = 1.0
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    logprobs: Optional[int] = None
    logit_bias: Optional[dict] = None
    banned_token_ids: Optional[list] = None
    min_tokens: int = 0
    min_p: Optional[float] = None
    allowed_token_ids: Optional[list] = None
    choices: Optional[list] = None
    automaton: Optional[Any] = None
    regex: Optional[str] = None

    def __post_init__(self):
        self._check_constraints()
        self._grammar = None
        if self.regex is not None:
            if not isinstance(self.regex, str):
                raise ValueError(f"regex must be a str, got {self.regex!r}")
            clash = [k for k in ("allowed_token_ids", "choices", "automaton", "banned_token_ids")
                     if getattr(self, k) is not None]
            if self.min_tokens:
                clash.append("min_tokens")
            if any(b == float("-inf") for _, b in self.bias_entries()) and "banned_token_ids" not in clash:
                clash.append("a -inf bias")
            if clash:
                raise ValueError(f"regex cannot be combined with {' / '.join(clash)}: the pattern decides what may "
                                 "appear and when the output ends")
            self._grammar = _compile_regex(self.regex)
        self.temperature, self.top_k, self.top_p = float(self.temperature), int(self.top_k), float(self.top_p)
        if not self.temperature >= 0.0 or self.temperature == float("inf"):
            raise ValueError(f"temperature must be a finite value >= 0, got {self.temperature}")
        if self.top_k < 0 or self.top_k >= 1 << 31:
            raise ValueError(f"top_k must be >= 0 (0 = off), got {self.top_k}")
        if not 0.0 < self.top_p <= 1.0:
            raise ValueError(f"top_p must be in (0, 1], got {self.top_p}")
        if self.seed is None:
            self.seed = int.from_bytes(os.urandom(8), "little")
        self.seed = int(self.seed)
        if not 0 <= self.seed < 1 << 64:
            raise ValueError(f"seed must be a 64-bit unsigned value, got {self.seed}")
        self.repetition_penalty = float(self.repetition_penalty)
        self.presence_penalty, self.frequency_penalty = float(self.presence_penalty), float(self.frequency_penalty)
        if not 0.0 < self.repetition_penalty < float("inf"):
            raise ValueError(f"repetition_penalty must be a finite value > 0 (1 = off), got {self.repetition_penalty}")
        for k in ("presence_penalty", "frequency_penalty"):
            if not abs(getattr(self, k)) < float("inf"):
                raise ValueError(f"{k} must be finite (0 = off), got {getattr(self, k)}")
        if self.logprobs is not None:
            lp = self.logprobs
            if isinstance(lp, bool) or not isinstance(lp, numbers.Integral) or not 0 <= lp <= LP.TOP_MAX:
                raise ValueError(f"logprobs must be None (off) or an integer in [0, {LP.TOP_MAX}], got {lp!r}")
            self.logprobs = int(lp)

    @property
    def greedy(self) -> bool:
        return self.temperature == 0.0

    @property
    def penalized(self) -> bool:
        return self.repetition_penalty != 1.0 or self.presence_penalty != 0.0 or self.frequency_penalty != 0.0

    def _check_constraints(self) -> None:
        """The checks of the constraint fields that need no vocabulary (``compile_constraints``
        does the rest against a configuration)."""
        def ids(x, what):
            if isinstance(x, (str, bytes)) or not hasattr(x, "__iter__"):
                raise ValueError(f"{what} must be a list of token ids, got {x!r}")
            out = []
            for t in x:
                if isinstance(t, bool) or not isinstance(t, numbers.Integral) or t < 0:
                    raise ValueError(f"{what}: token ids are integers >= 0, got {t!r}")
                out.append(int(t))
            return out

        if self.logit_bias is not None:
            if not isinstance(self.logit_bias, dict):
                raise ValueError(f"logit_bias must be a dict of token id -> bias, got {self.logit_bias!r}")
            lb = {}
            for k, v in self.logit_bias.items():
                try:
                    t, b = int(k), float(v)
                except (TypeError, ValueError):
                    raise ValueError(f"logit_bias: token id -> number, got {k!r}: {v!r}") from None
                if t < 0 or isinstance(k, (bool, float)):
                    raise ValueError(f"logit_bias: token ids are integers >= 0, got {k!r}")
                if math.isnan(b) or b == float("inf"):
                    raise ValueError(f"logit_bias[{t}] must be finite or -inf, got {b}")
                lb[t] = b
            self.logit_bias = lb or None
        if self.banned_token_ids is not None:
            self.banned_token_ids = sorted(set(ids(self.banned_token_ids, "banned_token_ids"))) or None
        if len(self.bias_entries()) > K.BIAS_MAX:
            raise ValueError(f"logit_bias and banned_token_ids together hold {len(self.bias_entries())} entries, more "
                             f"than {K.BIAS_MAX}")
        mt = self.min_tokens
        if isinstance(mt, bool) or not isinstance(mt, numbers.Integral) or not 0 <= mt < 1 << 30:
            raise ValueError(f"min_tokens must be an integer >= 0, got {mt!r}")
        self.min_tokens = int(mt)
        if self.min_p is not None:
            self.min_p = float(self.min_p)
            if not 0.0 < self.min_p <= 1.0:
                raise ValueError(f"min_p must be in (0, 1], got {self.min_p}")
        if self.allowed_token_ids is not None:
            self.allowed_token_ids = sorted(set(ids(self.allowed_token_ids, "allowed_token_ids")))
            if not self.allowed_token_ids:
                raise ValueError("allowed_token_ids: at least one token")
        if self.choices is not None:
            if isinstance(self.choices, (str, bytes)) or not hasattr(self.choices, "__iter__"):
                raise ValueError("choices must be a list of token-id sequences")
            self.choices = [ids(c, "choices") for c in self.choices]
            if not self.choices or any(not c for c in self.choices):
                raise ValueError("choices: at least one choice, and no empty choice")
        if self.automaton is not None and not isinstance(self.automaton, K.TokenAutomaton):
            raise ValueError("automaton must be an ops.constraints.TokenAutomaton")
        kinds = [k for k in ("allowed_token_ids", "choices", "automaton") if getattr(self, k) is not None]
        if len(kinds) > 1:
            raise ValueError(f"at most one of allowed_token_ids / choices / automaton, got {kinds}")
        if kinds and (self.min_tokens or any(b == float("-inf") for _, b in self.bias_entries())):
            raise ValueError(f"{kinds[0]} cannot be combined with banned_token_ids, a -inf bias or min_tokens: the "
                             "automaton decides what may appear and when the output ends")

    def bias_entries(self) -> list:
        """``[(token, bias)]`` of ``logit_bias`` and ``banned_token_ids`` (``-inf``; a ban wins),
        distinct tokens in ascending order."""
        e = dict(self.logit_bias or {})
        e.update({int(t): float("-inf") for t in self.banned_token_ids or ()})
        return sorted(e.items())

    @property
    def constrained(self) -> bool:
        """Any constraint field is on: the request needs a :class:`ConstraintState`."""
        return bool(self.logit_bias or self.banned_token_ids or self.min_tokens or self.min_p is not None
                    or self.allowed_token_ids is not None or self.choices is not None or self.automaton is not None)

    @property
    def grammar(self):
        """The compiled :class:`ops.grammar.ByteDFA` of ``regex`` (None without one): the request
        needs a :class:`GrammarState`."""
        return self._grammar

    @property
    def plain(self) -> bool:
        """Needs no sampling path at all: temperature 0, every penalty off, no logprobs, no
        constraint, no regex."""
        return (self.greedy and not self.penalized and self.logprobs is None and not self.constrained
                and self._grammar is None)

    @property
    def n_top(self) -> int:
        """The row's ``n_top`` of ``lsa_logprobs``: -1 (skip the row) without ``logprobs``."""
        return -1 if self.logprobs is None else self.logprobs

    @classmethod
    def from_dict(cls, d: dict) -> Optional["SamplingParams"]:
        """``temperature / top_k / top_p / seed / repetition_penalty / presence_penalty /
        frequency_penalty / logprobs / logit_bias / banned_token_ids / min_tokens / min_p /
        allowed_token_ids / choices / regex`` keys of a request dict (``logit_bias`` with string or integer
        keys); None (greedy) when none of them is present."""
        keys = ("temperature", "top_k", "top_p", "seed", "repetition_penalty", "presence_penalty", "frequency_penalty",
                "logprobs", "logit_bias", "banned_token_ids", "min_tokens", "min_p", "allowed_token_ids", "choices",
                "regex")
        if not any(d.get(k) is not None for k in keys):
            return None
        return cls(**{k: d[k] for k in keys if d.get(k) is not None})


_REGEX_CACHE: dict = {}


def _compile_regex(pattern: str):
    """``ByteDFA.from_regex`` behind a small cache: a ByteDFA is immutable, and servers see the same
    patterns again and again."""
    dfa = _REGEX_CACHE.get(pattern)
    if dfa is None:
        dfa = G.ByteDFA.from_regex(pattern)
        if len(_REGEX_CACHE) >= 256:
            _REGEX_CACHE.pop(next(iter(_REGEX_CACHE)))
        _REGEX_CACHE[pattern] = dfa
    return dfa


GREEDY = SamplingParams(0.0, 0, 1.0, 0)


def _check_full_head(eng: StageEngine) -> None:
    if eng.lm_head is None:
        raise RuntimeError("[ERROR] this stage has no lm_head")
    if (eng.head_v0, eng.head_v1) != (0, eng.cfg.head_rows):
        raise NotImplementedError("sampling needs the whole lm_head on one stage: this stage holds only vocabulary "
                                  f"rows [{eng.head_v0}, {eng.head_v1}) of {eng.cfg.head_rows} (split head)")


class PenaltyState:
    """The token statistics of the penalties: ``uint16 [n_slots, head_rows]`` on the engine's
    device (bit 15: the token occurs in the slot's prompt; bits 0..14: how often it has been
    generated, saturating) - 32.8 MB at 512 slots x 32000. Built when the first penalised
    request arrives, like the logits buffer. torch stores the table as int16 (same bits)."""

    def __init__(self, eng: StageEngine, n_slots: int):
        _check_full_head(eng)
        self.eng, self.n_slots = eng, int(n_slots)
        self.state = torch.zeros((self.n_slots, eng.cfg.head_rows), dtype=torch.int16, device=eng.device)

    def admit(self, slot: int, prompt_ids) -> None:
        """A penalised request enters ``slot``: zero its row, set the prompt bits."""
        if not 0 <= slot < self.n_slots:
            raise ValueError(f"slot {slot} outside the penalty table of {self.n_slots}")
        ids = torch.as_tensor([int(t) for t in prompt_ids], dtype=torch.long, device=self.state.device)
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= self.eng.cfg.vocab_size):
            raise ValueError("prompt token outside the vocabulary")
        row = self.state[slot]
        row.zero_()
        row[ids] = -0x8000  # int16 pattern of bit 15

    def counts(self, slot: int) -> torch.Tensor:
        """Generated-token counts of ``slot`` (int32 [vocab_size], on the host)."""
        return (self.state[slot, :self.eng.cfg.vocab_size].cpu().to(torch.int32) & P.COUNT_MAX)

    def apply(self, logits: torch.Tensor, slots, tokens_in, params_list: Sequence["SamplingParams"]) -> torch.Tensor:
        """Count ``tokens_in[i]`` (None: nothing) into ``slots[i]`` and penalise row i of bf16
        ``logits`` [n, >= vocab_size] by ``params_list[i]``: ``lsa_penalize`` in place on the GPU,
        the numpy reference on a CPU engine. Returns the penalised logits."""
        n, V = logits.shape[0], self.eng.cfg.vocab_size
        slots = [int(s) for s in slots]
        if len(slots) != n or len(params_list) != n or (tokens_in is not None and len(tokens_in) != n):
            raise ValueError(f"penalties: {n} rows, {len(slots)} slots, {len(params_list)} params")
        if len(set(slots)) != n or any(not 0 <= s < self.n_slots for s in slots):
            raise ValueError(f"penalties: slots {slots} must be distinct and below {self.n_slots}")
        rep, pres, freq = ([getattr(p, k) for p in params_list]
                           for k in ("repetition_penalty", "presence_penalty", "frequency_penalty"))
        if not self.eng.gpu:
            out, st = P.penalize_reference(logits.to(torch.bfloat16), V, self.state, slots, tokens_in, rep, pres, freq)
            self.state.copy_(torch.from_numpy(st.view("int16")))
            return out
        dev = self.eng.device
        f32 = lambda x: torch.tensor(x, dtype=torch.float32, device=dev)  # noqa: E731
        tin = None if tokens_in is None else torch.tensor([int(t) for t in tokens_in], dtype=torch.int32, device=dev)
        P.penalize(logits, V, n, torch.tensor(slots, dtype=torch.int32, device=dev), tin, self.state,
                   f32(rep), f32(pres), f32(freq))
        return logits


@dataclass
class CompiledConstraint:
    """One request's constraint fields against a configuration: what :meth:`ConstraintState.admit`
    writes into a slot."""
    automaton: Optional[K.TokenAutomaton]
    bias_tok: list
    bias_val: list
    min_tokens: int
    minp_delta: float  # float32(T * ln(min_p)); -inf = off


def compile_constraints(params: SamplingParams, vocab_size: int, eos_ids) -> CompiledConstraint:
    """The checks of ``params``' constraint fields that need the vocabulary and the EOS ids
    (ValueError), the automaton of ``allowed_token_ids`` / ``choices``, and ``minp_delta``."""
    V, eos = int(vocab_size), [int(e) for e in eos_ids or ()]
    if len(eos) > K.N_EOS:
        raise ValueError(f"constraints: at most {K.N_EOS} EOS ids, the configuration has {len(eos)}")
    entries = params.bias_entries()
    if any(t >= V for t, _ in entries):
        raise ValueError(f"logit_bias / banned_token_ids: token outside the vocabulary [0, {V})")
    auto = params.automaton
    if params.allowed_token_ids is not None:
        auto = K.TokenAutomaton.from_allowed(params.allowed_token_ids, V)
    elif params.choices is not None:
        auto = K.TokenAutomaton.from_choices(params.choices, V, eos)
    elif auto is not None and auto.vocab != V:
        raise ValueError(f"automaton: a table over {auto.vocab} tokens for a vocabulary of {V}")
    if auto is None:
        gone = {t for t, b in entries if b == float("-inf")} | set(eos if params.min_tokens else ())
        if len(gone) >= V:
            raise ValueError("banned_token_ids and the EOS ids cover the whole vocabulary")
    delta = float("-inf")
    if params.min_p is not None and params.temperature > 0.0:
        delta = float(np.float32(params.temperature * math.log(params.min_p)))
    return CompiledConstraint(auto, [t for t, _ in entries], [b for _, b in entries], params.min_tokens, delta)


class ConstraintState:
    """The tables of constrained decoding (``ops.constraints``) on the engine's device: the
    automaton arena ``int16 [state_rows, head_rows]`` (one row per automaton state - 256 rows are
    16 MB at a vocabulary of 32000 and 66 MB at 128256), the per-slot rows ``astate / abase / bias_n
    / bias_tok / bias_val / min_until / minp_delta / fault`` and the configuration's EOS ids. Built
    when the first constrained request arrives. ``allocator`` (an :class:`ops.constraints.ArenaAllocator`
    of ``state_rows`` rows, by default a new one) places automata in contiguous row ranges and
    shares them by content digest; an automaton's rows are uploaded when its first request is
    admitted."""

    def __init__(self, eng: StageEngine, n_slots: int, state_rows: int = 256,
                 allocator: Optional[K.ArenaAllocator] = None):
        _check_full_head(eng)
        self.eng, self.n_slots, self.state_rows = eng, int(n_slots), int(state_rows)
        self.alloc = K.ArenaAllocator(self.state_rows) if allocator is None else allocator
        if self.alloc.state_rows != self.state_rows or self.n_slots < 1:
            raise ValueError("ConstraintState: the allocator must cover state_rows rows, and n_slots >= 1")
        dev, n = eng.device, self.n_slots
        self.arena = torch.full((self.state_rows, eng.cfg.head_rows), -1, dtype=torch.int16, device=dev)
        self.astate = torch.full((n,), -1, dtype=torch.int32, device=dev)
        self.abase = torch.zeros(n, dtype=torch.int32, device=dev)
        self.bias_n = torch.zeros(n, dtype=torch.int32, device=dev)
        self.bias_tok = torch.zeros((n, K.BIAS_MAX), dtype=torch.int32, device=dev)
        self.bias_val = torch.zeros((n, K.BIAS_MAX), dtype=torch.float32, device=dev)
        self.min_until = torch.zeros(n, dtype=torch.int32, device=dev)
        self.minp_delta = torch.full((n,), float("-inf"), dtype=torch.float32, device=dev)
        self.fault = torch.zeros(n, dtype=torch.int32, device=dev)
        eos = [int(e) for e in eng.cfg.eos_ids][:K.N_EOS]
        self.eos = torch.tensor(eos + [-1] * (K.N_EOS - len(eos)), dtype=torch.int32, device=dev)
        self.resident: set = set()      # digests whose rows are in the arena
        self.held: dict = {}            # slot -> digest of the automaton it holds

    def compile(self, params: SamplingParams) -> CompiledConstraint:
        return compile_constraints(params, self.eng.cfg.vocab_size, self.eng.cfg.eos_ids)

    def admit(self, slot: int, params: Optional[SamplingParams], prompt_len: int,
              compiled: Optional[CompiledConstraint] = None, acquired: bool = False) -> None:
        """A request enters ``slot``: write its rows and point ``astate`` at its automaton's start
        state. ``compiled`` / ``acquired``: the caller has compiled the fields, and already holds
        the allocator's reference (the server does both when the request is submitted)."""
        if not 0 <= slot < self.n_slots:
            raise ValueError(f"slot {slot} outside the constraint tables of {self.n_slots}")
        self.release(slot)
        if params is None or not params.constrained:
            return
        c = self.compile(params) if compiled is None else compiled
        base = -1
        if c.automaton is not None:
            d = c.automaton.digest
            base = self.alloc.base(d) if acquired else self.alloc.acquire(c.automaton)
            self.held[slot] = d
            if d not in self.resident:
                rows = torch.from_numpy(np.array(c.automaton.next)).to(self.arena.device)
                self.arena[base:base + c.automaton.n_states, :c.automaton.vocab] = rows
                if self.eng.gpu:  # streams other than this one may admit the same automaton next
                    torch.cuda.current_stream(self.arena.device).synchronize()
                self.resident.add(d)
        n = len(c.bias_tok)
        self.abase[slot] = max(base, 0)
        self.astate[slot] = base
        self.bias_n[slot] = n
        if n:
            dev = self.bias_tok.device
            self.bias_tok[slot, :n] = torch.tensor(c.bias_tok, dtype=torch.int32, device=dev)
            self.bias_val[slot, :n] = torch.tensor(c.bias_val, dtype=torch.float32, device=dev)
        self.min_until[slot] = int(prompt_len) + c.min_tokens if c.min_tokens else 0
        self.minp_delta[slot] = c.minp_delta
        self.fault[slot] = 0

    def release(self, slot: int) -> None:
        """Clear ``slot``; the automaton it held loses one reference (``fault`` stays readable
        until the next :meth:`admit`)."""
        d = self.held.pop(slot, None)
        if d is not None and self.alloc.release(d):
            self.resident.discard(d)
        self.astate[slot] = -1
        self.bias_n[slot] = 0
        self.min_until[slot] = 0
        self.minp_delta[slot] = float("-inf")

    def apply(self, logits: torch.Tensor, slots, tokens_in, positions) -> torch.Tensor:
        """Advance ``slots[i]`` by ``tokens_in[i]`` (None: nothing) and process row i of bf16
        ``logits`` [n, >= vocab_size]; ``positions[i]`` is the position the sampled token will
        occupy. ``lsa_logit_process`` in place on the GPU, the numpy reference on a CPU engine.
        Returns the processed logits."""
        n, V = logits.shape[0], self.eng.cfg.vocab_size
        slots = [int(s) for s in slots]
        positions = [int(p) for p in (positions.tolist() if isinstance(positions, torch.Tensor) else positions)]
        if len(slots) != n or len(positions) != n or (tokens_in is not None and len(tokens_in) != n):
            raise ValueError(f"constraints: {n} rows, {len(slots)} slots, {len(positions)} positions")
        if len(set(slots)) != n or any(not 0 <= s < self.n_slots for s in slots):
            raise ValueError(f"constraints: slots {slots} must be distinct and below {self.n_slots}")
        if not self.eng.gpu:
            out, ast, flt = K.logit_process_reference(logits.to(torch.bfloat16), V, self, slots, tokens_in, positions)
            self.astate.copy_(torch.from_numpy(ast))
            self.fault.copy_(torch.from_numpy(flt))
            return out
        dev = self.eng.device
        tin = None if tokens_in is None else torch.tensor([int(t) for t in tokens_in], dtype=torch.int32, device=dev)
        K.logit_process(logits, V, n, torch.tensor(slots, dtype=torch.int32, device=dev), tin,
                        torch.tensor(positions, dtype=torch.int32, device=dev), self)
        return logits


class GrammarState:
    """The tables of regex-constrained decoding (``ops.grammar``) on the engine's device: the DFA
    arena ``int16 [dfa_rows, 256]`` with its ``accept`` bytes (513 B per state whatever the
    vocabulary - 2 MB at the default 4096 rows, where the dense arena of :class:`ConstraintState`
    takes 64 KB per state at a vocabulary of 32000), the vocabulary's byte strings (``offsets``,
    ``data``), the per-slot rows ``gstate / gbase / gfault`` (12 B per slot) and the configuration's
    EOS ids. Built when the first request with a regex arrives. ``allocator`` (an
    :class:`ops.constraints.ArenaAllocator` of ``dfa_rows`` rows, by default a new one) places DFAs
    in contiguous row ranges and shares them by content digest; a DFA's rows are uploaded when its
    first request is admitted."""

    def __init__(self, eng: StageEngine, n_slots: int, vocab: "G.VocabBytes", dfa_rows: int = 4096,
                 allocator: Optional[K.ArenaAllocator] = None):
        _check_full_head(eng)
        self.eng, self.n_slots, self.dfa_rows, self.vocab = eng, int(n_slots), int(dfa_rows), vocab
        if not isinstance(vocab, G.VocabBytes) or vocab.V != eng.cfg.vocab_size:
            raise ValueError(f"GrammarState: a VocabBytes over the configuration's {eng.cfg.vocab_size} tokens, got "
                             f"{getattr(vocab, 'V', None)}")
        self.alloc = K.ArenaAllocator(self.dfa_rows) if allocator is None else allocator
        if self.alloc.state_rows != self.dfa_rows or self.n_slots < 1:
            raise ValueError("GrammarState: the allocator must cover dfa_rows rows, and n_slots >= 1")
        dev, n = eng.device, self.n_slots
        self.arena = torch.full((self.dfa_rows, 256), -1, dtype=torch.int16, device=dev)
        self.accept = torch.zeros(self.dfa_rows, dtype=torch.uint8, device=dev)
        self.offsets = torch.from_numpy(np.array(vocab.offsets)).to(dev)
        self.data = torch.from_numpy(np.array(vocab.data)).to(dev)
        self.gstate = torch.full((n,), -1, dtype=torch.int32, device=dev)
        self.gbase = torch.zeros(n, dtype=torch.int32, device=dev)
        self.gfault = torch.zeros(n, dtype=torch.int32, device=dev)
        self.eos_ids = [int(e) for e in eng.cfg.eos_ids][:K.N_EOS]
        self.eos = torch.tensor(self.eos_ids + [-1] * (K.N_EOS - len(self.eos_ids)), dtype=torch.int32, device=dev)
        self.resident: set = set()      # digests whose rows are in the arena
        self.held: dict = {}            # slot -> digest of the DFA it holds
        self.checked = check_vocab_cache(vocab, self.eos_ids)

    def check(self, dfa: "G.ByteDFA") -> None:
        """ValueError unless every state of ``dfa`` allows at least one token of this vocabulary."""
        self.checked(dfa)

    def admit(self, slot: int, params: Optional[SamplingParams], acquired: bool = False) -> None:
        """A request enters ``slot``: point ``gstate`` at its DFA's start state (uploading the DFA's
        rows when it is new). ``acquired``: the caller already holds the allocator's reference and
        has run :meth:`check` (the server does both when the request is submitted)."""
        if not 0 <= slot < self.n_slots:
            raise ValueError(f"slot {slot} outside the grammar tables of {self.n_slots}")
        self.release(slot)
        dfa = None if params is None else params.grammar
        if dfa is None:
            return
        if not acquired:
            self.check(dfa)
        d = dfa.digest
        base = self.alloc.base(d) if acquired else self.alloc.acquire(dfa)
        self.held[slot] = d
        if d not in self.resident:
            S = dfa.n_states
            flags = dfa.accept.astype(np.uint8) * G.ACCEPT
            flags[S - 1] |= G.LAST
            self.arena[base:base + S] = torch.from_numpy(np.array(dfa.next)).to(self.arena.device)
            self.accept[base:base + S] = torch.from_numpy(flags).to(self.arena.device)
            if self.eng.gpu:  # streams other than this one may admit the same DFA next
                torch.cuda.current_stream(self.arena.device).synchronize()
            self.resident.add(d)
        self.gbase[slot] = base
        self.gstate[slot] = base
        self.gfault[slot] = 0

    def release(self, slot: int) -> None:
        """Clear ``slot``; the DFA it held loses one reference (``gfault`` stays readable until the
        next :meth:`admit`)."""
        d = self.held.pop(slot, None)
        if d is not None and self.alloc.release(d):
            self.resident.discard(d)
        self.gstate[slot] = -1

    def apply(self, logits: torch.Tensor, slots, tokens_in) -> torch.Tensor:
        """Advance ``slots[i]`` by the bytes of ``tokens_in[i]`` (None: nothing) and mask row i of
        bf16 ``logits`` [n, >= vocab_size]: ``lsa_grammar_mask`` in place on the GPU, the numpy
        reference on a CPU engine. Returns the masked logits."""
        n, V = logits.shape[0], self.eng.cfg.vocab_size
        slots = [int(s) for s in slots]
        if len(slots) != n or (tokens_in is not None and len(tokens_in) != n):
            raise ValueError(f"grammar: {n} rows, {len(slots)} slots")
        if len(set(slots)) != n or any(not 0 <= s < self.n_slots for s in slots):
            raise ValueError(f"grammar: slots {slots} must be distinct and below {self.n_slots}")
        if not self.eng.gpu:
            out, gst, flt = G.grammar_mask_reference(logits.to(torch.bfloat16), V, self, slots, tokens_in)
            self.gstate.copy_(torch.from_numpy(gst))
            self.gfault.copy_(torch.from_numpy(flt))
            return out
        dev = self.eng.device
        tin = None if tokens_in is None else torch.tensor([int(t) for t in tokens_in], dtype=torch.int32, device=dev)
        G.grammar_mask(logits, V, n, torch.tensor(slots, dtype=torch.int32, device=dev), tin, self)
        return logits


def check_vocab_cache(vocab: "G.VocabBytes", eos_ids):
    """A function ``check(dfa)`` that raises ValueError unless every state of ``dfa`` allows at least
    one token of ``vocab`` - so a row can never lose every column. First the cheap sufficient test
    (the state accepts and an EOS id exists, or a live byte of it exists as a one-byte token), then,
    only for the states that fail it, the exact vectorised walk. Results are kept per digest."""
    eos = [int(e) for e in eos_ids if 0 <= int(e) < vocab.V]
    ln = np.diff(vocab.offsets)
    one = ln == 1
    one[eos] = False                      # an EOS id's own bytes are ignored
    single = np.zeros(256, dtype=bool)
    single[vocab.data[vocab.offsets[:-1][one]]] = True
    done: dict = {}

    def check(dfa) -> None:
        bad = done.get(dfa.digest)
        if bad is None:
            ok = ((np.asarray(dfa.next) >= 0) & single[None, :]).any(axis=1)
            if eos:
                ok |= np.asarray(dfa.accept)
            bad = -1
            rest = np.nonzero(~ok)[0]
            for c0 in range(0, rest.size, 64):  # the exact walk, 64 states at a time
                alive = dfa.step_tokens(vocab, rest[c0:c0 + 64]) >= 0
                alive[:, eos] = False
                stuck = np.nonzero(~alive.any(axis=1))[0]
                if stuck.size:
                    bad = int(rest[c0 + stuck[0]])
                    break
            if len(done) >= 1024:
                done.pop(next(iter(done)))
            done[dfa.digest] = bad
        if bad >= 0:
            raise ValueError(f"regex {dfa.pattern!r}: state {bad} of its automaton allows no token of this "
                             "vocabulary (no token's bytes continue a match there)")

    return check


class Sampler:
    """Logits and sampled tokens of a stage that holds the whole lm_head. ``penalties``: the
    stage's :class:`PenaltyState`, applied by :meth:`sample` to the rows given ``slots``;
    ``grammar``: its :class:`GrammarState`, applied behind the penalties; ``constraints``: its
    :class:`ConstraintState`, applied behind both."""

    def __init__(self, eng: StageEngine, penalties: Optional[PenaltyState] = None,
                 constraints: Optional[ConstraintState] = None, grammar: Optional[GrammarState] = None):
        _check_full_head(eng)
        self.eng = eng
        self.penalties = penalties
        self.constraints = constraints
        self.grammar = grammar

    # ------------------------------------------------------------------ logits
    def logits(self, h: torch.Tensor, rows_idx=None) -> torch.Tensor:
        """final norm -> lm_head of the selected rows: bf16 ``[n, head_rows]`` (columns
        ``>= vocab_size`` are padding)."""
        eng = self.eng
        if rows_idx is None:
            rows_idx = list(range(h.shape[0]))
        if not eng.gpu:
            hs = h[torch.as_tensor(rows_idx, device=h.device, dtype=torch.long)]
            return eng.logits_torch(hs).to(torch.bfloat16)
        idx = eng._i32(rows_idx)
        out = torch.empty((idx.numel(), eng.cfg.head_rows), dtype=torch.bfloat16, device=eng.device)
        self.logits_into(h, idx.numel(), out, a_rows=idx)
        return out

    def logits_into(self, h: torch.Tensor, rows: int, out: torch.Tensor, a_rows: Optional[torch.Tensor] = None) -> None:
        """GPU: logits of ``rows`` rows of ``h`` (``a_rows``: int32 row gather) into bf16 ``out``
        [>= rows, head_rows], on the existing projection kernels with the EPI_STORE epilogue -
        the kernel family per row count mirrors ``StageEngine.head_gemv``."""
        from ..ops import hip
        eng, cfg = self.eng, self.eng.cfg
        N, H, eps, D = cfg.head_rows, cfg.hidden_size, cfg.rms_norm_eps, eng.DECODE_MAX_ROWS
        if out.dtype != torch.bfloat16 or out.shape[0] < rows or out.shape[1] != N:
            raise ValueError(f"logits_into: out must be bf16 [>= {rows}, {N}]")
        ep = hip.make_epi(out=out, ldo=out.stride(0), bias=eng.head_bias)
        if rows > D and (not cfg.is_gpt2 and eng.lm_head_s is None and eng.sk_ws is not None and N % 128 == 0
                         and rows <= eng.buf_xn.shape[0]):
            xn = eng.buf_xn[:rows]
            src = h[:rows] if a_rows is None else h.index_select(0, a_rows.long())
            hip.rmsnorm(src, None, xn, rows, eps, H)
            hip.gemm_sk(xn, eng.lm_head, rows, N, H, hip.EPI_STORE, ep, ws=eng.sk_ws)
            return
        if rows > D:  # the GEMV kernels take <= 128 rows per launch
            for c0 in range(0, rows, D):
                c = min(D, rows - c0)
                if a_rows is None:
                    self.logits_into(h[c0:c0 + c], c, out[c0:c0 + c])
                else:
                    self.logits_into(h, c, out[c0:c0 + c], a_rows=a_rows[c0:c0 + c])
            return
        if cfg.is_gpt2:  # ln_f (mean + bias) runs as its own kernel in front of a plain GEMV
            xn = eng.buf_xn[:rows]
            src = h if a_rows is None else h.index_select(0, a_rows.long())
            hip.layernorm(src, xn, eng.final_norm, eng.final_norm_b, rows, eps)
            if eng.lm_head_s is not None:
                hip.proj_fp8(xn, eng.lm_head.view(-1), eng.lm_head_s, rows, N, H, hip.EPI_STORE, ep, ws=eng.coop_ws)
            else:
                hip.gemv(xn, eng.lm_head, rows, N, H, hip.EPI_STORE, ep, ws=eng.coop_ws)
            return
        if eng.lm_head_s is not None:
            hip.proj_fp8(h, eng.lm_head.view(-1), eng.lm_head_s, rows, N, H, hip.EPI_STORE, ep, norm=True, eps=eps,
                         a_rows=a_rows, ws=eng.coop_ws)
        else:
            hip.gemv(h, eng.lm_head, rows, N, H, hip.EPI_STORE, ep, ws=eng.coop_ws, norm=True, eps=eps, a_rows=a_rows)

    # ------------------------------------------------------------------ tokens
    def sample_logits(self, logits: torch.Tensor, params_list: Sequence[SamplingParams], positions) -> torch.Tensor:
        """One token per row of bf16 ``logits`` [n, >= vocab_size]; ``positions[i]`` is the
        position the sampled token will occupy (its Philox counter). Returns int64 [n]."""
        eng, V = self.eng, self.eng.cfg.vocab_size
        n = logits.shape[0]
        positions = [int(p) for p in (positions.tolist() if isinstance(positions, torch.Tensor) else positions)]
        if len(params_list) != n or len(positions) != n:
            raise ValueError(f"sample: {n} rows, {len(params_list)} params, {len(positions)} positions")
        if not eng.gpu:
            tok, _, _, _ = S.sample_reference(logits.to(torch.bfloat16), V, [p.temperature for p in params_list],
                                              [p.top_k for p in params_list], [p.top_p for p in params_list],
                                              [p.seed for p in params_list], positions)
            return torch.from_numpy(tok)
        from ..ops import hip
        dev = eng.device
        arr = device_params(params_list, dev)
        ctr = torch.tensor(positions, dtype=torch.int32, device=dev)
        keys = torch.zeros(n, dtype=torch.int64, device=dev)
        S.sample(logits, V, n, arr["temperature"], arr["top_k"], arr["top_p"], arr["seed"], ctr, keys)
        out = torch.empty(n, dtype=torch.int32, device=dev)
        for c0 in range(0, n, 1024):  # argmax_finalize takes <= 1024 rows
            c = min(1024, n - c0)
            hip.argmax_finalize(keys[c0:c0 + c], c, out[c0:c0 + c])
        return out.long()

    def logprobs(self, logits: torch.Tensor, targets, n_top) -> LP.Logprobs:
        """Log-probabilities of bf16 ``logits`` [n, >= vocab_size] (``ops.logprobs``' contract):
        ``targets`` / ``n_top`` per row (or one value for all). ``lsa_logprobs`` on the GPU, the
        fp64 reference on a CPU engine. Returns :class:`ops.logprobs.Logprobs` of torch tensors on
        the logits' device: ``lse`` / ``tok_lp`` fp32 [n], ``tok_rank`` int32 [n], ``top_id`` int32
        and ``top_lp`` fp32 [n, TOP_MAX]; rows with ``n_top = -1`` hold NaN / 0 / -1 / -inf."""
        eng, V, n = self.eng, self.eng.cfg.vocab_size, logits.shape[0]

        def per_row(x):
            x = x.tolist() if isinstance(x, torch.Tensor) else x
            x = [int(v) for v in x] if isinstance(x, (list, tuple)) else [int(x)] * n
            if len(x) != n:
                raise ValueError(f"logprobs: {len(x)} per-row values for {n} rows")
            return x

        targets, n_top = per_row(targets), per_row(n_top)
        if any(k > LP.TOP_MAX for k in n_top):
            raise ValueError(f"logprobs: n_top above {LP.TOP_MAX}")
        if not eng.gpu:
            ref = LP.logprobs_reference(logits.to(torch.bfloat16), V, n_top, targets)
            return LP.Logprobs(torch.from_numpy(ref.lse).float(), torch.from_numpy(ref.tok_lp).float(),
                               torch.from_numpy(ref.tok_rank).int(), torch.from_numpy(ref.top_id).int(),
                               torch.from_numpy(ref.top_lp).float())
        dev = eng.device
        out = LP.alloc_outputs(n, dev)
        nt = torch.tensor(n_top, dtype=torch.int32, device=dev)
        tg = torch.tensor(targets, dtype=torch.int32, device=dev)
        for c0 in range(0, n, 32768):
            c = min(32768, n - c0)
            LP.logprobs(logits[c0:c0 + c], V, c, nt[c0:c0 + c], tg[c0:c0 + c],
                        LP.Logprobs(*(t[c0:c0 + c] for t in out)))
        return out

    def sample(self, h: torch.Tensor, rows_idx, params_list: Sequence[SamplingParams], positions,
               slots=None, tokens_in=None, return_logprobs: bool = False):
        """Sampled tokens (int64 [n]) of the selected rows of the final hidden ``h``: the first
        token after a prefill uses ``positions[i]`` = the prompt length. ``slots`` (with a
        :class:`PenaltyState`): row i belongs to sequence slot ``slots[i]`` and is penalised by
        its parameters first; ``tokens_in[i]`` is the token the row's step was fed (counted as
        generated) - None for the first token after a prefill, which only sees the prompt. With a
        :class:`ConstraintState` the rows of constrained requests are then processed
        (``ops.constraints``: the automaton advances by ``tokens_in[i]``), in the order penalise ->
        process -> sample -> logprobs. With a :class:`GrammarState` the rows whose slots hold a regex
        are masked between the two (``ops.grammar``).
        ``return_logprobs``: returns ``(tokens, Logprobs)`` - the log-probabilities of the sampled
        tokens under the (penalised) logits, for the rows whose parameters ask for them."""
        logits = self.logits(h, rows_idx)
        if any(p.penalized for p in params_list):
            if self.penalties is None or slots is None:
                raise RuntimeError("a penalised request needs a PenaltyState (Sampler(eng, penalties=...)) and slots=")
            logits = self.penalties.apply(logits, slots, tokens_in, params_list)
        if any(p.grammar is not None for p in params_list):
            if self.grammar is None or slots is None:
                raise RuntimeError("a request with a regex needs a GrammarState (Sampler(eng, grammar=...)) and slots=")
            logits = self.grammar.apply(logits, slots, tokens_in)
        if any(p.constrained for p in params_list):
            if self.constraints is None or slots is None:
                raise RuntimeError("a constrained request needs a ConstraintState (Sampler(eng, constraints=...)) and "
                                   "slots=")
            logits = self.constraints.apply(logits, slots, tokens_in, positions)
        tok = self.sample_logits(logits, params_list, positions)
        if not return_logprobs:
            return tok
        return tok, self.logprobs(logits, tok, [p.n_top for p in params_list])


def device_params(params_list: Sequence[SamplingParams], device) -> dict:
    """Per-row device arrays of ``lsa_sample``."""
    return {
        "temperature": torch.tensor([p.temperature for p in params_list], dtype=torch.float32, device=device),
        "top_k": torch.tensor([p.top_k for p in params_list], dtype=torch.int32, device=device),
        "top_p": torch.tensor([p.top_p for p in params_list], dtype=torch.float32, device=device),
        "seed": torch.tensor([S.seed_to_i64(p.seed) for p in params_list], dtype=torch.int64, device=device),
    }


class SamplingDecodeGraph(DecodeGraph):
    """A captured decode step that samples: ... layers -> bf16 logits -> ``lsa_sample`` ->
    ``argmax_finalize`` (modes ``"full"`` and ``"last"``). Every row starts greedy
    (``temperature`` 0: the arg-max of the bf16 logits); :meth:`set_params` writes a row's
    parameters between replays. The row's Philox counter is its device position + 1 - the
    position the sampled token will occupy - so no host work happens per token.

    With ``penalties`` (a :class:`PenaltyState` that covers this graph's slots) the step is logits
    -> ``lsa_penalize`` -> ``lsa_sample``: the kernel counts the step's input tokens
    (``self.tokens``) into the rows' slots and edits the logits by the per-row ``rep / pres / freq``
    device arrays; rows whose penalties are off are skipped. Without it the captured step is
    exactly the one above. ``debug_raw`` keeps a captured copy of the unpenalised logits in
    ``raw_logits``.

    With ``logprobs=True`` the step ends in one more launch, ``lsa_logprobs`` on the same logits
    with the freshly written ``self.tokens`` as targets: the per-row ``n_top`` (-1 = the row is
    skipped, written by :meth:`set_params`) and the outputs ``lp`` (:class:`ops.logprobs.Logprobs`)
    live on the device; with a token history, ``lp_history`` keeps ``tok_lp`` of the same steps
    (NaN where a row was skipped). Without it the captured step is exactly the one above.

    With ``constraints`` (a :class:`ConstraintState` that covers this graph's slots) one
    ``lsa_logit_process`` launch sits between ``lsa_penalize`` and ``lsa_sample``: it advances the
    rows' automaton states by the step's input tokens and applies bias, EOS mask, automaton mask
    and min-p from the per-slot device tables (written by :meth:`ConstraintState.admit`); rows
    whose slots hold no constraint are skipped. The log-probabilities then describe the processed
    row. Without it the captured step is exactly the one above.

    With ``grammar`` (a :class:`GrammarState` that covers this graph's slots) one
    ``lsa_grammar_mask`` launch sits between ``lsa_penalize`` and ``lsa_logit_process``: it advances
    the rows' DFA states by the bytes of the step's input tokens and masks every token whose bytes
    die in the automaton; rows whose slots hold no regex are skipped. Without it the captured step
    is exactly the one above.

    The logits buffer (``rows x head_rows`` bf16, 32 MB at 512 x 32000) is allocated only here."""

    def __init__(self, eng: StageEngine, rows: int, mode: str, slots: Optional[list] = None,
                 history_len: int = 0, scratch: int = 0, penalties: Optional[PenaltyState] = None,
                 debug_raw: bool = False, logprobs: bool = False, constraints: Optional[ConstraintState] = None,
                 grammar: Optional[GrammarState] = None):
        if mode not in ("full", "last"):
            raise ValueError("SamplingDecodeGraph runs the head: mode 'full' or 'last'")
        self.sampler = Sampler(eng, penalties, constraints, grammar)
        super().__init__(eng, rows, mode, slots=slots, history_len=history_len, scratch=scratch)
        dev = eng.device
        self.params = [GREEDY] * rows
        for k, v in device_params(self.params, dev).items():
            setattr(self, k, v)
        self.logits = torch.zeros((rows, eng.cfg.head_rows), dtype=torch.bfloat16, device=dev)
        self.penalties = penalties
        self.raw_logits = torch.zeros_like(self.logits) if debug_raw else None
        if penalties is not None:
            if penalties.eng is not eng or len(set(self.slots)) != rows or max(self.slots) >= penalties.n_slots:
                raise ValueError("penalties: a PenaltyState of this engine with a distinct row per graph slot")
            self.rep = torch.ones(rows, dtype=torch.float32, device=dev)
            self.pres = torch.zeros(rows, dtype=torch.float32, device=dev)
            self.freq = torch.zeros(rows, dtype=torch.float32, device=dev)
        self.constraints = constraints
        if constraints is not None:
            if constraints.eng is not eng or len(set(self.slots)) != rows or max(self.slots) >= constraints.n_slots:
                raise ValueError("constraints: a ConstraintState of this engine with a distinct row per graph slot")
        self.grammar = grammar
        if grammar is not None:
            if grammar.eng is not eng or len(set(self.slots)) != rows or max(self.slots) >= grammar.n_slots:
                raise ValueError("grammar: a GrammarState of this engine with a distinct row per graph slot")
        self.lp = self.n_top = self.lp_history = None
        if logprobs:
            self.n_top = torch.full((rows,), -1, dtype=torch.int32, device=dev)
            self.lp = LP.alloc_outputs(rows, dev)
            if self.history is not None:
                self.lp_history = torch.full(self.history.shape, float("nan"), dtype=torch.float32, device=dev)

    def set_params(self, row: int, params: Optional[SamplingParams]) -> None:
        """Small host-to-device copies on the current stream (like ``set_positions``)."""
        p = GREEDY if params is None else params
        if p.penalized and self.penalties is None:
            raise RuntimeError("a penalised request needs SamplingDecodeGraph(..., penalties=PenaltyState)")
        if p.logprobs is not None and self.lp is None:
            raise RuntimeError("a request with logprobs needs SamplingDecodeGraph(..., logprobs=True)")
        if p.constrained and self.constraints is None:
            raise RuntimeError("a constrained request needs SamplingDecodeGraph(..., constraints=ConstraintState)")
        if p.grammar is not None and self.grammar is None:
            raise RuntimeError("a request with a regex needs SamplingDecodeGraph(..., grammar=GrammarState)")
        self.params[row] = p
        self.temperature[row] = p.temperature
        self.top_k[row] = p.top_k
        self.top_p[row] = p.top_p
        self.seed[row] = S.seed_to_i64(p.seed)
        if self.penalties is not None:
            self.rep[row] = p.repetition_penalty
            self.pres[row] = p.presence_penalty
            self.freq[row] = p.frequency_penalty
        if self.lp is not None:
            self.n_top[row] = p.n_top

    def capture(self, warmup: bool = True) -> "SamplingDecodeGraph":
        """The warm-up run counts tokens into the penalty state and advances the automaton and
        grammar states: the graph's rows are restored."""
        cs, gs = self.constraints, self.grammar
        idx = self.slot.long()
        kept = None if cs is None else (cs.astate.index_select(0, idx), cs.fault.index_select(0, idx))
        gkept = None if gs is None else (gs.gstate.index_select(0, idx), gs.gfault.index_select(0, idx))
        if self.penalties is None:
            super().capture(warmup)
        else:
            saved = self.penalties.state.index_select(0, idx)
            super().capture(warmup)
            self.penalties.state.index_copy_(0, idx, saved)
        if kept is not None:
            cs.astate.index_copy_(0, idx, kept[0])
            cs.fault.index_copy_(0, idx, kept[1])
        if gkept is not None:
            gs.gstate.index_copy_(0, idx, gkept[0])
            gs.gfault.index_copy_(0, idx, gkept[1])
        if self.lp_history is not None:
            self.lp_history.fill_(float("nan"))
        return self

    def _step(self) -> None:
        hip, eng, rows = self._hip, self.eng, self.rows
        h = eng.buf_h[:rows]
        if self.mode == "full":
            hip.embed(self.tokens, eng.embed_w, h)
        else:
            h.copy_(self.h_in)
        eng._forward_hip(h, self.slot, self.pos, None, rows, nsplit=eng.decode_nsplit(rows))
        self.sampler.logits_into(h, rows, self.logits)
        if self.raw_logits is not None:
            self.raw_logits.copy_(self.logits)
        if self.penalties is not None:
            P.penalize(self.logits, eng.cfg.vocab_size, rows, self.slot, self.tokens, self.penalties.state,
                       self.rep, self.pres, self.freq)
        if self.grammar is not None:
            G.grammar_mask(self.logits, eng.cfg.vocab_size, rows, self.slot, self.tokens, self.grammar)
        if self.constraints is not None:
            K.logit_process(self.logits, eng.cfg.vocab_size, rows, self.slot, self.tokens, self.pos, self.constraints,
                            ctr_add=1)
        S.sample(self.logits, eng.cfg.vocab_size, rows, self.temperature, self.top_k, self.top_p, self.seed, self.pos,
                 self.keys, ctr_add=1)
        hip.argmax_finalize(self.keys, rows, self.tokens, self.pos, 1, self.history,
                            self.step_ctr if self.history is not None else None)
        if self.lp is not None:
            LP.logprobs(self.logits, eng.cfg.vocab_size, rows, self.n_top, self.tokens, self.lp,
                        lp_history=self.lp_history, step_ctr=self.step_ctr if self.lp_history is not None else None)


class EagerSamplingDecode(EagerDecode):
    """:class:`SamplingDecodeGraph`'s interface on devices without graphs (CPU engines)."""

    def __init__(self, eng: StageEngine, rows: int, mode: str, slots: Optional[list] = None, history_len: int = 0,
                 penalties: Optional[PenaltyState] = None, logprobs: bool = False,
                 constraints: Optional[ConstraintState] = None, grammar: Optional[GrammarState] = None):
        if mode not in ("full", "last"):
            raise ValueError("EagerSamplingDecode runs the head: mode 'full' or 'last'")
        super().__init__(eng, rows, mode, slots=slots, history_len=history_len)
        self.sampler = Sampler(eng, penalties, constraints, grammar)
        self.penalties = penalties
        self.constraints = constraints
        self.grammar = grammar
        self.params = [GREEDY] * rows
        self.lp = self.lp_history = None
        if logprobs:
            self.lp = self.sampler.logprobs(torch.zeros((rows, eng.cfg.head_rows), dtype=torch.bfloat16), 0, -1)
            if self.history is not None:
                self.lp_history = torch.full(self.history.shape, float("nan"), dtype=torch.float32)

    def set_params(self, row: int, params: Optional[SamplingParams]) -> None:
        p = GREEDY if params is None else params
        if p.logprobs is not None and self.lp is None:
            raise RuntimeError("a request with logprobs needs EagerSamplingDecode(..., logprobs=True)")
        if p.constrained and self.constraints is None:
            raise RuntimeError("a constrained request needs EagerSamplingDecode(..., constraints=ConstraintState)")
        if p.grammar is not None and self.grammar is None:
            raise RuntimeError("a request with a regex needs EagerSamplingDecode(..., grammar=GrammarState)")
        self.params[row] = p

    def _body(self) -> None:
        eng = self.eng
        h = eng.embed(self.tokens) if self.mode == "full" else self.h_in
        slot, pos = eng.prefill_rows(self.slots, [1] * self.rows)
        h = eng.forward(h, slot, pos)
        eng.advance(self.slots, [1] * self.rows)
        pen = {}
        if self.penalties is not None or self.constraints is not None or self.grammar is not None:
            pen = {"slots": self.slots, "tokens_in": self.tokens.tolist()}
        tok = self.sampler.sample(h, None, self.params, [p + 1 for p in pos], return_logprobs=self.lp is not None,
                                  **pen)
        if self.lp is not None:
            tok, self.lp = tok
        self.tokens.copy_(tok.to(torch.int32))
        if self.history is not None and self.step < self.history.shape[0]:
            self.history[self.step] = self.tokens
            if self.lp_history is not None:
                self.lp_history[self.step] = self.lp.tok_lp
        self.step += 1
        self._out = h

    replay = _body


SCORE_CHUNK_BYTES = 64 << 20  # score_prompt: no more logits than this exist at once


def score_prompt(eng: StageEngine, ids, top: int = 0, slot: int = 0):
    """Teacher-forced log-probabilities of a prompt: prefills ``ids`` into KV slot ``slot`` (from
    position 0) and returns :class:`ops.logprobs.Logprobs` of host tensors with ``len(ids) - 1``
    rows - ``tok_lp[t] = log p(ids[t + 1] | ids[..t])`` (fp32), ``tok_rank``, and the ``top``
    (0..20) most likely tokens per position in ``top_id`` / ``top_lp``. The logits are produced and
    reduced in chunks of at most 64 MiB; GPU and CPU engines, bf16 and fp8 heads; needs the whole
    model's head on this engine (NotImplementedError on a split head)."""
    sampler = Sampler(eng)
    if not eng.has_embed:
        raise RuntimeError("[ERROR] score_prompt needs the stage that owns the embedding")
    ids = [int(t) for t in ids]
    top = int(top)
    if len(ids) < 2:
        raise ValueError("score_prompt needs at least two tokens")
    if not 0 <= top <= LP.TOP_MAX:
        raise ValueError(f"top must be in [0, {LP.TOP_MAX}], got {top}")
    if len(ids) > eng.max_seq:
        raise ValueError(f"prompt ({len(ids)}) exceeds max_seq {eng.max_seq}")
    n = len(ids) - 1
    chunk = max(1, min(SCORE_CHUNK_BYTES // (2 * eng.cfg.head_rows), eng.max_prefill_rows))
    parts = []
    eng.seq_len[slot] = 0
    for c0 in range(0, len(ids), eng.max_prefill_rows):  # the prefill, in chunks the engine's scratch holds
        c = min(eng.max_prefill_rows, len(ids) - c0)
        h = eng.forward(eng.embed(torch.tensor(ids[c0:c0 + c], dtype=torch.int64)), [slot] * c,
                        list(range(c0, c0 + c)))
        eng.seq_len[slot] = c0 + c
        for r0 in range(0, min(c, n - c0), chunk):
            k = min(chunk, min(c, n - c0) - r0)
            logits = sampler.logits(h, list(range(r0, r0 + k)))
            lp = sampler.logprobs(logits, ids[c0 + r0 + 1:c0 + r0 + k + 1], top)
            parts.append([t.cpu() for t in lp])
            del logits
    return LP.Logprobs(*(torch.cat([p[i] for p in parts]) for i in range(5)))


__all__ = ["SamplingParams", "GREEDY", "Sampler", "PenaltyState", "ConstraintState", "GrammarState", "CompiledConstraint",
           "compile_constraints", "SamplingDecodeGraph", "EagerSamplingDecode",
           "device_params", "score_prompt", "SCORE_CHUNK_BYTES"]
