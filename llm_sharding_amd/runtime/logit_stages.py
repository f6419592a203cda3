"""The optional per-slot stages that edit a step's bf16 logits between the lm_head and the draw.

A stage (:class:`PenaltyState`, :class:`GrammarState`, :class:`ConstraintState`) owns device
tables indexed by KV slot and one kernel (with its numpy reference on a CPU engine) that advances
those tables by the step's input tokens and edits the rows in place. Each exists only once a
request asks for it; a Sampler, graph or server built without a stage runs exactly the step it
would run if the stage did not exist.

:data:`STAGE_CLASSES` is the one place that says in which order the stages run; the draw,
``argmax_finalize`` and the log-probabilities follow (``runtime.sampling``). Everything that runs a
step iterates that order: a new stage is one more class and one more entry.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch

from ..ops import constraints as K
from ..ops import grammar as G
from ..ops import pda as J
from ..ops import penalties as P
from .engine import StageEngine


def _check_full_head(eng: StageEngine) -> None:
    if eng.lm_head is None:
        raise RuntimeError("[ERROR] this stage has no lm_head")
    if (eng.head_v0, eng.head_v1) != (0, eng.cfg.head_rows):
        raise NotImplementedError("sampling needs the whole lm_head on one stage: this stage holds only vocabulary "
                                  f"rows [{eng.head_v0}, {eng.head_v1}) of {eng.cfg.head_rows} (split head)")


class LogitStage:
    """What the stages share: the argument checks, the eager call (:meth:`apply`), the captured
    call (:meth:`launch`) and the bookkeeping around a graph's warm-up run. A subclass names its
    tables and supplies ``_reference`` / ``_kernel``, ``admit`` / ``enter`` and ``wants``."""
    name = ""         # its entry of STAGE_ORDER: the keyword and attribute it is passed and kept by
    request = ""      # "a penalised request": who needs it, in the errors of a missing stage
    tables = ""       # "the penalty table", in the error of a slot outside it
    ROW_ARG = None    # the per-row argument of apply() beside slots and tokens: "params" / "positions"
    ROW_FIELDS = ()   # SamplingParams fields the kernel reads from per-row fp32 device arrays
    DISTURBED = ()    # the tables a step writes: what a warm-up run must not leave changed
    wants = None      # staticmethod wants(params) -> bool: the SamplingParams ask for this stage

    def __init__(self, eng: StageEngine, n_slots: int):
        _check_full_head(eng)
        self.eng, self.n_slots = eng, int(n_slots)

    @classmethod
    def needs(cls, owner: Optional[str] = None) -> str:
        """The RuntimeError text of a request that wants this stage where there is none: in
        ``owner`` (a graph class's name), or in ``Sampler.sample`` (None)."""
        if owner is None:
            return f"{cls.request} needs a {cls.__name__} (Sampler(eng, {cls.name}=...)) and slots="
        return f"{cls.request} needs {owner}(..., {cls.name}={cls.__name__})"

    def check_slot(self, slot: int) -> None:
        if not 0 <= slot < self.n_slots:
            raise ValueError(f"slot {slot} outside {self.tables} of {self.n_slots}")

    def check_covers(self, eng: StageEngine, slots, rows: int) -> None:
        """A graph of ``rows`` rows over ``slots`` can run this stage."""
        if self.eng is not eng or len(set(slots)) != rows or max(slots) >= self.n_slots:
            raise ValueError(f"{self.name}: a {type(self).__name__} of this engine with a distinct row per graph slot")

    # ------------------------------------------------------------------ requests
    def enter(self, slot: int, params, prompt_ids, reserved=None) -> None:
        """A request that :meth:`wants` this stage enters ``slot``: the one form of ``admit`` the
        servers use. ``reserved``: what the caller reserved for it at submission (None: nothing)."""

    def leave(self, slot: int, params) -> Optional[str]:
        """The request of ``slot`` is done: release what it held; a warning worth printing, or None."""

    # ------------------------------------------------------------------ the step
    def device_rows(self, params_list, device) -> tuple:
        """The per-row device arrays of ``ROW_FIELDS`` (a graph keeps them; :meth:`write_row`)."""
        return tuple(torch.tensor([getattr(p, k) for p in params_list], dtype=torch.float32, device=device)
                     for k in self.ROW_FIELDS)

    def write_row(self, arrays: tuple, row: int, params) -> None:
        for a, k in zip(arrays, self.ROW_FIELDS):
            a[row] = getattr(params, k)

    def apply(self, logits: torch.Tensor, slots, tokens_in, params_list=None, positions=None) -> torch.Tensor:
        """Advance ``slots[i]`` by ``tokens_in[i]`` (None: nothing) and edit row i of bf16 ``logits``
        [n, >= vocab_size] by ``params_list[i]``; ``positions[i]`` is the position the sampled token
        will occupy. A stage ignores what it does not need. The kernel in place on the GPU, the
        numpy reference on a CPU engine. Returns the edited logits."""
        n, V = logits.shape[0], self.eng.cfg.vocab_size
        slots = [int(s) for s in slots]
        per_row = {"params": params_list, "positions": positions}.get(self.ROW_ARG)
        if (len(slots) != n or (self.ROW_ARG and len(per_row) != n)
                or (tokens_in is not None and len(tokens_in) != n)):
            raise ValueError(f"{self.name}: {n} rows, {len(slots)} slots"
                             + (f", {len(per_row)} {self.ROW_ARG}" if self.ROW_ARG else ""))
        if len(set(slots)) != n or any(not 0 <= s < self.n_slots for s in slots):
            raise ValueError(f"{self.name}: slots {slots} must be distinct and below {self.n_slots}")
        if not self.eng.gpu:
            out, *new = self._reference(logits.to(torch.bfloat16), V, slots, tokens_in, per_row)
            for k, a in zip(self.DISTURBED, new):
                getattr(self, k).copy_(torch.from_numpy(a))
            return out
        i32 = lambda x: torch.tensor([int(v) for v in x], dtype=torch.int32, device=self.eng.device)  # noqa: E731
        self._kernel(logits, n, i32(slots), None if tokens_in is None else i32(tokens_in),
                     self.device_rows(params_list, self.eng.device),
                     i32(per_row) if self.ROW_ARG == "positions" else None, 0)
        return logits

    def launch(self, graph) -> None:
        """The stage's launch of a captured step, on the graph's buffers and its per-row arrays."""
        self._kernel(graph.logits, graph.rows, graph.slot, graph.tokens, graph.stage_rows[self.name], graph.pos, 1)

    def snapshot(self, idx: torch.Tensor) -> list:
        """The rows ``idx`` (int64 slots) of what a step writes, to :meth:`restore` after a warm-up."""
        return [getattr(self, k).index_select(0, idx) for k in self.DISTURBED]

    def restore(self, idx: torch.Tensor, saved: list) -> None:
        for k, t in zip(self.DISTURBED, saved):
            getattr(self, k).index_copy_(0, idx, t)


class PenaltyState(LogitStage):
    """The token statistics of the penalties: ``uint16 [n_slots, head_rows]`` on the engine's
    device (bit 15: the token occurs in the slot's prompt; bits 0..14: how often it has been
    generated, saturating) - 32.8 MB at 512 slots x 32000. Built when the first penalised
    request arrives, like the logits buffer. torch stores the table as int16 (same bits).
    In a step ``lsa_penalize`` counts the input tokens into the rows' slots and edits the logits by
    the per-row ``rep / pres / freq`` device arrays; rows whose penalties are off are skipped."""
    name, request, tables = "penalties", "a penalised request", "the penalty table"
    ROW_ARG, DISTURBED = "params", ("state",)
    ROW_FIELDS = ("repetition_penalty", "presence_penalty", "frequency_penalty")
    wants = staticmethod(lambda params: params.penalized)

    def __init__(self, eng: StageEngine, n_slots: int):
        super().__init__(eng, n_slots)
        self.state = torch.zeros((self.n_slots, eng.cfg.head_rows), dtype=torch.int16, device=eng.device)

    def admit(self, slot: int, prompt_ids) -> None:
        """A penalised request enters ``slot``: zero its row, set the prompt bits."""
        self.check_slot(slot)
        ids = torch.as_tensor([int(t) for t in prompt_ids], dtype=torch.long, device=self.state.device)
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= self.eng.cfg.vocab_size):
            raise ValueError("prompt token outside the vocabulary")
        row = self.state[slot]
        row.zero_()
        row[ids] = -0x8000  # int16 pattern of bit 15

    def enter(self, slot: int, params, prompt_ids, reserved=None) -> None:
        self.admit(slot, prompt_ids)

    def counts(self, slot: int) -> torch.Tensor:
        """Generated-token counts of ``slot`` (int32 [vocab_size], on the host)."""
        return (self.state[slot, :self.eng.cfg.vocab_size].cpu().to(torch.int32) & P.COUNT_MAX)

    def _reference(self, logits, V, slots, tokens_in, params_list):
        rep, pres, freq = ([getattr(p, k) for p in params_list] for k in self.ROW_FIELDS)
        out, st = P.penalize_reference(logits, V, self.state, slots, tokens_in, rep, pres, freq)
        return out, st.view("int16")

    def _kernel(self, logits, n, slot, tokens, rows, pos, ctr_add) -> None:
        P.penalize(logits, self.eng.cfg.vocab_size, n, slot, tokens, self.state, *rows)


@dataclass
class CompiledConstraint:
    """One request's constraint fields against a configuration: what :meth:`ConstraintState.admit`
    writes into a slot."""
    automaton: Optional[K.TokenAutomaton]
    bias_tok: list
    bias_val: list
    min_tokens: int
    minp_delta: float  # float32(T * ln(min_p)); -inf = off


def compile_constraints(params, vocab_size: int, eos_ids) -> CompiledConstraint:
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


class ArenaStage(LogitStage):
    """A stage whose requests share automata through an int16 ``arena`` of ``rows`` x ``width``:
    ``alloc`` (an :class:`ops.constraints.ArenaAllocator` of ``rows`` rows, by default a new one)
    places automata in contiguous row ranges and shares them by content digest; an automaton's rows
    are uploaded when its first request is admitted. ``eos``: the configuration's EOS ids, padded."""
    ROWS_ARG = ""  # the constructor's name for ``rows``, in its error

    def __init__(self, eng: StageEngine, n_slots: int, rows: int, allocator: Optional[K.ArenaAllocator], width: int):
        super().__init__(eng, n_slots)
        self.alloc = K.ArenaAllocator(rows) if allocator is None else allocator
        if self.alloc.state_rows != rows or self.n_slots < 1:
            raise ValueError(f"{type(self).__name__}: the allocator must cover {self.ROWS_ARG} rows, and n_slots >= 1")
        self.arena = torch.full((rows, width), -1, dtype=torch.int16, device=eng.device)
        self.eos_ids = [int(e) for e in eng.cfg.eos_ids][:K.N_EOS]
        pad = [-1] * (K.N_EOS - len(self.eos_ids))
        self.eos = torch.tensor(self.eos_ids + pad, dtype=torch.int32, device=eng.device)
        self.resident: set = set()      # digests whose rows are in the arena
        self.held: dict = {}            # slot -> digest of the automaton it holds

    def _hold(self, slot: int, auto, acquired: bool) -> int:
        """``slot`` holds a reference on ``auto`` (``acquired``: the caller took it from the allocator
        already) and ``auto``'s rows are in the arena. Returns their first row."""
        d = auto.digest
        base = self.alloc.base(d) if acquired else self.alloc.acquire(auto)
        self.held[slot] = d
        if d not in self.resident:
            self._upload(base, auto)
            if self.eng.gpu:  # streams other than this one may admit the same automaton next
                torch.cuda.current_stream(self.arena.device).synchronize()
            self.resident.add(d)
        return base

    def _drop(self, slot: int) -> None:
        """The automaton ``slot`` held loses one reference."""
        d = self.held.pop(slot, None)
        if d is not None and self.alloc.release(d):
            self.resident.discard(d)

    def leave(self, slot: int, params) -> Optional[str]:
        self.release(slot)


class ConstraintState(ArenaStage):
    """The tables of constrained decoding (``ops.constraints``) on the engine's device: the
    automaton arena ``int16 [state_rows, head_rows]`` (one row per automaton state - 256 rows are
    16 MB at a vocabulary of 32000 and 66 MB at 128256), the per-slot rows ``astate / abase / bias_n
    / bias_tok / bias_val / min_until / minp_delta / fault`` and the configuration's EOS ids. Built
    when the first constrained request arrives; ``allocator``: see :class:`ArenaStage`.
    In a step ``lsa_logit_process`` advances the rows' automaton states by the input tokens and
    applies bias, EOS mask, automaton mask and min-p from the per-slot tables (written by
    :meth:`admit`); rows whose slots hold no constraint are skipped."""
    name, request, tables = "constraints", "a constrained request", "the constraint tables"
    ROW_ARG, DISTURBED, ROWS_ARG = "positions", ("astate", "fault"), "state_rows"
    wants = staticmethod(lambda params: params.constrained)

    def __init__(self, eng: StageEngine, n_slots: int, state_rows: int = 256,
                 allocator: Optional[K.ArenaAllocator] = None):
        self.state_rows = int(state_rows)
        super().__init__(eng, n_slots, self.state_rows, allocator, eng.cfg.head_rows)
        dev, n = eng.device, self.n_slots
        self.astate = torch.full((n,), -1, dtype=torch.int32, device=dev)
        self.abase = torch.zeros(n, dtype=torch.int32, device=dev)
        self.bias_n = torch.zeros(n, dtype=torch.int32, device=dev)
        self.bias_tok = torch.zeros((n, K.BIAS_MAX), dtype=torch.int32, device=dev)
        self.bias_val = torch.zeros((n, K.BIAS_MAX), dtype=torch.float32, device=dev)
        self.min_until = torch.zeros(n, dtype=torch.int32, device=dev)
        self.minp_delta = torch.full((n,), float("-inf"), dtype=torch.float32, device=dev)
        self.fault = torch.zeros(n, dtype=torch.int32, device=dev)

    def compile(self, params) -> CompiledConstraint:
        return compile_constraints(params, self.eng.cfg.vocab_size, self.eng.cfg.eos_ids)

    def _upload(self, base: int, auto) -> None:
        rows = torch.from_numpy(np.array(auto.next)).to(self.arena.device)
        self.arena[base:base + auto.n_states, :auto.vocab] = rows

    def admit(self, slot: int, params, prompt_len: int, compiled: Optional[CompiledConstraint] = None,
              acquired: bool = False) -> None:
        """A request enters ``slot``: write its rows and point ``astate`` at its automaton's start
        state. ``compiled`` / ``acquired``: the caller has compiled the fields, and already holds
        the allocator's reference (the server does both when the request is submitted)."""
        self.check_slot(slot)
        self.release(slot)
        if params is None or not params.constrained:
            return
        c = self.compile(params) if compiled is None else compiled
        base = -1 if c.automaton is None else self._hold(slot, c.automaton, acquired)
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

    def enter(self, slot: int, params, prompt_ids, reserved=None) -> None:
        self.admit(slot, params, len(prompt_ids), compiled=reserved, acquired=reserved is not None)

    def release(self, slot: int) -> None:
        """Clear ``slot``; the automaton it held loses one reference (``fault`` stays readable
        until the next :meth:`admit`)."""
        self._drop(slot)
        self.astate[slot] = -1
        self.bias_n[slot] = 0
        self.min_until[slot] = 0
        self.minp_delta[slot] = float("-inf")

    def apply(self, logits: torch.Tensor, slots, tokens_in, positions, params_list=None) -> torch.Tensor:
        """:meth:`LogitStage.apply`, with the argument this stage needs in front."""
        positions = positions.tolist() if isinstance(positions, torch.Tensor) else positions
        return super().apply(logits, slots, tokens_in, params_list, [int(p) for p in positions])

    def _reference(self, logits, V, slots, tokens_in, positions):
        return K.logit_process_reference(logits, V, self, slots, tokens_in, positions)

    def _kernel(self, logits, n, slot, tokens, rows, pos, ctr_add) -> None:
        K.logit_process(logits, self.eng.cfg.vocab_size, n, slot, tokens, pos, self, ctr_add=ctr_add)


class GrammarState(ArenaStage):
    """The tables of regex-constrained decoding (``ops.grammar``) on the engine's device: the DFA
    arena ``int16 [dfa_rows, 256]`` with its ``accept`` bytes (513 B per state whatever the
    vocabulary - 2 MB at the default 4096 rows, where the dense arena of :class:`ConstraintState`
    takes 64 KB per state at a vocabulary of 32000), the vocabulary's byte strings (``offsets``,
    ``data``), the per-slot rows ``gstate / gbase / gfault`` (12 B per slot) and the configuration's
    EOS ids. Built when the first request with a regex arrives; ``allocator``: see
    :class:`ArenaStage`.
    In a step ``lsa_grammar_mask`` advances the rows' DFA states by the bytes of the input tokens
    and masks every token whose bytes die in the automaton; rows whose slots hold no regex are
    skipped.

    ``pda`` (an :class:`ops.pda.BytePDA`, in practice ``BytePDA.json()``): the stage also serves
    ``json_object`` requests. It then owns the automaton's planes ``ptab`` / ``paccept`` and the
    per-slot configuration ``jstate / jdepth / jstack`` (16 B per slot), and its step launches
    ``lsa_pda_mask`` after ``lsa_grammar_mask``: a slot holds a regex or JSON, never both, and each
    kernel skips the other's slots. The vocabulary is checked against the automaton here
    (``ops.pda.check_vocab``: ValueError), so an admitted request never meets a row without a
    column. Without ``pda`` the stage allocates and launches exactly what it does for a regex."""
    name, request, tables = "grammar", "a request with a regex or json_object", "the grammar tables"
    DISTURBED, ROWS_ARG = ("gstate", "gfault"), "dfa_rows"
    wants = staticmethod(lambda params: params.grammar is not None or params.json_object)

    def __init__(self, eng: StageEngine, n_slots: int, vocab: "G.VocabBytes", dfa_rows: int = 4096,
                 allocator: Optional[K.ArenaAllocator] = None, pda: Optional["J.BytePDA"] = None):
        _check_full_head(eng)
        if not isinstance(vocab, G.VocabBytes) or vocab.V != eng.cfg.vocab_size:
            raise ValueError(f"GrammarState: a VocabBytes over the configuration's {eng.cfg.vocab_size} tokens, got "
                             f"{getattr(vocab, 'V', None)}")
        self.dfa_rows, self.vocab = int(dfa_rows), vocab
        super().__init__(eng, n_slots, self.dfa_rows, allocator, 256)
        dev, n = eng.device, self.n_slots
        self.accept = torch.zeros(self.dfa_rows, dtype=torch.uint8, device=dev)
        self.offsets = torch.from_numpy(np.array(vocab.offsets)).to(dev)
        self.data = torch.from_numpy(np.array(vocab.data)).to(dev)
        self.gstate = torch.full((n,), -1, dtype=torch.int32, device=dev)
        self.gbase = torch.zeros(n, dtype=torch.int32, device=dev)
        self.gfault = torch.zeros(n, dtype=torch.int32, device=dev)
        self.checked = check_vocab_cache(vocab, self.eos_ids)
        self.pda = pda
        if pda is not None:
            if not isinstance(pda, J.BytePDA):
                raise ValueError(f"GrammarState: pda must be an ops.pda.BytePDA, got {type(pda).__name__}")
            J.check_vocab(pda, vocab, self.eos_ids)
            self.ptab = torch.from_numpy(np.array(pda.next)).to(dev)
            self.paccept = torch.from_numpy(np.array(pda.accept)).to(dev)
            self.jstate = torch.full((n,), -1, dtype=torch.int32, device=dev)
            self.jdepth = torch.zeros(n, dtype=torch.int32, device=dev)
            self.jstack = torch.zeros(n, dtype=torch.int64, device=dev)
            self.DISTURBED = ("gstate", "gfault", "jstate", "jdepth", "jstack")

    def check(self, dfa: "G.ByteDFA") -> None:
        """ValueError unless every state of ``dfa`` allows at least one token of this vocabulary."""
        self.checked(dfa)

    def _upload(self, base: int, dfa) -> None:
        S = dfa.n_states
        flags = dfa.accept.astype(np.uint8) * G.ACCEPT
        flags[S - 1] |= G.LAST
        self.arena[base:base + S] = torch.from_numpy(np.array(dfa.next)).to(self.arena.device)
        self.accept[base:base + S] = torch.from_numpy(flags).to(self.arena.device)

    def admit(self, slot: int, params, acquired: bool = False) -> None:
        """A request enters ``slot``: point ``gstate`` at its DFA's start state (uploading the DFA's
        rows when it is new). ``acquired``: the caller already holds the allocator's reference and
        has run :meth:`check` (the server does both when the request is submitted)."""
        self.check_slot(slot)
        self.release(slot)
        dfa = None if params is None else params.grammar
        if dfa is None:
            if params is not None and params.json_object:
                if self.pda is None:
                    raise ValueError("json_object needs a GrammarState built with pda=BytePDA.json()")
                if not self.eos_ids:
                    raise ValueError("json_object needs an EOS id in the configuration: the output ends with it")
                self.jdepth[slot] = 0
                self.jstack[slot] = 0
                self.jstate[slot] = 0
                self.gfault[slot] = 0
            return
        if not acquired:
            self.check(dfa)
        base = self._hold(slot, dfa, acquired)
        self.gbase[slot] = base
        self.gstate[slot] = base
        self.gfault[slot] = 0

    def enter(self, slot: int, params, prompt_ids, reserved=None) -> None:
        self.admit(slot, params, acquired=reserved is not None)

    def release(self, slot: int) -> None:
        """Clear ``slot``; the DFA it held loses one reference (``gfault`` stays readable until the
        next :meth:`admit`)."""
        self._drop(slot)
        self.gstate[slot] = -1
        if self.pda is not None:
            self.jstate[slot] = -1

    def leave(self, slot: int, params) -> Optional[str]:
        fault = int(self.gfault[slot])
        self.release(slot)
        what = "json_object" if params.grammar is None else f"regex {params.regex!r}"
        return (f"grammar fault {fault} under {what} (1: a token outside the pattern was fed, 2: a "
                "state allowed no token)") if fault else None

    def _reference(self, logits, V, slots, tokens_in, _):
        out, gstate, gfault = G.grammar_mask_reference(logits, V, self, slots, tokens_in)
        if self.pda is None:
            return out, gstate, gfault
        tb = SimpleNamespace(**{k: getattr(self, k) for k in J.TABLES})
        tb.gfault = gfault
        out, jstate, jdepth, jstack, gfault = J.pda_mask_reference(out, V, tb, slots, tokens_in)
        return out, gstate, gfault, jstate, jdepth, jstack

    def _kernel(self, logits, n, slot, tokens, rows, pos, ctr_add) -> None:
        G.grammar_mask(logits, self.eng.cfg.vocab_size, n, slot, tokens, self)
        if self.pda is not None:
            J.pda_mask(logits, self.eng.cfg.vocab_size, n, slot, tokens, self)


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


# The order of a step: penalise -> grammar mask -> process (min-p sees the masked row).
STAGE_CLASSES = (PenaltyState, GrammarState, ConstraintState)
STAGE_ORDER = tuple(c.name for c in STAGE_CLASSES)


def ordered_stages(penalties=None, constraints=None, grammar=None) -> list:
    """The stages that exist, in the order a step runs them."""
    given = {"penalties": penalties, "constraints": constraints, "grammar": grammar}
    return [given[k] for k in STAGE_ORDER if given[k] is not None]


__all__ = ["LogitStage", "ArenaStage", "PenaltyState", "ConstraintState", "GrammarState", "CompiledConstraint",
           "compile_constraints", "check_vocab_cache", "STAGE_CLASSES", "STAGE_ORDER", "ordered_stages"]
