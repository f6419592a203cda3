"""Constrained decoding: token automata, the ctypes binding of csrc/sampling/logit_process.hip and
the numpy float32 reference of the same contract (the CPU implementation and the tests' oracle).

Tables (``runtime.sampling.ConstraintState`` holds them on the engine's device):

* ``arena`` int16 ``[state_rows, ld >= V]``: one row per automaton state; an entry ``< 0`` means
  "token forbidden in this state", any other value is the next state, relative to the automaton's
  first row;
* per slot: ``astate`` int32 (arena row of the current state, -1 = no automaton), ``abase`` int32
  (arena row of the automaton's state 0), ``bias_n`` int32, ``bias_tok`` int32 ``[.., 320]`` and
  ``bias_val`` fp32 ``[.., 320]`` (distinct tokens; ``-inf`` = banned), ``min_until`` int32 (the
  first position at which an EOS id may be produced), ``minp_delta`` fp32 (``T * ln(min_p)``,
  ``-inf`` = off) and ``fault`` int32;
* ``eos`` int32 ``[8]``: the EOS ids, padded with -1.

Contract per row with slot ``s``, input token ``t`` (``t < 0`` or no ``tokens_in``: none) and
``c = ctr + ctr_add``, the position the sampled token will occupy:

0. ``astate[s] < 0``, ``bias_n[s] == 0``, ``c >= min_until[s]`` and ``minp_delta[s] == -inf``: the
   row is skipped - logits and state stay bit-identical and no table row is read;
1. ``a = astate[s]``. With ``a >= 0`` and a token ``t``: ``n = arena[a][t]``; ``n >= 0``:
   ``a = abase[s] + n`` and ``astate[s] = a``; otherwise (also for ``t >= V``) ``a`` stays and
   ``fault[s] = 1``. A state outside ``[0, state_rows)`` sets ``fault[s] = 1`` and the row runs
   without an automaton;
2. for every column ``v < V``, ``x = fp32(l_v)``: a bias entry ``(v, b)`` gives
   ``x = fp32(bf16_rne(x + b))`` (one fp32 add); ``c < min_until[s]`` and ``v`` an EOS id gives
   ``x = -inf``; ``a >= 0`` and ``arena[a][v] < 0`` gives ``x = -inf``;
3. ``minp_delta[s] > -inf``: ``m = max_v x``, ``thr = m + minp_delta[s]`` (one fp32 add), every
   ``x < thr`` becomes ``-inf`` (HF's ``MinPLogitsWarper`` in log space: ``p_i < min_p * p_max`` at
   temperature ``T`` is ``l_i < l_max + T ln(min_p)``). The maximum always survives;
4. ``l_v`` is rewritten only where it changed: the rounded sum, or the bf16 pattern ``0xFF80``.

Columns ``>= V`` (the lm_head padding) are never read or written. A slot outside the tables skips
its row. Every result is an exact function of the inputs: kernel and reference agree bitwise.
"""
from __future__ import annotations

import ctypes
import hashlib
import threading
from typing import Optional

import numpy as np
import torch

from .penalties import bf16_bits_to_f32, bf16_rne_bits

BIAS_MAX = 320
N_EOS = 8
MAX_STATES = 32767
NEG_INF_BITS = 0xFF80
TABLES = ("arena", "astate", "abase", "bias_n", "bias_tok", "bias_val", "min_until", "minp_delta", "fault", "eos")


# ------------------------------------------------------------------------------ automata
class TokenAutomaton:
    """A deterministic automaton over token ids: ``next`` int16 ``[S, V]``, ``1 <= S <= 32767``,
    start state 0, ``-1`` = "token forbidden in this state", any other entry = the next state.
    Every state allows at least one token. ``digest`` identifies the content: equal automata share
    their rows of the arena."""

    def __init__(self, next):  # noqa: A002 - the issue's name of the table
        a = np.asarray(next)
        if a.ndim != 2 or a.dtype.kind not in "iu":
            raise ValueError("TokenAutomaton: next must be an integer [states, vocabulary] table")
        S, V = a.shape
        if not 1 <= S <= MAX_STATES or V < 1:
            raise ValueError(f"TokenAutomaton: 1 <= states <= {MAX_STATES} and a non-empty vocabulary, got {a.shape}")
        if int(a.min()) < -1 or int(a.max()) >= S:
            raise ValueError(f"TokenAutomaton: entries must be -1 (forbidden) or a state in [0, {S})")
        dead = np.nonzero((a >= 0).sum(axis=1) == 0)[0]
        if dead.size:
            raise ValueError(f"TokenAutomaton: state {int(dead[0])} allows no token")
        self.next = np.ascontiguousarray(a, dtype=np.int16)
        self.next.setflags(write=False)
        h = hashlib.sha256(np.array([S, V], dtype=np.int64).tobytes())
        h.update(self.next.tobytes())
        self.digest = h.hexdigest()

    @property
    def n_states(self) -> int:
        return self.next.shape[0]

    @property
    def vocab(self) -> int:
        return self.next.shape[1]

    def __eq__(self, other):
        return isinstance(other, TokenAutomaton) and other.digest == self.digest

    def __hash__(self):
        return hash(self.digest)

    def __repr__(self):
        return f"TokenAutomaton(states={self.n_states}, vocab={self.vocab}, digest={self.digest[:12]})"

    def walk(self, tokens, state: int = 0) -> int:
        """The state after feeding ``tokens`` from ``state``; -1 as soon as one is forbidden."""
        for t in tokens:
            t = int(t)
            if state < 0 or not 0 <= t < self.vocab:
                return -1
            state = int(self.next[state, t])
        return state

    @classmethod
    def from_table(cls, next) -> "TokenAutomaton":  # noqa: A002
        return cls(next)

    @staticmethod
    def _ids(ids, V: int, what: str) -> list:
        out = [int(t) for t in ids]
        if any(not 0 <= t < V for t in out):
            raise ValueError(f"{what}: token outside the vocabulary [0, {V})")
        return out

    @classmethod
    def from_allowed(cls, ids, V: int) -> "TokenAutomaton":
        """One state that loops on the allowed tokens."""
        ids = cls._ids(ids, V, "allowed_token_ids")
        if not ids:
            raise ValueError("allowed_token_ids: at least one token")
        t = np.full((1, V), -1, dtype=np.int16)
        t[0, ids] = 0
        return cls(t)

    @classmethod
    def from_choices(cls, choices, V: int, eos_ids) -> "TokenAutomaton":
        """A trie of the token-id sequences ``choices``. A node where a choice ends also allows
        every EOS id, leading to an absorbing end state that allows only the EOS ids - a choice
        that is a prefix of another may continue or end. Duplicates merge."""
        eos = cls._ids(eos_ids or (), V, "eos ids")
        if not eos:
            raise ValueError("choices need an EOS id: the configuration has none")
        choices = [cls._ids(c, V, "choices") for c in choices]
        if not choices or any(not c for c in choices):
            raise ValueError("choices: at least one choice, and no empty choice")
        if any(t in eos for c in choices for t in c):
            raise ValueError("choices: a choice must not contain an EOS id")
        kids, ends = [{}], [False]
        for c in sorted(set(map(tuple, choices))):  # one numbering of the states whatever the order given
            node = 0
            for t in c:
                nxt = kids[node].get(t)
                if nxt is None:
                    nxt = len(kids)
                    kids.append({})
                    ends.append(False)
                    kids[node][t] = nxt
                node = nxt
            ends[node] = True
        end = len(kids)
        if end + 1 > MAX_STATES:
            raise ValueError(f"choices: the trie needs {end + 1} states, more than {MAX_STATES}")
        t = np.full((end + 1, V), -1, dtype=np.int16)
        for node, ch in enumerate(kids):
            for tok, nxt in ch.items():
                t[node, tok] = nxt
            if ends[node]:
                t[node, eos] = end
        t[end, eos] = end
        return cls(t)


class ArenaAllocator:
    """Host bookkeeping of the arena's rows: automata sit in contiguous row ranges (first fit), one
    reference count per digest; a range is freed when its last holder releases it. Every method
    takes the allocator's own lock: a server reserves rows on the thread that submits a request and
    returns them on the thread that serves."""

    def __init__(self, state_rows: int):
        self.state_rows = int(state_rows)
        if self.state_rows < 1:
            raise ValueError("the automaton arena needs at least one row")
        self.free = [(0, self.state_rows)]
        self.entries = {}  # digest -> [base, automaton, references]
        self._lock = threading.Lock()

    def acquire(self, automaton: TokenAutomaton) -> int:
        """Reserve (or share) the rows of ``automaton``: its base row. ValueError when it does not fit."""
        with self._lock:
            e = self.entries.get(automaton.digest)
            if e is not None:
                e[2] += 1
                return e[0]
            n = automaton.n_states
            for i, (b, ln) in enumerate(self.free):
                if ln >= n:
                    if ln == n:
                        del self.free[i]
                    else:
                        self.free[i] = (b + n, ln - n)
                    self.entries[automaton.digest] = [b, automaton, 1]
                    return b
            raise ValueError(f"an automaton of {n} states does not fit the arena: {sum(ln for _, ln in self.free)} of "
                             f"{self.state_rows} rows are free, the largest range has "
                             f"{max((ln for _, ln in self.free), default=0)}")

    def release(self, digest: str) -> bool:
        """Drop one reference; True when the range was freed."""
        with self._lock:
            e = self.entries[digest]
            e[2] -= 1
            if e[2] > 0:
                return False
            del self.entries[digest]
            merged = []
            for fb, fl in sorted(self.free + [(e[0], e[1].n_states)]):
                if merged and merged[-1][0] + merged[-1][1] == fb:
                    merged[-1] = (merged[-1][0], merged[-1][1] + fl)
                else:
                    merged.append((fb, fl))
            self.free = merged
            return True

    def base(self, digest: str) -> int:
        with self._lock:
            return self.entries[digest][0]

    def refs(self, digest: str) -> int:
        with self._lock:
            e = self.entries.get(digest)
            return 0 if e is None else e[2]

    def rows_free(self) -> int:
        with self._lock:
            return sum(ln for _, ln in self.free)


# ------------------------------------------------------------------------------ reference
def _np(x, dtype) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().contiguous().numpy()
    return np.asarray(x, dtype=dtype)


def _bits_of(logits) -> np.ndarray:
    if isinstance(logits, torch.Tensor):
        if logits.dtype != torch.bfloat16:
            raise ValueError("logit_process_reference takes bf16 logits (or their uint16 bit patterns)")
        a = logits.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16).copy()
    else:
        a = np.array(logits, dtype=np.uint16)
    return a[None] if a.ndim == 1 else a


def processed_values(x: np.ndarray, eos_on: bool, eos, bias_tok, bias_val, allowed: Optional[np.ndarray],
                     delta) -> np.ndarray:
    """Steps 2-3 on one row: fp32 logits ``x`` [V] -> fp32 values (exact bf16 numbers or -inf)."""
    V = x.size
    x = np.array(x, dtype=np.float32)
    ninf = np.float32(-np.inf)
    for v, b in zip(bias_tok, bias_val):
        v = int(v)
        if 0 <= v < V:
            y = np.array([x[v] + np.float32(b)], dtype=np.float32)
            x[v] = bf16_bits_to_f32(bf16_rne_bits(y))[0]
    if eos_on:
        for e in eos:
            if 0 <= int(e) < V:
                x[int(e)] = ninf
    if allowed is not None:
        x[~allowed] = ninf
    delta = np.float32(delta)
    if delta > ninf:
        thr = np.float32(x.max() + delta)
        x[x < thr] = ninf
    return x


def logit_process_reference(logits_bf16, V: int, tables, slot, tokens_in, ctr, ctr_add: int = 0):
    """The contract in numpy float32, operation by operation. ``logits_bf16``: [rows, >= V] bf16
    tensor (or uint16 bit patterns); ``tables``: an object with the attributes :data:`TABLES`
    (numpy or torch); ``slot`` / ``ctr``: per row; ``tokens_in``: per row or None. The inputs are
    not modified. Returns ``(logits, astate, fault)``: a bf16 tensor (a uint16 array when bit
    patterns were given) of the input's shape and two int32 arrays ``[n_slots]``."""
    was_tensor = isinstance(logits_bf16, torch.Tensor)
    one_row = (logits_bf16.dim() if was_tensor else np.ndim(logits_bf16)) == 1
    bits = _bits_of(logits_bf16)
    rows = bits.shape[0]
    arena = _np(tables.arena, np.int16)
    astate, fault = _np(tables.astate, np.int32).copy(), _np(tables.fault, np.int32).copy()
    abase, bias_n = _np(tables.abase, np.int32), _np(tables.bias_n, np.int32)
    bias_tok = _np(tables.bias_tok, np.int32).reshape(-1, BIAS_MAX)
    bias_val = _np(tables.bias_val, np.float32).reshape(-1, BIAS_MAX)
    min_until, minp_delta = _np(tables.min_until, np.int32), _np(tables.minp_delta, np.float32)
    eos = _np(tables.eos, np.int32)
    n_slots, state_rows = astate.size, arena.shape[0]
    slot = [int(s) for s in (slot.tolist() if hasattr(slot, "tolist") else slot)]
    ctr = [int(c) for c in (ctr.tolist() if hasattr(ctr, "tolist") else ctr)]
    if tokens_in is None:
        tokens_in = [-1] * rows
    tokens_in = [int(t) for t in (tokens_in.tolist() if hasattr(tokens_in, "tolist") else tokens_in)]
    if not len(slot) == len(tokens_in) == len(ctr) == rows:
        raise ValueError(f"logit_process_reference: per-row arguments do not match {rows} rows")
    if bits.shape[1] < V or arena.ndim != 2 or arena.shape[1] < V:
        raise ValueError("logit_process_reference: a row is shorter than V")
    ninf = np.float32(-np.inf)
    for r in range(rows):
        s = slot[r]
        if not 0 <= s < n_slots:
            continue
        c = ctr[r] + int(ctr_add)
        a = int(astate[s])
        bn = min(max(int(bias_n[s]), 0), BIAS_MAX)
        eos_on = c < int(min_until[s])
        delta = minp_delta[s]
        if a < 0 and bn == 0 and not eos_on and not delta > ninf:
            continue
        if a >= state_rows:
            fault[s] = 1
            a = -1
        elif a >= 0 and tokens_in[r] >= 0:
            t = tokens_in[r]
            n = int(arena[a, t]) if t < V else -1
            a1 = int(abase[s]) + n if n >= 0 else -1
            if 0 <= a1 < state_rows:
                a = a1
                astate[s] = a
            else:
                fault[s] = 1
        old = bits[r, :V]
        x = processed_values(bf16_bits_to_f32(old), eos_on, eos, bias_tok[s, :bn], bias_val[s, :bn],
                             arena[a, :V] >= 0 if a >= 0 else None, delta)
        new = bf16_rne_bits(x)
        bits[r, :V] = np.where(new != old, new, old)
    if one_row:
        bits = bits[0]
    if was_tensor:
        return torch.from_numpy(bits.view(np.int16).copy()).view(torch.bfloat16), astate, fault
    return bits, astate, fault


# ------------------------------------------------------------------------------ HIP binding
_declared = None


def _lib() -> ctypes.CDLL:
    """The kernel library (``hip.lib()``) with the constraint entry points declared."""
    global _declared
    from . import hip
    L = hip.lib()
    if _declared is not L:
        vp, i, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
        if not hasattr(L, "lsa_logit_process"):
            raise RuntimeError("the kernel library has no lsa_logit_process: rebuild it (python csrc/build.py)")
        L.lsa_logit_process.argtypes = [vp, ll, i, i, vp, i, vp, vp, i, vp, ll, i] + [vp] * 10
        L.lsa_logit_process.restype = i
        L.lsa_logit_process_calls.argtypes = []
        L.lsa_logit_process_calls.restype = ll
        L.lsa_logit_process_reread.argtypes = L.lsa_logit_process.argtypes
        L.lsa_logit_process_reread.restype = i
        _declared = L
    return L


def logit_process_calls() -> int:
    """How often this process has enqueued ``lsa_logit_process`` (a captured graph counts at capture)."""
    return int(_lib().lsa_logit_process_calls())


def logit_process(logits: torch.Tensor, V: int, rows: int, slot: torch.Tensor, tokens_in: Optional[torch.Tensor],
                  ctr: torch.Tensor, tables, ctr_add: int = 0, reread: bool = False) -> None:
    """``lsa_logit_process``: advance the automaton states of the slots ``slot`` (int32 [rows],
    distinct) by ``tokens_in`` (int32 [rows] or None) and edit the first ``rows`` rows of bf16
    ``logits`` [>= rows, ld >= V] in place; ``ctr`` int32 [rows], ``tables``: an object with the
    attributes :data:`TABLES` as cuda tensors. No host reads: graph-capturable. ``reread``
    (measurement and tests): the entry ``lsa_logit_process_reread``, whose min-p pass re-reads the
    row from L2 at every size instead of keeping rows of up to 32768 columns in registers - the
    same bits."""
    from .hip import _check, _p, _req, _stream
    from .sampling import _chk
    _req(logits.is_cuda and logits.dtype == torch.bfloat16 and logits.dim() == 2 and logits.stride(1) == 1,
         "logit_process: logits must be a row-major bf16 cuda matrix")
    _req(1 <= rows <= logits.shape[0] and 1 <= V <= logits.shape[1] and rows <= 65535,
         f"logit_process: rows={rows}, V={V} outside logits {tuple(logits.shape)}")
    _req(rows == 1 or logits.stride(0) >= V, "logit_process: row stride below V")
    _req(all(getattr(tables, k, None) is not None for k in TABLES), "logit_process: a table is missing")
    arena = tables.arena
    _req(arena.is_cuda and arena.dtype == torch.int16 and arena.dim() == 2 and arena.stride(1) == 1
         and arena.shape[1] >= V and (arena.shape[0] == 1 or arena.stride(0) >= V) and arena.device == logits.device,
         "logit_process: the arena must be a row-major int16 cuda table [state_rows, >= V] on the logits' device")
    n_slots = tables.astate.numel()
    _req(n_slots >= 1, "logit_process: empty slot tables")
    _chk(slot, torch.int32, rows, "slot")
    _chk(ctr, torch.int32, rows, "ctr")
    if tokens_in is not None:
        _chk(tokens_in, torch.int32, rows, "tokens_in")
    for k in ("astate", "abase", "bias_n", "min_until", "fault"):
        _chk(getattr(tables, k), torch.int32, n_slots, k)
    _chk(tables.minp_delta, torch.float32, n_slots, "minp_delta")
    _chk(tables.bias_tok, torch.int32, n_slots * BIAS_MAX, "bias_tok")
    _chk(tables.bias_val, torch.float32, n_slots * BIAS_MAX, "bias_val")
    _chk(tables.eos, torch.int32, N_EOS, "eos")
    ld = logits.stride(0) if rows > 1 else max(logits.stride(0), V)
    lda = arena.stride(0) if arena.shape[0] > 1 else max(arena.stride(0), V)
    L = _lib()
    rc = (L.lsa_logit_process_reread if reread else L.lsa_logit_process)(_p(logits), ld, V, rows, _p(slot), n_slots, _p(tokens_in), _p(ctr), int(ctr_add),
                                  _p(arena), lda, arena.shape[0], _p(tables.astate), _p(tables.abase),
                                  _p(tables.bias_n), _p(tables.bias_tok), _p(tables.bias_val), _p(tables.min_until),
                                  _p(tables.minp_delta), _p(tables.fault), _p(tables.eos), _stream())
    _check(rc, "lsa_logit_process")


__all__ = ["BIAS_MAX", "N_EOS", "MAX_STATES", "NEG_INF_BITS", "TABLES", "TokenAutomaton", "ArenaAllocator",
           "processed_values", "logit_process_reference", "logit_process", "logit_process_calls"]
