"""JSON-constrained decoding: a deterministic byte-level pushdown automaton with 1-bit stack
symbols, the hand-built automaton of RFC 8259 JSON text, the ctypes binding of
csrc/sampling/pda_mask.hip and the numpy reference of the same contract (the CPU implementation
and the tests' oracle).

The automaton (:class:`BytePDA`): ``next`` int16 ``[3, S, 256]`` (``1 <= S <= 1023``) and ``accept``
uint8 ``[S]``. Plane ``p`` is selected by the stack top: 0 = empty stack, 1 = top symbol 0, 2 = top
symbol 1. An entry is ``-1`` (dead) or ``e >= 0`` with ``state = e & 0x3FF`` and ``op = e >> 10``:
0 none, 1 push 0, 2 push 1, 3 pop. A configuration is ``(q, d, stack)`` with ``0 <= d <= 64`` and
``stack`` a uint64 whose bit ``i`` is the symbol at level ``i`` (bits ``>= d`` are zero); it accepts
iff ``accept[q] & 1`` and ``d == 0``. A step on byte ``b``: pick the plane by the top symbol; a dead
entry kills the walk; a push at ``d == 64`` kills it, otherwise it sets bit ``d`` and increments
``d``; a pop at ``d == 0`` kills it, otherwise it clears bit ``d - 1`` and decrements ``d``; then
the new ``q`` is taken.

Tables (``runtime.logit_stages.GrammarState`` holds them on the engine's device):

* ``ptab`` int16 ``[3, S, 256]`` and ``paccept`` uint8 ``[S]``: the one automaton of the stage;
* ``offsets`` / ``data`` (``ops.grammar.VocabBytes``) and ``eos`` int32 ``[8]``, shared with the regex;
* per slot: ``jstate`` int32 (``-1`` = none), ``jdepth`` int32, ``jstack`` int64 and the regex's
  ``gfault``.

Contract per row with slot ``s`` and input token ``t`` (``tokens_in`` may be None):

0. ``jstate[s] < 0``: the row is skipped - logits and state stay bit-identical, no table is read.
   ``jstate[s] >= S`` or ``jdepth[s]`` outside ``[0, 64]``: ``gfault[s] |= 4``, row skipped. A slot
   outside ``[0, n_slots)`` skips its row.
1. advance: ``t < 0`` or ``t`` an EOS id: nothing. Otherwise walk ``bytes(t)`` from the
   configuration; ``t >= V``, a token of length 0 or a walk that dies: the configuration stays and
   ``gfault[s] |= 1``; otherwise the three state words are stored.
2. ``allowed(v)`` for ``v < V`` from the configuration after step 1: an EOS id iff the
   configuration accepts; any other token iff it is non-empty and its walk stays alive through
   its last byte (its pushes and pops are not stored).
3. ``n`` = the number of allowed ``v``. ``n == 0``: ``gfault[s] |= 2`` and the row is left untouched;
   otherwise every ``v < V`` that is not allowed and whose logit is not already the bf16 pattern
   ``0xFF80`` becomes ``0xFF80``. Nothing else is written; columns ``>= V`` are never read or written.

There is no floating-point arithmetic: kernel and reference agree bitwise.
"""
from __future__ import annotations

import ctypes
import hashlib
from typing import Optional

import numpy as np
import torch

from .constraints import N_EOS, NEG_INF_BITS, _bits_of, _np
from .grammar import FAULT_STATE, FAULT_STUCK, FAULT_TOKEN, VocabBytes

TABLES = ("ptab", "paccept", "offsets", "data", "jstate", "jdepth", "jstack", "gfault", "eos")
MAX_DEPTH = 64
MAX_PDA_STATES = 1023
OP_NONE, OP_PUSH0, OP_PUSH1, OP_POP = 0, 1, 2, 3
_STATE_MASK, _OP_SHIFT, _ENTRY_END = 0x3FF, 10, 4 << 10
EMPTY, TOP0, TOP1 = 0, 1, 2        # the planes
_WS = b" \t\n\r"
_M64 = (1 << 64) - 1


class BytePDA:
    """A deterministic pushdown automaton over bytes with a binary stack alphabet (module
    docstring), start configuration ``(0, 0, 0)``. ``names``: an optional name per state, for
    error messages. ``digest`` identifies the content."""

    def __init__(self, next, accept, names=None):  # noqa: A002 - the table's name
        a, acc = np.asarray(next), np.asarray(accept)
        if a.ndim != 3 or a.shape[0] != 3 or a.shape[2] != 256 or a.dtype.kind not in "iu" or acc.shape != (a.shape[1],):
            raise ValueError("BytePDA: next must be an integer [3, states, 256] table and accept [states]")
        S = a.shape[1]
        if not 1 <= S <= MAX_PDA_STATES:
            raise ValueError(f"BytePDA: 1 <= states <= {MAX_PDA_STATES}, got {S}")
        if int(a.min()) < -1 or int(a.max()) >= _ENTRY_END:
            raise ValueError("BytePDA: entries must be -1 (dead) or state | op << 10 with op in 0..3")
        if int((a[a >= 0] & _STATE_MASK).max(initial=0)) >= S:
            raise ValueError(f"BytePDA: an entry's state is outside [0, {S})")
        if acc.dtype.kind not in "iub" or int(acc.min()) < 0 or int(acc.max()) > 255:
            raise ValueError("BytePDA: accept must hold bytes")
        self.next = np.ascontiguousarray(a, dtype=np.int16)
        self.accept = np.ascontiguousarray(acc, dtype=np.uint8)
        self.next.setflags(write=False)
        self.accept.setflags(write=False)
        self.names = None if names is None else tuple(str(n) for n in names)
        if self.names is not None and len(self.names) != S:
            raise ValueError("BytePDA: one name per state")
        h = hashlib.sha256(np.array([3, S, 256], dtype=np.int64).tobytes())
        h.update(self.next.tobytes())
        h.update(self.accept.tobytes())
        self.digest = h.hexdigest()

    @property
    def n_states(self) -> int:
        return self.next.shape[1]

    def name(self, q: int) -> str:
        return f"{q}" if self.names is None else f"{q} ({self.names[q]})"

    def __eq__(self, other):
        return isinstance(other, BytePDA) and other.digest == self.digest

    def __hash__(self):
        return hash(self.digest)

    def __repr__(self):
        return f"BytePDA(states={self.n_states}, digest={self.digest[:12]})"

    # ------------------------------------------------------------------ the plain walker
    def step(self, config, b: int):
        """One byte from ``config = (q, d, stack)``: the next configuration, or None once dead."""
        q, d, stack = config
        plane = EMPTY if d == 0 else TOP0 + ((stack >> (d - 1)) & 1)
        e = int(self.next[plane, q, b])
        if e < 0:
            return None
        op = e >> _OP_SHIFT
        if op == OP_PUSH0 or op == OP_PUSH1:
            if d == MAX_DEPTH:
                return None
            stack |= (op - OP_PUSH0) << d
            d += 1
        elif op == OP_POP:
            if d == 0:
                return None
            d -= 1
            stack &= ~(1 << d) & _M64
        return e & _STATE_MASK, d, stack

    def walk(self, data: bytes, config=(0, 0, 0)):
        """The configuration after ``data`` from ``config``, one byte at a time; None once dead."""
        for b in bytes(data):
            config = self.step(config, b)
            if config is None:
                return None
        return config

    def accepting(self, config) -> bool:
        return config is not None and bool(self.accept[config[0]] & 1) and config[1] == 0

    def alive(self, data: bytes) -> bool:
        return self.walk(data) is not None

    def accepts(self, data: bytes) -> bool:
        return self.accepting(self.walk(data))

    # ------------------------------------------------------------------ JSON
    @classmethod
    def json(cls, top_level: str = "object", max_ws: int = 2) -> "BytePDA":
        """The automaton of RFC 8259 JSON text, built by hand. ``top_level``: ``"object"`` (the
        top-level value is an object) or ``"any"``. A whitespace run (space, tab, LF, CR) where
        the RFC allows whitespace has at most ``max_ws`` bytes (``0 <= max_ws <= 8``). Strings: no
        bytes below 0x20, the escapes ``\\" \\\\ \\/ \\b \\f \\n \\r \\t \\uXXXX`` (any four hex
        digits), bytes from 0x80 on as well-formed UTF-8 (no overlongs, no surrogates, nothing above
        U+10FFFF). Numbers as the RFC defines them, ended by the following structural or
        whitespace byte. ``{`` pushes 0, ``[`` pushes 1; only ``, } ]`` and the end of input depend on
        the top symbol."""
        if top_level not in ("object", "any"):
            raise ValueError(f"BytePDA.json: top_level must be 'object' or 'any', got {top_level!r}")
        if isinstance(max_ws, bool) or not isinstance(max_ws, int) or not 0 <= max_ws <= 8:
            raise ValueError(f"BytePDA.json: max_ws must be an integer in [0, 8], got {max_ws!r}")
        key = (top_level, max_ws)
        if key not in _JSON_CACHE:
            _JSON_CACHE[key] = _build_json(top_level, max_ws)
        return _JSON_CACHE[key]


_JSON_CACHE: dict = {}


def _build_json(top_level: str, max_ws: int) -> BytePDA:
    names, rows, acc = [], [], []

    def sid(name: str) -> int:
        if name not in names:
            names.append(name)
            rows.append(np.full((3, 256), -1, dtype=np.int32))
            acc.append(0)
        return names.index(name)

    def put(src: str, bs, dst: str, op: int = OP_NONE, planes=(EMPTY, TOP0, TOP1)) -> None:
        s, e = sid(src), sid(dst) | op << _OP_SHIFT
        for p in planes:
            for b in bs:
                assert rows[s][p, b] == -1, (src, p, b)
                rows[s][p, b] = e

    digits, hexd = b"0123456789", b"0123456789abcdefABCDEF"

    def ws_family(fam: str, start_w: int = 0) -> None:
        """fam.w reads one more whitespace byte while w < max_ws."""
        for w in range(start_w, max_ws):
            put(f"{fam}.{w}", _WS, f"{fam}.{w + 1}")

    def value_start(src: str) -> None:
        put(src, b'"', "vstr")
        put(src, b"{", "obj_open.0", OP_PUSH0)
        put(src, b"[", "arr_open.0", OP_PUSH1)
        put(src, b"-", "num_minus")
        put(src, b"0", "num_zero")
        put(src, b"123456789", "num_int")
        put(src, b"t", "lit_t")
        put(src, b"f", "lit_f")
        put(src, b"n", "lit_n")

    def value_end(src: str) -> None:
        """What may follow a complete value: the only transitions that depend on the top symbol."""
        put(src, b",", "key.0", planes=(TOP0,))
        put(src, b",", "value.0", planes=(TOP1,))
        put(src, b"}", "after.0", OP_POP, planes=(TOP0,))
        put(src, b"]", "after.0", OP_POP, planes=(TOP1,))
        acc[sid(src)] = 1

    # state 0
    if top_level == "object":
        for w in range(max_ws + 1):
            put(f"start.{w}", b"{", "obj_open.0", OP_PUSH0)
        ws_family("start")
    else:
        sid("value.0")
    for w in range(max_ws + 1):
        put(f"obj_open.{w}", b'"', "kstr")
        put(f"obj_open.{w}", b"}", "after.0", OP_POP, planes=(TOP0,))
        put(f"key.{w}", b'"', "kstr")
        put(f"after_key.{w}", b":", "value.0")
        value_start(f"value.{w}")
        value_start(f"arr_open.{w}")
        put(f"arr_open.{w}", b"]", "after.0", OP_POP, planes=(TOP1,))
        value_end(f"after.{w}")
    for fam in ("obj_open", "key", "after_key", "value", "arr_open", "after"):
        ws_family(fam)
    # strings: a key ends in after_key.0, a value in after.0
    for s, end in (("kstr", "after_key.0"), ("vstr", "after.0")):
        put(s, b'"', end)
        put(s, b"\\", s + "_esc")
        put(s, [b for b in range(0x20, 0x80) if b not in b'"\\'], s)
        put(s + "_esc", b'"\\/bfnrt', s)
        put(s + "_esc", b"u", s + "_u0")
        for i in range(4):
            put(f"{s}_u{i}", hexd, s if i == 3 else f"{s}_u{i + 1}")
        put(s, range(0xC2, 0xE0), s + "_c1")
        put(s, [0xE0], s + "_e0")
        put(s, [b for b in range(0xE1, 0xF0) if b != 0xED], s + "_c2")
        put(s, [0xED], s + "_ed")
        put(s, [0xF0], s + "_f0")
        put(s, range(0xF1, 0xF4), s + "_c3")
        put(s, [0xF4], s + "_f4")
        put(s + "_c1", range(0x80, 0xC0), s)
        put(s + "_c2", range(0x80, 0xC0), s + "_c1")
        put(s + "_e0", range(0xA0, 0xC0), s + "_c1")
        put(s + "_ed", range(0x80, 0xA0), s + "_c1")
        put(s + "_c3", range(0x80, 0xC0), s + "_c2")
        put(s + "_f0", range(0x90, 0xC0), s + "_c2")
        put(s + "_f4", range(0x80, 0x90), s + "_c2")
    # numbers: the four states a number may end in behave like after.0 on what follows a value
    put("num_minus", b"0", "num_zero")
    put("num_minus", b"123456789", "num_int")
    put("num_int", digits, "num_int")
    put("num_dot", digits, "num_frac")
    put("num_frac", digits, "num_frac")
    put("num_e", b"+-", "num_esign")
    put("num_e", digits, "num_exp")
    put("num_esign", digits, "num_exp")
    put("num_exp", digits, "num_exp")
    for s in ("num_zero", "num_int"):
        put(s, b".", "num_dot")
    for s in ("num_zero", "num_int", "num_frac"):
        put(s, b"eE", "num_e")
    for s in ("num_zero", "num_int", "num_frac", "num_exp"):
        value_end(s)
        if max_ws:
            put(s, _WS, "after.1")
    # literals
    for word in (b"true", b"false", b"null"):
        for i in range(1, len(word)):
            src = "lit_" + word[:i].decode()
            put(src, word[i:i + 1], "after.0" if i == len(word) - 1 else "lit_" + word[:i + 1].decode())
    return BytePDA(np.stack(rows, axis=1).astype(np.int16), np.array(acc, dtype=np.uint8), names)


# ------------------------------------------------------------------------------ reference
def _walk_tokens(nxt: np.ndarray, vocab: VocabBytes, config, sel: Optional[np.ndarray] = None) -> tuple:
    """The vectorised walk from one configuration: ``(q int32, d int32, stack uint64)`` after the
    bytes of every token (``sel``: these token ids), ``q = -1`` = dead or length 0. Loop over the
    byte position, gather per position."""
    S = nxt.shape[1]
    off = vocab.offsets.astype(np.int64)
    start, ln = off[:-1], off[1:] - off[:-1]
    if sel is not None:
        sel = np.asarray(sel, dtype=np.int64)
        start, ln = start[sel], ln[sel]
    n = start.size
    q = np.full(n, int(config[0]), dtype=np.int32)
    d = np.full(n, int(config[1]), dtype=np.int32)
    st = np.full(n, int(config[2]) & _M64, dtype=np.uint64)
    q[ln == 0] = -1
    data = vocab.data
    one = np.uint64(1)
    for p in range(int(ln.max()) if n else 0):
        cols = np.nonzero((ln > p) & (q >= 0))[0]
        if not cols.size:
            break
        b = data[start[cols] + p].astype(np.int64)
        qc, dc, sc = q[cols].astype(np.int64), d[cols], st[cols]
        top = (sc >> np.maximum(dc - 1, 0).astype(np.uint64)) & one
        plane = np.where(dc > 0, TOP0 + top.astype(np.int64), EMPTY)
        e = nxt[plane, qc, b].astype(np.int64)
        op = e >> _OP_SHIFT
        nq = e & _STATE_MASK
        push, pop = (op == OP_PUSH0) | (op == OP_PUSH1), op == OP_POP
        dead = (e < 0) | (e >= _ENTRY_END) | (nq >= S) | (push & (dc == MAX_DEPTH)) | (pop & (dc == 0))
        bit = one << np.where(push, dc, np.maximum(dc - 1, 0)).clip(0, 63).astype(np.uint64)
        sc = np.where(push & (op == OP_PUSH1), sc | bit, np.where(pop, sc & ~bit, sc))
        dc = dc + push.astype(np.int32) - pop.astype(np.int32)
        ok = ~dead
        q[cols] = np.where(ok, nq, -1).astype(np.int32)
        d[cols] = np.where(ok, dc, d[cols])
        st[cols] = np.where(ok, sc, st[cols])
    return q, d, st


def allowed_reference(pda_next: np.ndarray, accept: np.ndarray, vocab: VocabBytes, config, eos) -> np.ndarray:
    """Step 2 for one row: bool ``[V]`` from ``config``."""
    ok = _walk_tokens(pda_next, vocab, config)[0] >= 0
    accepting = bool(accept[config[0]] & 1) and config[1] == 0
    for e in eos:
        if 0 <= int(e) < vocab.V:
            ok[int(e)] = accepting
    return ok


def allowed_python(pda: BytePDA, vocab: VocabBytes, config, eos) -> np.ndarray:
    """Step 2 by the plain per-token walker (the tests' cross-check of :func:`allowed_reference`)."""
    eos = {int(e) for e in eos}
    ok = np.zeros(vocab.V, dtype=bool)
    for v in range(vocab.V):
        if v in eos:
            ok[v] = pda.accepting(config)
        else:
            piece = vocab.token(v)
            ok[v] = bool(piece) and pda.walk(piece, config) is not None
    return ok


def pda_mask_reference(logits_bf16, V: int, tables, slot, tokens_in):
    """The contract in numpy, vectorised over tokens, the stacks as uint64 arrays. ``logits_bf16``:
    [rows, >= V] bf16 tensor (or uint16 bit patterns); ``tables``: an object with the attributes
    :data:`TABLES` (numpy or torch); ``slot``: per row; ``tokens_in``: per row or None. The inputs
    are not modified. Returns ``(logits, jstate, jdepth, jstack, gfault)``, ``jstack`` as int64."""
    was_tensor = isinstance(logits_bf16, torch.Tensor)
    one_row = (logits_bf16.dim() if was_tensor else np.ndim(logits_bf16)) == 1
    bits = _bits_of(logits_bf16)
    rows = bits.shape[0]
    nxt = _np(tables.ptab, np.int16).reshape(3, -1, 256)
    accept = _np(tables.paccept, np.uint8)
    vocab = VocabBytes(_np(tables.offsets, np.int32)[:V + 1], _np(tables.data, np.uint8))
    jstate, jdepth = _np(tables.jstate, np.int32).copy(), _np(tables.jdepth, np.int32).copy()
    jstack, gfault = _np(tables.jstack, np.int64).copy(), _np(tables.gfault, np.int32).copy()
    eos = [int(e) for e in _np(tables.eos, np.int32)]
    n_slots, S = jstate.size, nxt.shape[1]
    slot = [int(s) for s in (slot.tolist() if hasattr(slot, "tolist") else slot)]
    if tokens_in is None:
        tokens_in = [-1] * rows
    tokens_in = [int(t) for t in (tokens_in.tolist() if hasattr(tokens_in, "tolist") else tokens_in)]
    if not len(slot) == len(tokens_in) == rows:
        raise ValueError(f"pda_mask_reference: per-row arguments do not match {rows} rows")
    if bits.shape[1] < V or vocab.V != V:
        raise ValueError("pda_mask_reference: a row or the vocabulary is shorter than V")
    for r in range(rows):
        s = slot[r]
        if not 0 <= s < n_slots:
            continue
        q, d = int(jstate[s]), int(jdepth[s])
        if q < 0:
            continue
        if q >= S or not 0 <= d <= MAX_DEPTH:
            gfault[s] |= FAULT_STATE
            continue
        config = (q, d, int(jstack[s]) & ((1 << d) - 1))     # bits >= d are zero by contract
        t = tokens_in[r]
        if t >= 0 and t not in eos:
            nq = -1
            if t < V:
                wq, wd, ws = _walk_tokens(nxt, vocab, config, np.array([t]))
                nq = int(wq[0])
            if nq >= 0:
                config = (nq, int(wd[0]), int(ws[0]))
                jstate[s], jdepth[s] = config[0], config[1]
                jstack[s] = np.uint64(config[2]).astype(np.int64)
            else:
                gfault[s] |= FAULT_TOKEN
        ok = allowed_reference(nxt, accept, vocab, config, eos)
        if not ok.any():
            gfault[s] |= FAULT_STUCK
            continue
        row = bits[r, :V]
        row[~ok & (row != NEG_INF_BITS)] = NEG_INF_BITS
    if one_row:
        bits = bits[0]
    if was_tensor:
        bits = torch.from_numpy(bits.view(np.int16).copy()).view(torch.bfloat16)
    return bits, jstate, jdepth, jstack, gfault


# ------------------------------------------------------------------------------ vocabulary check
def check_vocab(pda: BytePDA, vocab: VocabBytes, eos_ids) -> None:
    """ValueError unless a request admitted under ``pda`` can never lose every column with this
    vocabulary: for every reachable ``(q, top)`` either the configuration can accept (and an EOS
    id exists), or some token walks alive from it whatever lies below the top - it makes no push
    (the depth limit cannot kill it) and, once it has popped the one known symbol, reads only bytes
    on which all three planes agree and pops no further. Under an empty stack nothing is unknown -
    the configuration is ``(q, 0, 0)`` - so there the exact walk decides, pushes included."""
    nxt = pda.next.astype(np.int32)
    S, V = pda.n_states, vocab.V
    eos = [int(e) for e in eos_ids if 0 <= int(e) < V]
    alive_e = nxt >= 0
    op, tgt = np.where(alive_e, nxt >> _OP_SHIFT, -1), nxt & _STATE_MASK
    # reachable (q, top): after a pop the top may be anything
    seen = np.zeros((3, S), dtype=bool)
    seen[EMPTY, 0] = True
    todo = [(EMPTY, 0)]
    while todo:
        p, q = todo.pop()
        for b in np.nonzero(alive_e[p, q])[0]:
            o, t = int(op[p, q, b]), int(tgt[p, q, b])
            if o == OP_POP and p == EMPTY:
                continue
            for p2 in {OP_NONE: (p,), OP_PUSH0: (TOP0,), OP_PUSH1: (TOP1,), OP_POP: (EMPTY, TOP0, TOP1)}[o]:
                if not seen[p2, t]:
                    seen[p2, t] = True
                    todo.append((p2, t))
    ln = np.diff(vocab.offsets)
    one = ln == 1
    one[eos] = False                      # an EOS id's own bytes are ignored
    single = np.zeros(256, dtype=bool)
    single[vocab.data[vocab.offsets[:-1][one]]] = True
    # the cheap sufficient test: a one-byte token that does not push (on an empty stack: does not pop)
    empty = (np.arange(3) == EMPTY)[:, None, None]
    safe = alive_e & np.where(empty, op != OP_POP, (op == OP_NONE) | (op == OP_POP))
    good = (safe & single[None, None, :]).any(axis=2)
    if eos:
        good[EMPTY] |= (pda.accept & 1).astype(bool)
    agree = (nxt[0] == nxt[1]) & (nxt[1] == nxt[2]) & alive_e[0] & (op[0] == OP_NONE)   # [S, 256]: top-blind steps
    walkable = ln > 0
    walkable[eos] = False
    ids = np.nonzero(walkable)[0]
    for p, q in zip(*np.nonzero(seen & ~good)):
        if p == EMPTY:
            st = _walk_tokens(nxt, vocab, (int(q), 0, 0), ids)[0]
        else:
            st = _walk_known_top(nxt, op, agree, vocab, ids, int(p), int(q))
        if not (st >= 0).any():
            top = ("an empty stack", "an object on top", "an array on top")[int(p)]
            raise ValueError(f"json: state {pda.name(int(q))} of the automaton under {top} allows no token of this "
                             "vocabulary (no token's bytes continue the text there)")


def _walk_known_top(nxt, op, agree, vocab: VocabBytes, ids, p: int, q: int) -> np.ndarray:
    """The walk of the tokens ``ids`` from state ``q`` under the known top symbol of plane ``p`` and
    an unknown stack below it (:func:`check_vocab`): the state reached, -1 = not safely alive."""
    off, data, ln = vocab.offsets.astype(np.int64), vocab.data, np.diff(vocab.offsets)
    st = np.full(ids.size, q, dtype=np.int64)
    known = np.ones(ids.size, dtype=bool)         # the top symbol is still the known one
    for pos in range(int(ln[ids].max()) if ids.size else 0):
        cols = np.nonzero((ln[ids] > pos) & (st >= 0))[0]
        if not cols.size:
            break
        b = data[off[ids[cols]] + pos].astype(np.int64)
        sc, kc = st[cols], known[cols]
        e_known, o_known = nxt[p, sc, b], op[p, sc, b]
        ok_known = kc & (e_known >= 0) & ((o_known == OP_NONE) | (o_known == OP_POP))
        ok_blind = ~kc & agree[sc, b]
        st[cols] = np.where(ok_known, e_known & _STATE_MASK, np.where(ok_blind, nxt[0, sc, b] & _STATE_MASK, -1))
        known[cols] = kc & ~(ok_known & (o_known == OP_POP))
    return st


# ------------------------------------------------------------------------------ HIP binding
_declared = None


def _lib() -> ctypes.CDLL:
    """The kernel library (``hip.lib()``) with the entry points of pda_mask.hip declared."""
    global _declared
    from . import hip
    L = hip.lib()
    if _declared is not L:
        vp, i, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
        if not hasattr(L, "lsa_pda_mask"):
            raise RuntimeError("the kernel library has no lsa_pda_mask: rebuild it (python csrc/build.py)")
        L.lsa_pda_mask.argtypes = [vp, ll, i, i, vp, i, vp, vp, vp, i, vp, vp, ll, vp, vp, vp, vp, vp, vp]
        L.lsa_pda_mask.restype = i
        for name, res in (("lsa_pda_mask_calls", ll), ("lsa_pda_mask_lds_states", i), ("lsa_pda_mask_threads", i),
                          ("lsa_pda_mask_max_v", i)):
            getattr(L, name).argtypes = []
            getattr(L, name).restype = res
        _declared = L
    return L


def pda_mask_calls() -> int:
    """How often this process has enqueued ``lsa_pda_mask`` (a captured graph counts at capture)."""
    return int(_lib().lsa_pda_mask_calls())


def lds_states() -> int:
    """Automata of up to this many states are walked from LDS, larger ones from global memory."""
    return int(_lib().lsa_pda_mask_lds_states())


def block_threads() -> int:
    return int(_lib().lsa_pda_mask_threads())


def max_vocab() -> int:
    """The largest ``V`` the kernel takes (the allow bits of a row stay in registers)."""
    return int(_lib().lsa_pda_mask_max_v())


def pda_mask(logits: torch.Tensor, V: int, rows: int, slot: torch.Tensor, tokens_in: Optional[torch.Tensor],
             tables) -> None:
    """``lsa_pda_mask``: advance the configurations of the slots ``slot`` (int32 [rows], distinct) by
    ``tokens_in`` (int32 [rows] or None) and mask the first ``rows`` rows of bf16 ``logits``
    [>= rows, ld >= V] in place; ``tables``: an object with the attributes :data:`TABLES` as cuda
    tensors. No host reads: graph-capturable."""
    from .hip import _check, _p, _req, _stream
    from .sampling import _chk
    _req(logits.is_cuda and logits.dtype == torch.bfloat16 and logits.dim() == 2 and logits.stride(1) == 1,
         "pda_mask: logits must be a row-major bf16 cuda matrix")
    _req(1 <= rows <= logits.shape[0] and 1 <= V <= logits.shape[1] and rows <= 32768,
         f"pda_mask: rows={rows}, V={V} outside logits {tuple(logits.shape)} (at most 32768 rows)")
    _req(rows == 1 or logits.stride(0) >= V, "pda_mask: row stride below V")
    _req(all(getattr(tables, k, None) is not None for k in TABLES), "pda_mask: a table is missing")
    ptab, data = tables.ptab, tables.data
    _req(ptab.is_cuda and ptab.dtype == torch.int16 and ptab.dim() == 3 and ptab.shape[0] == 3 and ptab.shape[2] == 256
         and ptab.is_contiguous() and ptab.device == logits.device and 1 <= ptab.shape[1] <= MAX_PDA_STATES,
         "pda_mask: ptab must be a contiguous int16 cuda table [3, states <= 1023, 256] on the logits' device")
    _chk(tables.paccept, torch.uint8, ptab.shape[1], "paccept")
    _chk(tables.offsets, torch.int32, V + 1, "offsets")
    _req(data.is_cuda and data.dtype == torch.uint8 and data.dim() == 1 and data.is_contiguous()
         and data.numel() % 4 == 0 and data.numel() >= 4, "pda_mask: data must be contiguous uint8, a multiple of 4 bytes")
    n_slots = tables.jstate.numel()
    _req(n_slots >= 1, "pda_mask: empty slot tables")
    _chk(slot, torch.int32, rows, "slot")
    if tokens_in is not None:
        _chk(tokens_in, torch.int32, rows, "tokens_in")
    for k in ("jstate", "jdepth", "gfault"):
        _chk(getattr(tables, k), torch.int32, n_slots, k)
    _chk(tables.jstack, torch.int64, n_slots, "jstack")
    _chk(tables.eos, torch.int32, N_EOS, "eos")
    ld = logits.stride(0) if rows > 1 else max(logits.stride(0), V)
    rc = _lib().lsa_pda_mask(_p(logits), ld, V, rows, _p(slot), n_slots, _p(tokens_in), _p(ptab), _p(tables.paccept),
                             ptab.shape[1], _p(tables.offsets), _p(data), data.numel(), _p(tables.jstate),
                             _p(tables.jdepth), _p(tables.jstack), _p(tables.gfault), _p(tables.eos), _stream())
    _check(rc, "lsa_pda_mask")


__all__ = ["TABLES", "MAX_DEPTH", "MAX_PDA_STATES", "OP_NONE", "OP_PUSH0", "OP_PUSH1", "OP_POP", "BytePDA",
           "allowed_reference", "allowed_python", "pda_mask_reference", "check_vocab", "pda_mask", "pda_mask_calls",
           "lds_states", "block_threads", "max_vocab"]
