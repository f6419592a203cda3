"""Regex-constrained decoding: a byte-level DFA compiled from a regular expression, the byte
strings of a vocabulary, the ctypes binding of csrc/sampling/grammar_mask.hip and the numpy
reference of the same contract (the CPU implementation and the tests' oracle).

The automaton runs over **bytes** (``[states, 256]`` int16, 512 B per state, independent of the
vocabulary); which tokens survive is decided per step: a token survives when its byte string walks
through the automaton from the sequence's current state without dying.

Tables (``runtime.sampling.GrammarState`` holds them on the engine's device):

* ``arena`` int16 ``[dfa_rows, 256]``: one row per DFA state; an entry is the next state relative
  to the automaton's first row, ``-1`` = dead;
* ``accept`` uint8 ``[dfa_rows]``: bit 0 = the state accepts (the output may end here), bit 1 =
  the row is the last one of its automaton (how the kernel learns an automaton's size);
* ``offsets`` int32 ``[V + 1]`` and ``data`` uint8 (a multiple of 4 bytes): the byte string of every
  token; length 0 = a special or unknown token, never allowed;
* per slot: ``gstate`` int32 (arena row of the current state, -1 = no grammar), ``gbase`` int32
  (arena row of the automaton's state 0) and ``gfault`` int32;
* ``eos`` int32 ``[8]``: the EOS ids, padded with -1.

Contract per row with slot ``s`` and input token ``t`` (``tokens_in`` may be None):

0. ``gstate[s] < 0``: the row is skipped - logits and state stay bit-identical, no table is read.
   (A state or base outside the arena sets ``gfault[s] |= 4`` and skips the row as well.)
1. advance: ``t < 0`` or ``t`` an EOS id: nothing. Otherwise walk ``bytes(t)`` from
   ``q = gstate[s]``; ``t >= V``, a token of length 0 or a walk that dies: the state stays and
   ``gfault[s] |= 1``; otherwise ``gstate[s] = gbase[s] + walked state``;
2. ``allowed(v)`` for ``v < V`` from the state after step 1: an EOS id: ``accept[q] & 1`` (its own
   bytes are ignored); any other token: ``len(v) > 0`` and the walk of ``bytes(v)`` from ``q``
   stays alive through its last byte;
3. ``n`` = the number of allowed ``v``. ``n == 0``: ``gfault[s] |= 2`` and the row is left
   untouched; otherwise every ``v < V`` that is not allowed and whose logit is not already the
   bf16 pattern ``0xFF80`` becomes ``0xFF80``. Nothing else is written; columns ``>= V`` are never
   read or written.

There is no floating-point arithmetic: kernel and reference agree bitwise.
"""
from __future__ import annotations

import ctypes
import hashlib
from typing import Optional

import numpy as np
import torch

from .constraints import MAX_STATES, N_EOS, NEG_INF_BITS, TokenAutomaton, _bits_of, _np

TABLES = ("arena", "accept", "offsets", "data", "gstate", "gbase", "gfault", "eos")
ACCEPT, LAST = 1, 2         # bits of the accept table
FAULT_TOKEN, FAULT_STUCK, FAULT_STATE = 1, 2, 4
MAX_NFA = 1 << 18           # Thompson nodes: a bound on what {m,n} may expand to

# ------------------------------------------------------------------------------ regex -> AST
_DIGIT = frozenset(range(0x30, 0x3A))
_WORD = frozenset(range(0x30, 0x3A)) | frozenset(range(0x41, 0x5B)) | frozenset(range(0x61, 0x7B)) | {0x5F}
_SPACE = frozenset(b" \t\n\r\f\v")
_ALL = frozenset(range(256))
_CLASSES = {"d": _DIGIT, "D": _ALL - _DIGIT, "w": _WORD, "W": _ALL - _WORD, "s": _SPACE, "S": _ALL - _SPACE}
_CHAR_ESC = {"n": 0x0A, "t": 0x09, "r": 0x0D}
_PUNCT = frozenset("!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~ ")
_HEX = "0123456789abcdefABCDEF"


class _Parser:
    """Recursive descent over the pattern (a str). AST nodes: ``("set", frozenset)``,
    ``("cat", [nodes])``, ``("alt", [nodes])``, ``("rep", node, m, n or None)``."""

    def __init__(self, pattern: str):
        if not isinstance(pattern, str):
            raise ValueError(f"regex: the pattern must be a str, got {type(pattern).__name__}")
        self.p, self.i = pattern, 0

    def err(self, what: str, at: Optional[int] = None):
        at = self.i if at is None else at
        return ValueError(f"regex: {what} at position {at} of {self.p!r}")

    def peek(self) -> str:
        return self.p[self.i] if self.i < len(self.p) else ""

    def parse(self):
        node = self.alt()
        if self.i < len(self.p):
            raise self.err("unbalanced ')'")
        return node

    def alt(self):
        branches = [self.cat()]
        while self.peek() == "|":
            self.i += 1
            branches.append(self.cat())
        return branches[0] if len(branches) == 1 else ("alt", branches)

    def cat(self):
        items = []
        while self.i < len(self.p) and self.peek() not in "|)":
            at = self.i
            atom, quantifiable = self.atom()
            q = self.quantifier()
            if q is not None:
                if not quantifiable:
                    raise self.err("a quantifier on a non-ASCII literal (wrap the character in a group)", at)
                atom = ("rep", atom, q[0], q[1])
                c = self.peek()
                if c == "?":
                    raise self.err("unsupported lazy quantifier")
                if c == "+":
                    raise self.err("unsupported possessive quantifier")
                if c == "*" or (c == "{" and self.braces() is not None):
                    raise self.err("multiple repeat")
            items.append(atom)
        return items[0] if len(items) == 1 else ("cat", items)

    def braces(self):
        """``{m} {m,} {m,n} {,n}`` at the cursor: ``(m, n, end)`` or None (then '{' is a literal,
        as in Python's re)."""
        j = self.p.find("}", self.i)
        if j < 0:
            return None
        body = self.p[self.i + 1:j]
        lo, sep, hi = body.partition(",")
        if not ((lo.isdigit() and lo.isascii()) or (sep and lo == "")) or not (hi == "" or (hi.isdigit() and hi.isascii())):
            return None
        if not sep and not lo:
            return None
        if sep and not lo and not hi:
            return None
        m = int(lo) if lo else 0
        n = m if not sep else (int(hi) if hi else None)
        return m, n, j + 1

    def quantifier(self):
        c = self.peek()
        if c == "*":
            self.i += 1
            return 0, None
        if c == "+":
            self.i += 1
            return 1, None
        if c == "?":
            self.i += 1
            return 0, 1
        if c == "{":
            b = self.braces()
            if b is None:
                return None
            m, n, end = b
            if n is not None and n < m:
                raise self.err(f"bad repeat interval {{{m},{n}}}")
            if max(m, n or 0) > MAX_NFA:
                raise self.err("repeat count too large")
            self.i = end
            return m, n
        return None

    def atom(self):
        """One atom: ``(node, quantifiable)``."""
        c = self.peek()
        at = self.i
        if c == "(":
            self.i += 1
            if self.peek() == "?":
                nxt = self.p[self.i + 1:self.i + 2]
                if nxt != ":":
                    names = {"=": "look-ahead (?=", "!": "look-ahead (?!", "<": "look-behind or named group (?<",
                             "P": "named group or reference (?P", "#": "comment (?#", "(": "conditional (?("}
                    raise self.err("unsupported " + names.get(nxt, f"inline flag (?{nxt}"), at)
                self.i += 2
            node = self.alt()
            if self.peek() != ")":
                raise self.err("missing ')'", at)
            self.i += 1
            return node, True
        if c in "*+?":
            raise self.err("nothing to repeat")
        if c == "{" and self.braces() is not None:
            raise self.err("nothing to repeat")
        if c == "^" or c == "$":
            raise self.err(f"unsupported anchor '{c}' (the whole output is matched)")
        self.i += 1
        if c == ".":
            return ("set", _ALL - {0x0A}), True
        if c == "[":
            return ("set", self.char_class(at)), True
        if c == "\\":
            e = self.escape(at, in_class=False)
            return ("set", e if isinstance(e, frozenset) else frozenset((e,))), True
        if ord(c) < 0x80:
            return ("set", frozenset((ord(c),))), True
        return ("cat", [("set", frozenset((b,))) for b in c.encode("utf-8")]), False

    def escape(self, at: int, in_class: bool):
        """The escape whose backslash was just consumed: a byte or a frozenset of bytes."""
        if self.i >= len(self.p):
            raise self.err("a trailing backslash", at)
        c = self.p[self.i]
        self.i += 1
        if c in _CLASSES:
            return _CLASSES[c]
        if c in _CHAR_ESC:
            return _CHAR_ESC[c]
        if c == "x":
            h = self.p[self.i:self.i + 2]
            if len(h) != 2 or h[0] not in _HEX or h[1] not in _HEX:
                raise self.err("incomplete escape \\x", at)
            self.i += 2
            return int(h, 16)
        if c in _PUNCT:
            return ord(c)
        if c.isdigit():
            raise self.err(f"unsupported back-reference or octal escape \\{c}", at)
        if c in "AZbB":
            raise self.err(f"unsupported anchor \\{c}", at)
        raise self.err(f"unsupported escape \\{c}", at)

    def char_class(self, at: int) -> frozenset:
        neg = self.peek() == "^"
        if neg:
            self.i += 1
        members, first = set(), True
        while True:
            if self.i >= len(self.p):
                raise self.err("unterminated character class", at)
            c = self.p[self.i]
            if c == "]" and not first:
                self.i += 1
                break
            first = False
            lo = self.class_item()
            if self.peek() == "-" and self.p[self.i + 1:self.i + 2] not in ("]", ""):
                self.i += 1
                hi = self.class_item()
                if isinstance(lo, frozenset) or isinstance(hi, frozenset):
                    raise self.err("bad character range (a class shorthand as an end point)", at)
                if hi < lo:
                    raise self.err(f"bad character range {chr(lo)}-{chr(hi)}", at)
                members.update(range(lo, hi + 1))
            elif isinstance(lo, frozenset):
                members |= lo
            else:
                members.add(lo)
        return frozenset(_ALL - members) if neg else frozenset(members)

    def class_item(self):
        c = self.p[self.i]
        at = self.i
        self.i += 1
        if c == "\\":
            return self.escape(at, in_class=True)
        if ord(c) >= 0x80:
            raise self.err("a non-ASCII character in a character class", at)
        return ord(c)


# ------------------------------------------------------------------------------ AST -> NFA -> DFA
class _NFA:
    def __init__(self):
        self.eps, self.trans = [], []   # per node: epsilon targets; [(frozenset of bytes, target)]

    def new(self) -> int:
        if len(self.eps) >= MAX_NFA:
            raise ValueError(f"regex: the pattern expands to more than {MAX_NFA} NFA states")
        self.eps.append([])
        self.trans.append([])
        return len(self.eps) - 1

    def build(self, node, start: int) -> int:
        """Thompson construction: the fragment of ``node`` from ``start``; returns its end node."""
        kind = node[0]
        if kind == "set":
            end = self.new()
            if node[1]:
                self.trans[start].append((node[1], end))
            return end
        if kind == "cat":
            cur = start
            for ch in node[1]:
                cur = self.build(ch, cur)
            return cur
        if kind == "alt":
            end = self.new()
            for ch in node[1]:
                s = self.new()
                self.eps[start].append(s)
                self.eps[self.build(ch, s)].append(end)
            return end
        _, ch, m, n = node
        cur = start
        for _ in range(m):
            cur = self.build(ch, cur)
        end = self.new()
        if n is None:       # loop: s -> body -> s, s -> end
            s = self.new()
            self.eps[cur].append(s)
            self.eps[self.build(ch, s)].append(s)
            self.eps[s].append(end)
        else:               # every optional copy may leave straight to the end
            self.eps[cur].append(end)
            for _ in range(n - m):
                s = self.new()
                self.eps[cur].append(s)
                cur = self.build(ch, s)
                self.eps[cur].append(end)
        return end


def _byte_classes(sets) -> tuple:
    """The coarsest partition of 0..255 that no set of ``sets`` splits: ``(class of byte [256],
    one representative byte per class)``, classes numbered by their smallest byte."""
    sig = [0] * 256
    for k, s in enumerate(sets):
        for b in s:
            sig[b] |= 1 << k
    ids, cls, reps = {}, np.zeros(256, dtype=np.int64), []
    for b in range(256):
        if sig[b] not in ids:
            ids[sig[b]] = len(reps)
            reps.append(b)
        cls[b] = ids[sig[b]]
    return cls, reps


def _closure(nfa: _NFA, seeds) -> frozenset:
    seen, stack = set(seeds), list(seeds)
    while stack:
        for t in nfa.eps[stack.pop()]:
            if t not in seen:
                seen.add(t)
                stack.append(t)
    return frozenset(seen)


def _subset(nfa: _NFA, start: int, final: int, reps, limit: int) -> tuple:
    """Subset construction over the byte classes: ``(T int32 [S, C] with -1 = dead, accept [S])``."""
    memo = {}

    def close1(t):
        c = memo.get(t)
        if c is None:
            c = memo[t] = _closure(nfa, (t,))
        return c

    s0 = close1(start)
    index, order, rows = {s0: 0}, [s0], []
    k = 0
    while k < len(order):
        cur = order[k]
        k += 1
        moves = [(bs, t) for q in cur for bs, t in nfa.trans[q]]
        row = []
        for rep in reps:
            tgt = set()
            for bs, t in moves:
                if rep in bs:
                    tgt |= close1(t)
            if not tgt:
                row.append(-1)
                continue
            key = frozenset(tgt)
            j = index.get(key)
            if j is None:
                j = index[key] = len(order)
                order.append(key)
                if j >= limit:
                    raise ValueError(f"regex: the automaton needs more than {limit} states before minimisation")
            row.append(j)
        rows.append(row)
    T = np.array(rows, dtype=np.int32).reshape(len(order), len(reps))
    return T, np.array([final in s for s in order], dtype=bool)


def _trim(T: np.ndarray, accept: np.ndarray) -> tuple:
    """Drop the states that cannot reach an accepting state (every state is reachable by
    construction). ValueError when state 0 goes: the language is empty."""
    S = T.shape[0]
    rev = [[] for _ in range(S)]
    for s, c in zip(*np.nonzero(T >= 0)):
        rev[T[s, c]].append(int(s))
    live = accept.copy()
    stack = [int(s) for s in np.nonzero(accept)[0]]
    while stack:
        for p in rev[stack.pop()]:
            if not live[p]:
                live[p] = True
                stack.append(p)
    if not live[0]:
        raise ValueError("regex: the pattern matches nothing (empty language)")
    new = np.full(S + 1, -1, dtype=np.int32)   # slot S serves the -1 entries
    new[:S][live] = np.arange(int(live.sum()), dtype=np.int32)
    return new[T[live]], accept[live]


def _minimise(T: np.ndarray, accept: np.ndarray) -> tuple:
    """Hopcroft's partition refinement on the DFA completed by one dead state."""
    S, C = T.shape
    dead = S
    full = np.vstack([np.where(T < 0, dead, T), np.full((1, C), dead, dtype=T.dtype)])
    inv = [[[] for _ in range(S + 1)] for _ in range(C)]
    for c in range(C):
        col = full[:, c].tolist()
        ic = inv[c]
        for s, t in enumerate(col):
            ic[t].append(s)
    blocks = [b for b in (set(np.nonzero(accept)[0].tolist()), set(np.nonzero(~accept)[0].tolist()) | {dead}) if b]
    block_of = [0] * (S + 1)
    for i, b in enumerate(blocks):
        for s in b:
            block_of[s] = i
    work = set(range(len(blocks)))
    while work:
        a = list(blocks[work.pop()])
        for c in range(C):
            ic = inv[c]
            touched = {}
            for t in a:
                for s in ic[t]:
                    touched.setdefault(block_of[s], set()).add(s)
            for bi, part in touched.items():
                whole = blocks[bi]
                if len(part) == len(whole):
                    continue
                rest = whole - part
                small, large = (part, rest) if len(part) <= len(rest) else (rest, part)
                blocks[bi] = large
                ni = len(blocks)
                blocks.append(small)
                for s in small:
                    block_of[s] = ni
                work.add(ni)   # the smaller half always suffices, whether bi waits or not
    # number the blocks breadth-first from the start state, classes in byte order: one numbering
    # per language
    dead_block = block_of[dead]
    num, order = {block_of[0]: 0}, [block_of[0]]
    k = 0
    rows = []
    while k < len(order):
        s = next(iter(blocks[order[k]]))
        k += 1
        row = []
        for c in range(C):
            b = block_of[int(full[s, c])]
            if b == dead_block:
                row.append(-1)
                continue
            if b not in num:
                num[b] = len(order)
                order.append(b)
            row.append(num[b])
        rows.append(row)
    T2 = np.array(rows, dtype=np.int32).reshape(len(order), C)
    acc2 = np.array([bool(accept[next(iter(blocks[b]))]) for b in order], dtype=bool)
    return T2, acc2


class ByteDFA:
    """A trimmed, minimal deterministic automaton over bytes: ``next`` int16 ``[S, 256]`` (``-1`` =
    dead), ``accept`` bool ``[S]``, start state 0, ``1 <= S <= 32767``. Every state is reachable
    from 0 and can reach an accepting state: a live state has a completion. ``digest`` identifies
    the content (states are numbered breadth-first in byte order, so two spellings of one language
    give one digest)."""

    def __init__(self, next, accept):  # noqa: A002 - the table's name
        a, acc = np.asarray(next), np.asarray(accept, dtype=bool)
        if a.ndim != 2 or a.shape[1] != 256 or a.dtype.kind not in "iu" or acc.shape != (a.shape[0],):
            raise ValueError("ByteDFA: next must be an integer [states, 256] table and accept [states]")
        S = a.shape[0]
        if not 1 <= S <= MAX_STATES:
            raise ValueError(f"ByteDFA: 1 <= states <= {MAX_STATES}, got {S}")
        if int(a.min()) < -1 or int(a.max()) >= S:
            raise ValueError(f"ByteDFA: entries must be -1 (dead) or a state in [0, {S})")
        self.next = np.ascontiguousarray(a, dtype=np.int16)
        self.accept = np.ascontiguousarray(acc)
        self.next.setflags(write=False)
        self.accept.setflags(write=False)
        h = hashlib.sha256(np.array([S, 256], dtype=np.int64).tobytes())
        h.update(self.next.tobytes())
        h.update(self.accept.tobytes())
        self.digest = h.hexdigest()
        self.pattern = None

    @property
    def n_states(self) -> int:
        return self.next.shape[0]

    def __eq__(self, other):
        return isinstance(other, ByteDFA) and other.digest == self.digest

    def __hash__(self):
        return hash(self.digest)

    def __repr__(self):
        return f"ByteDFA(states={self.n_states}, digest={self.digest[:12]}, pattern={self.pattern!r})"

    @classmethod
    def from_regex(cls, pattern: str, max_states: int = MAX_STATES) -> "ByteDFA":
        """Compile ``pattern`` with the semantics of ``re.fullmatch(pattern.encode(), data)``:
        whole-string, byte-level. Supported: literals (a non-ASCII character outside a class is its
        UTF-8 byte sequence), ``\\\\ \\. \\n \\t \\r \\xHH`` and escaped punctuation, ``\\d \\D \\w \\W \\s
        \\S`` (ASCII), ``.`` (any byte but ``\\n``), ``[...]`` with ranges and negation, ``( )``,
        ``(?: )``, ``|``, ``* + ?``, ``{m} {m,} {m,n}``. Anything else raises ValueError naming the
        construct, as do an empty language and more than ``max_states`` states."""
        max_states = min(int(max_states), MAX_STATES)
        if max_states < 1:
            raise ValueError("regex: max_states must be at least 1")
        ast = _Parser(pattern).parse()
        nfa = _NFA()
        start = nfa.new()
        final = nfa.build(ast, start)
        cls_of, reps = _byte_classes(list({bs for tr in nfa.trans for bs, _ in tr}))
        T, acc = _subset(nfa, start, final, reps, 4 * max_states + 256)
        T, acc = _minimise(*_trim(T, acc))
        if T.shape[0] > max_states:
            raise ValueError(f"regex: the automaton of {pattern!r} has {T.shape[0]} states, more than {max_states}")
        dfa = cls(T[:, cls_of].astype(np.int16), acc)
        dfa.pattern = pattern
        return dfa

    def walk(self, data: bytes, state: int = 0) -> int:
        """The state after feeding ``data`` from ``state``; -1 once dead."""
        nx = self.next
        for b in bytes(data):
            if state < 0:
                return -1
            state = int(nx[state, b])
        return state

    def accepts(self, data: bytes) -> bool:
        q = self.walk(data)
        return q >= 0 and bool(self.accept[q])

    def step_tokens(self, vocab: "VocabBytes", states: np.ndarray, sel: Optional[np.ndarray] = None) -> np.ndarray:
        """The vectorised walk: the state after the bytes of every token (``sel``: these token
        ids) from each of ``states`` - int32 ``[len(states), n_tokens]``, -1 = dead or length 0."""
        return _walk_tokens(self.next, vocab, np.asarray(states, dtype=np.int64), sel)

    def to_token_automaton(self, vocab: "VocabBytes", eos_ids) -> TokenAutomaton:
        """The dense equivalent over token ids (for small cases and cross-checks): state ``q``
        allows the tokens whose bytes stay alive from ``q``; accepting states also allow the EOS
        ids, which lead to an absorbing state that allows only them (as ``from_choices`` does)."""
        S, V = self.n_states, vocab.V
        eos = [int(e) for e in eos_ids or () if 0 <= int(e) < V]
        if S + 1 > MAX_STATES:
            raise ValueError(f"to_token_automaton: {S + 1} states, more than {MAX_STATES}")
        t = np.full((S + 1, V), -1, dtype=np.int16)
        t[:S] = self.step_tokens(vocab, np.arange(S)).astype(np.int16)
        if eos:
            t[:S, eos] = -1
            t[np.nonzero(self.accept)[0][:, None], np.array(eos)[None, :]] = S
            t[S, eos] = S
        else:
            t = t[:S]
        return TokenAutomaton(t)


def _walk_tokens(nxt: np.ndarray, vocab: "VocabBytes", states: np.ndarray, sel: Optional[np.ndarray] = None) -> np.ndarray:
    """Loop over the byte position, gather per position: every token still alive and not yet at
    its end takes one step."""
    off = vocab.offsets.astype(np.int64)
    if sel is not None:
        sel = np.asarray(sel, dtype=np.int64)
        start, ln = off[:-1][sel], (off[1:] - off[:-1])[sel]
    else:
        start, ln = off[:-1], off[1:] - off[:-1]
    q = np.broadcast_to(states[:, None], (states.size, start.size)).astype(np.int32).copy()
    q[:, ln == 0] = -1
    data = vocab.data
    for p in range(int(ln.max()) if ln.size else 0):
        cols = np.nonzero(ln > p)[0]
        if not cols.size:
            break
        b = data[start[cols] + p].astype(np.int64)
        cur = q[:, cols]
        q[:, cols] = np.where(cur >= 0, nxt[np.maximum(cur, 0), b[None, :]], -1)
    return q


# ------------------------------------------------------------------------------ vocabulary bytes
def _gpt2_unicode_to_byte() -> dict:
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAD)) + list(range(0xAE, 0x100))
    cs, n = bs[:], 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return {chr(c): b for b, c in zip(bs, cs)}


_U2B = _gpt2_unicode_to_byte()


def pieces_to_bytes(pieces, kind: str, special=()) -> list:
    """The byte string of every piece string of a tokenizer's vocabulary. ``kind="sentencepiece"``:
    ``▁`` is a space, ``<0xNN>`` is that byte, any other ``<...>`` piece is special (empty);
    ``kind="bytelevel"``: GPT-2's unicode-to-byte table, a piece with a character outside it is
    special. ``special``: pieces that are special whatever they look like. None pieces are empty."""
    special = set(special)
    out = []
    if kind not in ("sentencepiece", "bytelevel"):
        raise ValueError(f"pieces_to_bytes: kind must be 'sentencepiece' or 'bytelevel', got {kind!r}")
    for p in pieces:
        if p is None or p in special:
            out.append(b"")
        elif kind == "sentencepiece":
            if len(p) == 6 and p.startswith("<0x") and p.endswith(">") and all(c in _HEX for c in p[3:5]):
                out.append(bytes([int(p[3:5], 16)]))
            elif len(p) >= 2 and p.startswith("<") and p.endswith(">"):
                out.append(b"")
            else:
                out.append(p.replace("▁", " ").encode("utf-8"))
        else:
            out.append(bytes(_U2B[c] for c in p) if all(c in _U2B for c in p) else b"")
    return out


def detect_kind(pieces) -> str:
    """``"sentencepiece"`` when a piece carries ``▁`` or is a ``<0xNN>`` byte piece, else ``"bytelevel"``."""
    for p in pieces:
        if p and ("▁" in p or (len(p) == 6 and p.startswith("<0x") and p.endswith(">"))):
            return "sentencepiece"
    return "bytelevel"


class VocabBytes:
    """The byte string of every token id ``< V``: ``offsets`` int32 ``[V + 1]`` into ``data`` uint8
    (padded with zeros to a multiple of 4 bytes plus 4, so a kernel may read whole dwords). Length
    0 marks a special or unknown token, which is never allowed."""

    def __init__(self, offsets, data):
        self.offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        total = int(self.offsets[-1]) if self.offsets.size else -1
        if self.offsets.ndim != 1 or self.offsets.size < 2 or self.offsets[0] != 0 or np.any(np.diff(self.offsets) < 0):
            raise ValueError("VocabBytes: offsets must be [V + 1] int32, ascending from 0, with V >= 1")
        d = np.asarray(data, dtype=np.uint8).reshape(-1)
        if d.size < total:
            raise ValueError(f"VocabBytes: offsets end at {total}, data holds {d.size} bytes")
        self.n_bytes = total
        self.data = np.zeros((total + 3) // 4 * 4 + 4, dtype=np.uint8)
        self.data[:total] = d[:total]
        self.offsets.setflags(write=False)
        self.data.setflags(write=False)
        ln = np.diff(self.offsets)
        self.single = np.zeros(256, dtype=bool)     # bytes that exist as a one-byte token
        self.single[self.data[self.offsets[:-1][ln == 1]]] = True

    @property
    def V(self) -> int:
        return self.offsets.size - 1

    def token(self, v: int) -> bytes:
        return self.data[self.offsets[v]:self.offsets[v + 1]].tobytes()

    def decode(self, ids) -> bytes:
        return b"".join(self.token(int(t)) for t in ids if 0 <= int(t) < self.V)

    @classmethod
    def from_pieces(cls, pieces) -> "VocabBytes":
        pieces = [bytes(p) for p in pieces]
        off = np.zeros(len(pieces) + 1, dtype=np.int64)
        np.cumsum([len(p) for p in pieces], out=off[1:])
        if off[-1] >= 1 << 31:
            raise ValueError("VocabBytes: more than 2 GiB of token bytes")
        return cls(off.astype(np.int32), np.frombuffer(b"".join(pieces), dtype=np.uint8))

    @classmethod
    def from_tokenizer(cls, tok, V: int) -> "VocabBytes":
        """``V`` token ids of ``tok``: the synthetic byte tokenizer (id ``offset + b`` is the one
        byte ``b``, everything else empty) or an HF tokenizer through ``convert_ids_to_tokens`` and
        its special-token list, the kind detected from the pieces."""
        V = int(V)
        if type(tok).__name__ == "SyntheticByteTokenizer":
            return cls.from_pieces([bytes([v - tok.offset]) if 0 <= v - tok.offset < 256 else b"" for v in range(V)])
        n = min(V, len(tok))
        pieces = list(tok.convert_ids_to_tokens(list(range(n)))) + [None] * (V - n)
        special = set(getattr(tok, "all_special_tokens", ()) or ())
        return cls.from_pieces(pieces_to_bytes(pieces, detect_kind(pieces), special))


# ------------------------------------------------------------------------------ reference
def _relative(arena: np.ndarray, base: int) -> np.ndarray:
    """The rows from ``base`` on as int32; an entry that would leave the arena is dead."""
    rel = arena[base:].astype(np.int32)
    return np.where(rel >= arena.shape[0] - base, -1, rel)


def allowed_reference(rel: np.ndarray, accepting: bool, vocab: VocabBytes, q: int, eos) -> np.ndarray:
    """Step 2 for one row: bool ``[V]`` from state ``q`` of the (relative) table ``rel``."""
    ok = _walk_tokens(rel, vocab, np.array([q], dtype=np.int64))[0] >= 0
    for e in eos:
        if 0 <= int(e) < vocab.V:
            ok[int(e)] = accepting
    return ok


def grammar_mask_reference(logits_bf16, V: int, tables, slot, tokens_in):
    """The contract in numpy, vectorised over tokens. ``logits_bf16``: [rows, >= V] bf16 tensor (or
    uint16 bit patterns); ``tables``: an object with the attributes :data:`TABLES` (numpy or
    torch); ``slot``: per row; ``tokens_in``: per row or None. The inputs are not modified. Returns
    ``(logits, gstate, gfault)``."""
    was_tensor = isinstance(logits_bf16, torch.Tensor)
    one_row = (logits_bf16.dim() if was_tensor else np.ndim(logits_bf16)) == 1
    bits = _bits_of(logits_bf16)
    rows = bits.shape[0]
    arena = _np(tables.arena, np.int16).reshape(-1, 256)
    accept = _np(tables.accept, np.uint8)
    vocab = VocabBytes(_np(tables.offsets, np.int32)[:V + 1], _np(tables.data, np.uint8))
    gstate, gfault = _np(tables.gstate, np.int32).copy(), _np(tables.gfault, np.int32).copy()
    gbase, eos = _np(tables.gbase, np.int32), [int(e) for e in _np(tables.eos, np.int32)]
    n_slots, dfa_rows = gstate.size, arena.shape[0]
    slot = [int(s) for s in (slot.tolist() if hasattr(slot, "tolist") else slot)]
    if tokens_in is None:
        tokens_in = [-1] * rows
    tokens_in = [int(t) for t in (tokens_in.tolist() if hasattr(tokens_in, "tolist") else tokens_in)]
    if not len(slot) == len(tokens_in) == rows:
        raise ValueError(f"grammar_mask_reference: per-row arguments do not match {rows} rows")
    if bits.shape[1] < V or vocab.V != V:
        raise ValueError("grammar_mask_reference: a row or the vocabulary is shorter than V")
    rels = {}
    for r in range(rows):
        s = slot[r]
        if not 0 <= s < n_slots:
            continue
        q = int(gstate[s])
        if q < 0:
            continue
        base = int(gbase[s])
        if q >= dfa_rows or base < 0 or base > q:
            gfault[s] |= FAULT_STATE
            continue
        rel = rels.get(base)
        if rel is None:
            rel = rels[base] = _relative(arena, base)
        t = tokens_in[r]
        if t >= 0 and t not in eos:
            n = int(_walk_tokens(rel, vocab, np.array([q - base]), np.array([t]))[0, 0]) if t < V else -1
            if n >= 0:
                q = base + n
                gstate[s] = q
            else:
                gfault[s] |= FAULT_TOKEN
        ok = allowed_reference(rel, bool(accept[q] & ACCEPT), vocab, q - base, eos)
        if not ok.any():
            gfault[s] |= FAULT_STUCK
            continue
        row = bits[r, :V]
        row[~ok & (row != NEG_INF_BITS)] = NEG_INF_BITS
    if one_row:
        bits = bits[0]
    if was_tensor:
        return torch.from_numpy(bits.view(np.int16).copy()).view(torch.bfloat16), gstate, gfault
    return bits, gstate, gfault


# ------------------------------------------------------------------------------ HIP binding
_declared = None


def _lib() -> ctypes.CDLL:
    """The kernel library (``hip.lib()``) with the grammar entry points declared."""
    global _declared
    from . import hip
    L = hip.lib()
    if _declared is not L:
        vp, i, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
        if not hasattr(L, "lsa_grammar_mask"):
            raise RuntimeError("the kernel library has no lsa_grammar_mask: rebuild it (python csrc/build.py)")
        L.lsa_grammar_mask.argtypes = [vp, ll, i, i, vp, i, vp, vp, vp, i, vp, vp, ll, vp, vp, vp, vp, vp]
        L.lsa_grammar_mask.restype = i
        L.lsa_grammar_mask_alt.argtypes = L.lsa_grammar_mask.argtypes
        L.lsa_grammar_mask_alt.restype = i
        for name, res in (("lsa_grammar_mask_calls", ll), ("lsa_grammar_mask_lds_states", i),
                          ("lsa_grammar_mask_alt_lds_states", i),
                          ("lsa_grammar_mask_threads", i), ("lsa_grammar_mask_max_v", i)):
            getattr(L, name).argtypes = []
            getattr(L, name).restype = res
        _declared = L
    return L


def grammar_mask_calls() -> int:
    """How often this process has enqueued ``lsa_grammar_mask`` (a captured graph counts at capture)."""
    return int(_lib().lsa_grammar_mask_calls())


def lds_states(alt: bool = False) -> int:
    """``LDS_STATES``: automata of up to this many states are walked from LDS, larger ones from
    global memory. ``alt``: the threshold of the entry ``lsa_grammar_mask_alt``."""
    L = _lib()
    return int(L.lsa_grammar_mask_alt_lds_states() if alt else L.lsa_grammar_mask_lds_states())


def block_threads() -> int:
    """Threads of the kernel's one workgroup per row."""
    return int(_lib().lsa_grammar_mask_threads())


def max_vocab() -> int:
    """The largest ``V`` the kernel takes (the allow bits of a row stay in registers)."""
    return int(_lib().lsa_grammar_mask_max_v())


def grammar_mask(logits: torch.Tensor, V: int, rows: int, slot: torch.Tensor, tokens_in: Optional[torch.Tensor],
                 tables, alt: bool = False) -> None:
    """``lsa_grammar_mask``: advance the grammar states of the slots ``slot`` (int32 [rows], distinct)
    by ``tokens_in`` (int32 [rows] or None) and mask the first ``rows`` rows of bf16 ``logits``
    [>= rows, ld >= V] in place; ``tables``: an object with the attributes :data:`TABLES` as cuda
    tensors. No host reads: graph-capturable. ``alt`` (measurement and tests): the entry
    ``lsa_grammar_mask_alt``, the same kernel with the other LDS threshold (``lds_states(alt=True)``)
    - the same bits."""
    from .hip import _check, _p, _req, _stream
    from .sampling import _chk
    _req(logits.is_cuda and logits.dtype == torch.bfloat16 and logits.dim() == 2 and logits.stride(1) == 1,
         "grammar_mask: logits must be a row-major bf16 cuda matrix")
    _req(1 <= rows <= logits.shape[0] and 1 <= V <= logits.shape[1] and rows <= 32768,
         f"grammar_mask: rows={rows}, V={V} outside logits {tuple(logits.shape)} (at most 32768 rows)")
    _req(rows == 1 or logits.stride(0) >= V, "grammar_mask: row stride below V")
    _req(all(getattr(tables, k, None) is not None for k in TABLES), "grammar_mask: a table is missing")
    arena, accept, data = tables.arena, tables.accept, tables.data
    _req(arena.is_cuda and arena.dtype == torch.int16 and arena.dim() == 2 and arena.shape[1] == 256
         and arena.is_contiguous() and arena.device == logits.device and arena.shape[0] >= 1,
         "grammar_mask: the arena must be a contiguous int16 cuda table [dfa_rows, 256] on the logits' device")
    _chk(accept, torch.uint8, arena.shape[0], "accept")
    _chk(tables.offsets, torch.int32, V + 1, "offsets")
    _req(data.is_cuda and data.dtype == torch.uint8 and data.dim() == 1 and data.is_contiguous()
         and data.numel() % 4 == 0 and data.numel() >= 4, "grammar_mask: data must be contiguous uint8, a multiple of 4 bytes")
    n_slots = tables.gstate.numel()
    _req(n_slots >= 1, "grammar_mask: empty slot tables")
    _chk(slot, torch.int32, rows, "slot")
    if tokens_in is not None:
        _chk(tokens_in, torch.int32, rows, "tokens_in")
    for k in ("gstate", "gbase", "gfault"):
        _chk(getattr(tables, k), torch.int32, n_slots, k)
    _chk(tables.eos, torch.int32, N_EOS, "eos")
    ld = logits.stride(0) if rows > 1 else max(logits.stride(0), V)
    L = _lib()
    rc = (L.lsa_grammar_mask_alt if alt else L.lsa_grammar_mask)(_p(logits), ld, V, rows, _p(slot), n_slots, _p(tokens_in), _p(arena), _p(accept),
        arena.shape[0], _p(tables.offsets), _p(data), data.numel(), _p(tables.gstate),
        _p(tables.gbase), _p(tables.gfault), _p(tables.eos), _stream())
    _check(rc, "lsa_grammar_mask")


__all__ = ["TABLES", "ACCEPT", "LAST", "FAULT_TOKEN", "FAULT_STUCK", "FAULT_STATE", "ByteDFA", "VocabBytes",
           "pieces_to_bytes", "detect_kind", "allowed_reference", "grammar_mask_reference", "grammar_mask",
           "grammar_mask_calls", "lds_states", "block_threads", "max_vocab"]
