"""Shared builders of the regex-constrained decoding tests (tests/test_grammar.py,
tests/test_grammar_gpu.py): a hand-built vocabulary for the tiny model, deterministic kernel cases
- bf16 logits as bit patterns, a DFA arena with automata at non-zero bases, a permuted slot table
with a different mode per row - and their reference results, computed once."""
import functools
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np

from llm_sharding_amd.ops import grammar as G
from llm_sharding_amd.ops.penalties import bf16_rne_bits

LOGIT_PAD = 0x42C8   # bf16 100.0: the sentinel of logits columns [V, ld)
NINF_BITS = 0xFF80
NAN_BITS = 0x7FC1
EOS = (2,)

TIGHT, PERMISSIVE, BIG = r"-?[0-9]{1,6}", r"[ -~]*", r"[ab]{0,1999}"

# what a row asks for, cycled over the rows of the 129-row case
MODES = ("off", "tight", "tight_step", "permissive", "accept_eos", "nonaccept_eos", "forbidden_in", "empty_in",
         "eos_in", "neg_in", "stuck", "big_step", "beyond_v_in", "based")


def tiny_pieces(V: int = 512) -> list:
    """The tiny model's vocabulary: 0..2 special, 3..258 the single bytes (as the synthetic byte
    tokenizer has them), then multi-byte strings, the rest unknown (empty)."""
    multi = [b"yes", b"no", b"ye", b"es", b"12", b"00", b"-1", b".5", b".25", b"ab", b"abc", b"bcx", b"cx", b"aa",
             b"ccx", b"999", b"1.0", b"0.00", b"-12.50", b"abcab", b"bx", b"yesno", b"7.", b".", b"acx", b"\xc3\xa9"]
    pieces = [b""] * 3 + [bytes([b]) for b in range(256)] + multi
    assert len(pieces) <= V
    return pieces + [b""] * (V - len(pieces))


def sample_walk(dfa: G.ByteDFA, rng, n: int, state: int = 0) -> bytes:
    """A string of up to ``n`` bytes that stays alive in ``dfa`` from ``state``."""
    out = []
    for _ in range(n):
        live = np.nonzero(dfa.next[state] >= 0)[0]
        if not live.size:
            break
        b = int(rng.choice(live))
        out.append(b)
        state = int(dfa.next[state, b])
    return bytes(out)


def random_vocab(rng, V: int, max_len: int, alphabet: bytes, dfas=(), singles: int = 256, long_tail=()) -> G.VocabBytes:
    """0..2 special; the first ``singles`` byte values as one-byte tokens; then strings of 0 to
    ``max_len`` bytes: a third random over ``alphabet``, the rest live walks of ``dfas``.
    ``long_tail``: lengths of a few extra-long tokens placed at the end."""
    pieces = [b""] * 3 + [bytes([b]) for b in range(singles)]
    alpha = np.frombuffer(alphabet, dtype=np.uint8)
    while len(pieces) < V - len(long_tail):
        n = int(rng.integers(0, max_len + 1))
        k = int(rng.integers(0, 3))
        if k == 0 or not dfas:
            pieces.append(rng.choice(alpha, n).astype(np.uint8).tobytes())
        else:
            d = dfas[int(rng.integers(0, len(dfas)))]
            pieces.append(sample_walk(d, rng, n, int(rng.integers(0, min(d.n_states, 4)))))
    for n in long_tail:
        pieces.append(sample_walk(dfas[-1], rng, n))
    return G.VocabBytes.from_pieces(pieces[:V])


class Arena:
    """A numpy DFA arena: ``place(dfa, base)`` writes the rows and the accept flags."""

    def __init__(self, dfa_rows: int):
        self.arena = np.full((dfa_rows, 256), -1, dtype=np.int16)
        self.accept = np.zeros(dfa_rows, dtype=np.uint8)

    def place(self, dfa: G.ByteDFA, base: int) -> int:
        S = dfa.n_states
        assert base + S <= self.arena.shape[0] and (self.arena[base:base + S] == -1).all()
        self.arena[base:base + S] = dfa.next
        self.accept[base:base + S] = dfa.accept.astype(np.uint8) * G.ACCEPT
        self.accept[base + S - 1] |= G.LAST
        return base


def tables(ar: Arena, vocab: G.VocabBytes, n_slots: int, eos=EOS) -> SimpleNamespace:
    return SimpleNamespace(arena=ar.arena, accept=ar.accept, offsets=np.array(vocab.offsets), data=np.array(vocab.data),
                           gstate=np.full(n_slots, -1, dtype=np.int32), gbase=np.zeros(n_slots, dtype=np.int32),
                           gfault=np.zeros(n_slots, dtype=np.int32),
                           eos=np.array(list(eos) + [-1] * (8 - len(eos)), dtype=np.int32))


def random_logits(rng, rows: int, V: int, ld: int) -> np.ndarray:
    """bf16 bit patterns with a few -inf and NaN already in place, the sentinel beyond V."""
    x = np.full((rows, ld), LOGIT_PAD, dtype=np.uint16)
    x[:, :V] = bf16_rne_bits((4.0 * rng.standard_normal((rows, V))).astype(np.float32))
    for r in range(rows):
        x[r, rng.integers(0, V, 5)] = NINF_BITS
        x[r, rng.integers(0, V, 3)] = NAN_BITS
    return x


@dataclass(frozen=True)
class Case:
    V: int
    logits: np.ndarray     # uint16 [rows, ld]
    slot: np.ndarray       # int32 [rows]
    tokens: np.ndarray     # int32 [rows], -1 = none
    tables: SimpleNamespace
    modes: tuple
    vocab: G.VocabBytes


@functools.lru_cache(maxsize=None)
def dfa(pattern: str) -> G.ByteDFA:
    return G.ByteDFA.from_regex(pattern)


def stuck_dfa() -> G.ByteDFA:
    """State 0 moves on byte 0xFE only, which no token of the test vocabularies starts with."""
    nxt = np.full((2, 256), -1, dtype=np.int16)
    nxt[0, 0xFE] = 1
    return G.ByteDFA(nxt, [False, True])


def token_of(vocab: G.VocabBytes, piece: bytes) -> int:
    for v in range(vocab.V):
        if vocab.token(v) == piece:
            return v
    raise KeyError(piece)


@functools.lru_cache(maxsize=None)
def small_case() -> Case:
    """1 row, V = 1000, token lengths 0 to 20, a 3-state DFA (the test offsets the row base)."""
    rng = np.random.default_rng(1)
    d = dfa(r"([a-m][n-z])*[0-9]?")
    assert d.n_states == 3
    vocab = random_vocab(rng, 1000, 20, b"agnz05", dfas=(d,))
    ar = Arena(8)
    tb = tables(ar, vocab, 2)
    tb.gstate[1] = tb.gbase[1] = ar.place(d, 2)
    return Case(1000, random_logits(rng, 1, 1000, 1000 + 13), np.array([1], dtype=np.int32),
                np.array([token_of(vocab, b"a")], dtype=np.int32), tb, ("tight_step",), vocab)


@functools.lru_cache(maxsize=None)
def mixed_case() -> Case:
    """129 rows over a permuted 160-slot table, V = 4099, one mode per row."""
    rng = np.random.default_rng(2)
    rows, V, n_slots = 129, 4099, 160
    t, p, big, st = dfa(TIGHT), dfa(PERMISSIVE), dfa(BIG), stuck_dfa()
    vocab = random_vocab(rng, V, 12, b"ab0123456789-. xyz", dfas=(t, big), singles=0xF0)
    ar = Arena(2100)
    bp, bt, bs, bb = ar.place(p, 0), ar.place(t, 5), ar.place(st, 30), ar.place(big, 40)
    tb = tables(ar, vocab, n_slots)
    slot = rng.permutation(n_slots)[:rows].astype(np.int32)
    tokens = np.full(rows, -1, dtype=np.int32)
    digit, minus, ab = token_of(vocab, b"7"), token_of(vocab, b"-"), token_of(vocab, b"ab")
    modes = tuple(MODES[r % len(MODES)] for r in range(rows))
    for r, m in enumerate(modes):
        s = slot[r]
        if m == "off":
            tokens[r] = digit
            continue
        base, q, tin = bt, 0, -1
        if m == "tight_step":
            tin = (minus, digit)[r % 2]
        elif m == "permissive":
            base, tin = bp, ab
        elif m == "accept_eos":
            q = t.walk(b"12")
        elif m == "forbidden_in":
            q, tin = t.walk(b"1"), ab
        elif m == "empty_in":
            tin = 0
        elif m == "eos_in":
            q, tin = t.walk(b"123456"), EOS[0]
        elif m == "stuck":
            base = bs
        elif m == "big_step":
            base, q, tin = bb, int(rng.integers(0, 1990)), ab
        elif m == "beyond_v_in":
            tin = V + 5
        elif m == "based":
            base, q = bb, 1999
        tb.gbase[s], tb.gstate[s], tokens[r] = base, base + q, tin
    return Case(V, random_logits(rng, rows, V, V + 4), slot, tokens, tb, modes, vocab)


@functools.lru_cache(maxsize=None)
def edge_case(lds_states: int) -> Case:
    """DFAs of exactly LDS_STATES, LDS_STATES + 1 and 2000 states, each from its start state, from
    a middle state by a token, and from its last state."""
    rng = np.random.default_rng(3)
    V = 1500
    ds = [dfa(r"[ab]{0,%d}" % (lds_states - 1)), dfa(r"[ab]{0,%d}" % lds_states), dfa(BIG)]
    assert [d.n_states for d in ds] == [lds_states, lds_states + 1, 2000]
    vocab = random_vocab(rng, V, 9, b"abc", dfas=(ds[2],))
    ar = Arena(3 + 2 * lds_states + 1 + 2000 + 7)
    tb = tables(ar, vocab, 12)
    bases, b = [], 3
    for d in ds:
        bases.append(ar.place(d, b))
        b += d.n_states + 2
    slot, tokens = [], []
    ab = token_of(vocab, b"ab")
    for i, (d, base) in enumerate(zip(ds, bases)):
        for j, (q, tin) in enumerate(((0, -1), (d.n_states - 4, ab), (d.n_states - 1, -1))):
            s = 3 * i + j
            tb.gbase[s], tb.gstate[s] = base, base + q
            slot.append(s)
            tokens.append(tin)
    return Case(V, random_logits(rng, 9, V, V + 3), np.array(slot, dtype=np.int32), np.array(tokens, dtype=np.int32),
                tb, ("edge",) * 9, vocab)


@functools.lru_cache(maxsize=None)
def wide_case() -> Case:
    """V = 128256 with 2 rows and tokens of up to 300 bytes."""
    rng = np.random.default_rng(4)
    V = 128256
    p, big = dfa(PERMISSIVE), dfa(BIG)
    vocab = random_vocab(rng, V, 10, b"ab cde", dfas=(p, big), long_tail=(300, 299, 257, 150, 64, 33))
    ar = Arena(2010)
    tb = tables(ar, vocab, 3)
    tb.gstate[0] = tb.gbase[0] = ar.place(p, 0)
    tb.gbase[2] = ar.place(big, 4)
    tb.gstate[2] = tb.gbase[2] + 1600
    return Case(V, random_logits(rng, 2, V, V + 1), np.array([2, 0], dtype=np.int32),
                np.array([V - 6, token_of(vocab, b"a")], dtype=np.int32), tb, ("big", "permissive"), vocab)   # V - 6: 300 bytes


def reference(c: Case, tokens="own", rows=None):
    """``grammar_mask_reference`` on the case (``tokens=None``: no input tokens; ``rows``: a subset)."""
    tok = c.tokens if isinstance(tokens, str) else tokens
    sel = slice(None) if rows is None else rows
    return G.grammar_mask_reference(c.logits[sel], c.V, c.tables, c.slot[sel], None if tok is None else tok[sel])


_REFS: dict = {}


def cached_reference(name: str, c: Case):
    if name not in _REFS:
        _REFS[name] = reference(c)
    return _REFS[name]
