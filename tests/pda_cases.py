"""Shared builders of the JSON-mode tests (tests/test_pda.py, tests/test_pda_gpu.py): the independent
oracle of the JSON language, a seeded corpus, small general pushdown automata, deterministic kernel
cases - bf16 logits as bit patterns, a slot table that holds regex rows and JSON rows - and their
reference results, computed once."""
import functools
import json
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np

import grammar_cases as GC
from llm_sharding_amd.ops import grammar as G
from llm_sharding_amd.ops import pda as J

EOS = GC.EOS
WS = b" \t\n\r"
ALL_TABLES = tuple(dict.fromkeys(G.TABLES + J.TABLES))
STATE_WORDS = ("gstate", "jstate", "jdepth", "jstack", "gfault")


# ------------------------------------------------------------------------------ the oracle
def _raise(x):
    raise ValueError(x)


def ok(data: bytes, max_ws: int = 2) -> bool:
    """The language of ``BytePDA.json(max_ws=max_ws)`` by other means: UTF-8, ``json.loads``, a dict
    on top, whitespace runs outside strings of at most ``max_ws`` bytes, nesting of at most 64."""
    try:
        value = json.loads(data.decode("utf-8"), parse_constant=_raise)
    except (ValueError, RecursionError):
        return False
    if not isinstance(value, dict):
        return False
    run = depth = 0
    in_str = esc = False
    for b in data:
        if in_str:
            if esc:
                esc = False
            elif b == 0x5C:
                esc = True
            elif b == 0x22:
                in_str = False
            continue
        if b in WS:
            run += 1
            if run > max_ws:
                return False
            continue
        run = 0
        if b == 0x22:
            in_str = True
        elif b in b"{[":
            depth += 1
            if depth > J.MAX_DEPTH:
                return False
        elif b in b"}]":
            depth -= 1
    return True


def outside_strings(data: bytes) -> list:
    """The positions ``i`` of a well-formed text at which whitespace may be inserted before byte
    ``i``: next to a structural byte, outside strings."""
    out, in_str, esc = [], False, False
    for i, b in enumerate(data):
        if in_str:
            if esc:
                esc = False
            elif b == 0x5C:
                esc = True
            elif b == 0x22:
                in_str = False
                out.append(i + 1)
            continue
        if b == 0x22:
            in_str = True
            out.append(i)
        elif b in b"{}[],:":
            out += [i, i + 1]
    return sorted(set(out))


_CHARS = ["a", "b", "Z", "0", " ", '"', "\\", "/", "\n", "\t", "\x01", "\x7f", "\u00e9", "\u20ac", "\u2028", "\ud7ff",
          "\ue000", "\U0001F600", "\U0010FFFF", "{", "]", ","]


def _rand_string(rng) -> str:
    return "".join(_CHARS[int(i)] for i in rng.integers(0, len(_CHARS), int(rng.integers(0, 6))))


def _rand_value(rng, depth: int):
    k = int(rng.integers(0, 10 if depth < 4 else 7))
    if k == 0:
        return [None, True, False][int(rng.integers(0, 3))]
    if k == 1:
        return int(rng.integers(-1000, 1000)) * int(rng.integers(0, 2) * 10 ** int(rng.integers(0, 12)) + 1)
    if k == 2:
        return float(rng.standard_normal()) * 10.0 ** int(rng.integers(-20, 20))
    if k == 3:
        return [0, -0.0, 1e300, 5e-324, 0.5, 1e16, float("inf"), float("nan")][int(rng.integers(0, 8))]
    if k <= 6:
        return _rand_string(rng)
    if k == 7:
        return [_rand_value(rng, depth + 1) for _ in range(int(rng.integers(0, 4)))]
    return {_rand_string(rng): _rand_value(rng, depth + 1) for _ in range(int(rng.integers(0, 4)))}


_SEPARATORS = [(",", ":"), (", ", ": "), (" , ", " : "), (",\n", ":\t"), (",  ", ": "), (",\r\n", ":  "), (",   ", ":")]


def corpus(seed: int, max_ws: int = 2, n: int = 260) -> list:
    """Texts of at most 200 bytes: ``json.dumps`` of random values under several separators and both
    ``ensure_ascii``, each once more with hand-inserted whitespace runs of ``max_ws`` and
    ``max_ws + 1`` bytes, and byte-level mutations of all of those."""
    rng = np.random.default_rng(seed)
    base = []
    while len(base) < n:
        top = _rand_value(rng, 0) if rng.integers(0, 6) == 0 else \
            {_rand_string(rng): _rand_value(rng, 1) for _ in range(int(rng.integers(0, 4)))}
        sep = _SEPARATORS[int(rng.integers(0, len(_SEPARATORS)))]
        text = json.dumps(top, separators=sep, indent=None, ensure_ascii=bool(rng.integers(0, 2)))
        data = text.encode("utf-8")
        if len(data) <= 200:
            base.append(data)
    spaced = []
    for data in base:
        spots = outside_strings(data)
        for run in (max_ws, max_ws + 1):
            if spots and run:
                i = spots[int(rng.integers(0, len(spots)))]
                ws = bytes(WS[int(j)] for j in rng.integers(0, 4, run))
                if i > 0 and data[i - 1] in WS or i < len(data) and data[i] in WS:
                    continue                          # would join an existing run
                spaced.append(data[:i] + ws + data[i:])
    out = base + [d for d in spaced if len(d) <= 200]
    pool = b'{}[]",:\\u0019eE.-+ \n\x00\x1f\x7f\x80\xbf\xc0\xc2\xe0\xed\xa0\xf0\xf4\x90\xffatn'
    for data in list(out):
        if not data:
            continue
        for _ in range(3):
            kind, i = int(rng.integers(0, 4)), int(rng.integers(0, len(data)))
            b = bytes([pool[int(rng.integers(0, len(pool)))]])
            if kind == 0:
                m = data[:i] + (bytes([data[i] ^ (1 << int(rng.integers(0, 8)))]) if rng.integers(0, 2) else b) + data[i + 1:]
            elif kind == 1:
                m = data[:i] + data[i + 1:]
            elif kind == 2:
                m = data[:i] + b + data[i:]
            else:
                m = data[:i]
            if len(m) <= 200:
                out.append(m)
    return out


# ------------------------------------------------------------------------------ automata
def bracket_pda() -> J.BytePDA:
    """Two states: balanced ``( )`` / ``[ ]`` in state 0; ``x`` on an empty stack leads to state 1,
    which accepts and reads nothing."""
    nxt = np.full((3, 2, 256), -1, dtype=np.int16)
    nxt[:, 0, ord("(")] = 0 | J.OP_PUSH0 << 10
    nxt[:, 0, ord("[")] = 0 | J.OP_PUSH1 << 10
    nxt[J.TOP0, 0, ord(")")] = 0 | J.OP_POP << 10
    nxt[J.TOP1, 0, ord("]")] = 0 | J.OP_POP << 10
    nxt[J.EMPTY, 0, ord("x")] = 1
    return J.BytePDA(nxt, [0, 1])


@functools.lru_cache(maxsize=None)
def general_pda(S: int) -> J.BytePDA:
    """``S`` states over ``a b c d ( ) [ ]``: ``a`` and ``b`` move the state, brackets push and pop
    and move it, ``c`` lives only inside ``[``, ``d`` only on an empty stack."""
    q = np.arange(S)
    nxt = np.full((3, S, 256), -1, dtype=np.int32)
    nxt[:, q, ord("a")] = (q + 1) % S
    nxt[:, q, ord("b")] = (2 * q + 1) % S
    nxt[:, q, ord("(")] = q | J.OP_PUSH0 << 10
    nxt[:, q, ord("[")] = ((q + 1) % S) | J.OP_PUSH1 << 10
    nxt[J.TOP0, q, ord(")")] = q | J.OP_POP << 10
    nxt[J.TOP1, q, ord("]")] = ((q + 3) % S) | J.OP_POP << 10
    nxt[J.TOP1, q, ord("c")] = (q + 5) % S
    nxt[J.EMPTY, q, ord("d")] = (S - 1 - q)
    return J.BytePDA(nxt.astype(np.int16), (q % 3 == 0).astype(np.uint8))


# ------------------------------------------------------------------------------ vocabularies
SPECIAL_TOKENS = (b'{"a":[[', b"]]}", b"}}]")


def json_vocab(rng, V: int, max_len: int, long_tail=()) -> G.VocabBytes:
    """0..2 special; the 256 single bytes; :data:`SPECIAL_TOKENS`; then strings of 0 to ``max_len``
    bytes: a third random over a JSON-ish alphabet, the rest slices of well-formed texts.
    ``long_tail``: the extra-long tokens placed at the end."""
    pieces = [b""] * 3 + [bytes([b]) for b in range(256)] + list(SPECIAL_TOKENS)
    alpha = np.frombuffer(b'{}[]",:0123456789.eE-+ \ntrufalsn\\\xc3\xa9', dtype=np.uint8)
    texts = [t for t in corpus(11, n=60)[:60] if len(t) > 4]
    while len(pieces) < V - len(long_tail):
        n = int(rng.integers(0, max_len + 1))
        if rng.integers(0, 3) == 0:
            pieces.append(rng.choice(alpha, n).astype(np.uint8).tobytes())
        else:
            t = texts[int(rng.integers(0, len(texts)))]
            i = int(rng.integers(0, len(t)))
            pieces.append(t[i:i + n])
    return G.VocabBytes.from_pieces(pieces[:V - len(long_tail)] + list(long_tail))


def bracket_vocab(rng, V: int, max_len: int) -> G.VocabBytes:
    pieces = [b""] * 3 + [bytes([b]) for b in b"ab()[]cdx"]
    alpha = np.frombuffer(b"ab()[]cdab()[]x", dtype=np.uint8)
    while len(pieces) < V:
        pieces.append(rng.choice(alpha, int(rng.integers(0, max_len + 1))).astype(np.uint8).tobytes())
    return G.VocabBytes.from_pieces(pieces)


# ------------------------------------------------------------------------------ kernel cases
def tables(pda: J.BytePDA, vocab: G.VocabBytes, n_slots: int, arena: GC.Arena = None, eos=EOS) -> SimpleNamespace:
    """The numpy tables of both kernels of the stage: the regex's and the automaton's."""
    ar = GC.Arena(4) if arena is None else arena
    tb = GC.tables(ar, vocab, n_slots, eos)
    tb.ptab, tb.paccept = np.array(pda.next), np.array(pda.accept)
    tb.jstate = np.full(n_slots, -1, dtype=np.int32)
    tb.jdepth = np.zeros(n_slots, dtype=np.int32)
    tb.jstack = np.zeros(n_slots, dtype=np.int64)
    return tb


def put(tb: SimpleNamespace, s: int, config) -> None:
    tb.jstate[s], tb.jdepth[s] = config[0], config[1]
    tb.jstack[s] = np.uint64(config[2]).astype(np.int64)


@dataclass(frozen=True)
class Case:
    V: int
    logits: np.ndarray     # uint16 [rows, ld]
    slot: np.ndarray       # int32 [rows]
    tokens: np.ndarray     # int32 [rows], -1 = none
    tables: SimpleNamespace
    modes: tuple
    vocab: G.VocabBytes
    pda: J.BytePDA


def reference(c: Case, tokens="own"):
    """What a stage step computes: ``grammar_mask_reference``, then ``pda_mask_reference`` on its
    logits and fault flags -> ``(logits, gstate, jstate, jdepth, jstack, gfault)``."""
    tok = c.tokens if isinstance(tokens, str) else tokens
    lg, gstate, gfault = G.grammar_mask_reference(c.logits, c.V, c.tables, c.slot, tok)
    tb = SimpleNamespace(**vars(c.tables))
    tb.gfault = gfault
    lg, jstate, jdepth, jstack, gfault = J.pda_mask_reference(lg, c.V, tb, c.slot, tok)
    return lg, gstate, jstate, jdepth, jstack, gfault


_REFS: dict = {}


def cached_reference(name: str, c: Case):
    if name not in _REFS:
        _REFS[name] = reference(c)
    return _REFS[name]


def deep(n: int) -> bytes:
    """A live prefix at depth ``n``: the top-level object and ``n - 1`` arrays."""
    return b'{"a":' + b"[" * (n - 1)


@functools.lru_cache(maxsize=None)
def small_case() -> Case:
    """1 row, V = 1003 (not a multiple of 8), token lengths 0 to 20, JSON inside an array."""
    rng = np.random.default_rng(21)
    pda, V = J.BytePDA.json(), 1003
    vocab = json_vocab(rng, V, 20)
    tb = tables(pda, vocab, 2)
    put(tb, 1, pda.walk(b'{"k":[1'))
    return Case(V, GC.random_logits(rng, 1, V, V + 13), np.array([1], dtype=np.int32),
                np.array([GC.token_of(vocab, b",")], dtype=np.int32), tb, ("step",), vocab, pda)


MODES = ("off", "regex", "d0", "in_string", "after_top0", "after_top1", "d63", "d64", "accept", "nonaccept",
         "forbidden_in", "step_push", "step_pop", "eos_in", "beyond_v_in", "empty_in", "neg_in")


@functools.lru_cache(maxsize=None)
def mixed_case() -> Case:
    """129 rows over a permuted 160-slot table, V = 4099, one mode per row; the regex rows belong to
    lsa_grammar_mask."""
    rng = np.random.default_rng(22)
    rows, V, n_slots = 129, 4099, 160
    pda = J.BytePDA.json()
    vocab = json_vocab(rng, V, 12)
    ar = GC.Arena(16)
    tight = GC.dfa(GC.TIGHT)
    bt = ar.place(tight, 3)
    tb = tables(pda, vocab, n_slots, ar)
    slot = rng.permutation(n_slots)[:rows].astype(np.int32)
    tokens = np.full(rows, -1, dtype=np.int32)
    tok = lambda piece: GC.token_of(vocab, piece)  # noqa: E731
    modes = tuple(MODES[r % len(MODES)] for r in range(rows))
    start = {"d0": b"", "in_string": b'{"a":"x', "after_top0": b'{"a":"x"', "after_top1": b'{"a":["x"',
             "d63": deep(63), "d64": deep(64), "accept": b'{"a":1}', "nonaccept": b'{"a"', "forbidden_in": b"",
             "step_push": b"", "step_pop": b'{"b":[[7', "eos_in": b"{}", "beyond_v_in": b"{", "empty_in": b"{", "neg_in": b"{"}
    feed = {"forbidden_in": tok(b"}}]"), "step_push": tok(b'{"a":[['), "step_pop": tok(b"]]}"), "eos_in": EOS[0],
            "beyond_v_in": V + 5, "empty_in": 0, "neg_in": -7, "off": tok(b"7"), "regex": tok(b"7")}
    for r, m in enumerate(modes):
        s = slot[r]
        tokens[r] = feed.get(m, -1)
        if m == "regex":
            tb.gbase[s], tb.gstate[s] = bt, bt
        elif m != "off":
            put(tb, s, pda.walk(start[m]))
    return Case(V, GC.random_logits(rng, rows, V, V + 4), slot, tokens, tb, modes, vocab, pda)


@functools.lru_cache(maxsize=None)
def general_case(S: int) -> Case:
    """An automaton of ``S`` states (2: the bracket automaton) from five configurations: the start,
    a deep stack with a token fed, depth 64, a state near the end, an empty stack in an accepting
    state."""
    rng = np.random.default_rng(23)
    V = 1500
    pda = bracket_pda() if S == 2 else general_pda(S)
    vocab = bracket_vocab(rng, V, 9)
    tb = tables(pda, vocab, 8)
    tok = lambda piece: GC.token_of(vocab, piece)  # noqa: E731
    if S == 2:
        configs = [(0, 0, 0), (0, 3, 0b101), (0, 64, (1 << 64) - 1 - 2), (0, 1, 1), (1, 0, 0)]
    else:
        configs = [(0, 0, 0), (S // 2, 3, 0b101), (S - 1, 64, (1 << 64) - 1 - 2), (S - 2, 1, 1), (3 * ((S - 1) // 3), 0, 0)]
    tokens = [-1, tok(b"]"), tok(b"]"), tok(b"["), -1]
    for s, cf in enumerate(configs):
        put(tb, s, cf)
    return Case(V, GC.random_logits(rng, 5, V, V + 3), np.arange(5, dtype=np.int32), np.array(tokens, dtype=np.int32),
                tb, ("general",) * 5, vocab, pda)


LONG = (b',[[[{"k":[[]]}]]]' * 20)[:300]


@functools.lru_cache(maxsize=None)
def wide_case() -> Case:
    """V = 128256 with 2 rows and tokens of 300 bytes that push and pop many times."""
    rng = np.random.default_rng(24)
    V = 128256
    pda = J.BytePDA.json()
    tail = (LONG, LONG[:299], (b',{"q":[[{}]]}' * 20)[:257], LONG[:150], b"x" * 64, LONG[:33])
    vocab = json_vocab(rng, V, 10, long_tail=tail)
    tb = tables(pda, vocab, 3)
    put(tb, 2, pda.walk(b'{"a":[1'))
    put(tb, 0, pda.walk(b'{"a":[1'))
    return Case(V, GC.random_logits(rng, 2, V, V + 1), np.array([2, 0], dtype=np.int32),
                np.array([V - 6, GC.token_of(vocab, b"7")], dtype=np.int32), tb, ("long_in", "number"), vocab, pda)
