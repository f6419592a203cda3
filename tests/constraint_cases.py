"""Shared builders of the constrained-decoding tests (tests/test_constraints.py,
tests/test_constraints_gpu.py): deterministic kernel cases - bf16 logits as bit patterns, an arena
with automata at non-zero bases, per-slot tables with a different mode per row - and their
reference results, computed once."""
import functools
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np
import torch

from llm_sharding_amd.ops import constraints as K
from llm_sharding_amd.ops.penalties import bf16_rne_bits

LOGIT_PAD = 0x42C8   # bf16 100.0: the sentinel of logits columns [V, ld)
ARENA_PAD = 0x1234   # the sentinel of arena columns [V, ld_arena) and of rows no automaton owns
NINF = float("-inf")

# what a row's slot asks for, cycled over the rows
MODES = ("off", "bias", "bias_all", "auto", "auto_minp", "eos_on", "eos_off", "minp_zero", "minp_max_only",
         "auto_fault", "bias_auto_minp", "eos_bias", "auto_no_token", "minp")

# (rows, V, ld, n_slots): an odd ld (rows start unaligned, except row 0), an aligned ld with a
# V % 8 tail, more rows than slots are skipped at the Llama-2 vocabulary, one row of Llama-3's
KERNEL_CASES = ((3, 1003, 1008 + 5, 5), (14, 1003, 1008, 20), (129, 32000, 32000, 160), (1, 128256, 128256, 3))


@dataclass(frozen=True)
class Case:
    rows: int
    V: int
    ld: int
    logits: np.ndarray     # uint16 [rows, ld] bf16 bit patterns
    slot: np.ndarray       # int32 [rows], distinct, not the identity
    tokens: np.ndarray     # int32 [rows], -1 = none
    ctr: np.ndarray        # int32 [rows]
    ctr_add: int
    tables: SimpleNamespace  # numpy arrays named as ops.constraints.TABLES
    modes: tuple           # per row


def bf16_bits(a) -> np.ndarray:
    return bf16_rne_bits(np.asarray(a, dtype=np.float32))


def random_automaton(rng, S: int, V: int, p_allow: float = 0.4) -> np.ndarray:
    """int16 [S, V]: each entry forbidden with probability 1 - p_allow, else a random state; every
    state allows at least one token, and columns 0, V - 1 and the tail are mixed."""
    t = rng.integers(0, S, (S, V)).astype(np.int16)
    t[rng.random((S, V)) >= p_allow] = -1
    for s in range(S):
        t[s, (7 * s + 3) % V] = (s + 1) % S
        t[s, 0] = -1 if s % 2 else s
        t[s, V - 1] = s if s % 2 else -1
    return t


def tail_col(V: int) -> int:
    return (V & ~7) + (V % 8) // 2 if V % 8 else V - 8


def empty_tables(n_slots: int, state_rows: int, ld_arena: int, eos=()) -> SimpleNamespace:
    eos = list(eos)
    return SimpleNamespace(
        arena=np.full((state_rows, ld_arena), ARENA_PAD, dtype=np.int16),
        astate=np.full(n_slots, -1, dtype=np.int32), abase=np.zeros(n_slots, dtype=np.int32),
        bias_n=np.zeros(n_slots, dtype=np.int32), bias_tok=np.zeros((n_slots, K.BIAS_MAX), dtype=np.int32),
        bias_val=np.zeros((n_slots, K.BIAS_MAX), dtype=np.float32), min_until=np.zeros(n_slots, dtype=np.int32),
        minp_delta=np.full(n_slots, NINF, dtype=np.float32), fault=np.zeros(n_slots, dtype=np.int32),
        eos=np.array(eos + [-1] * (K.N_EOS - len(eos)), dtype=np.int32))


def set_bias(tb, s: int, toks, vals) -> None:
    n = len(toks)
    tb.bias_n[s] = n
    tb.bias_tok[s, :n] = toks
    tb.bias_val[s, :n] = vals


@functools.lru_cache(maxsize=None)
def make_case(rows: int, V: int, ld: int, n_slots: int) -> Case:
    rng = np.random.default_rng(77 * rows + V + ld)
    logits = np.full((rows, ld), LOGIT_PAD, dtype=np.uint16)
    logits[:, :V] = bf16_bits(4.0 * rng.standard_normal((rows, V)))
    # two automata, the first at base 3 (rows 0..2 belong to nobody), the second right behind it
    SA, SB = 5, 3
    state_rows, ld_arena = 3 + SA + SB + 2, ld       # an odd ld: arena rows start unaligned too
    tb = empty_tables(n_slots, state_rows, ld_arena, eos=(2, V - 1, tail_col(V)))
    autos = ((3, random_automaton(rng, SA, V)), (3 + SA, random_automaton(rng, SB, V, 0.05)))
    for base, t in autos:
        tb.arena[base:base + t.shape[0], :V] = t
    if rows == 1:
        slot = np.array([n_slots - 2], dtype=np.int32)
    elif rows < 8:
        slot = np.concatenate([[0], 1 + rng.permutation(n_slots - 1)[:rows - 1]]).astype(np.int32)
    else:
        slot = rng.permutation(n_slots)[:rows].astype(np.int32)
        assert (slot != np.arange(rows)).any()
    ctr_add = 1
    ctr = rng.integers(5, 900, rows).astype(np.int32)
    tokens = np.full(rows, -1, dtype=np.int32)
    modes = tuple(MODES[(r + (10 if rows == 1 else 1 if rows < 8 else 0)) % len(MODES)] for r in range(rows))
    few = [0, V - 1, tail_col(V), 8 * 37 + 3, 2]
    few_val = [1.5, -2.25, NINF, 0.375, 7.0]
    for r, mode in enumerate(modes):
        s, c = int(slot[r]), int(ctr[r]) + ctr_add
        if "auto" in mode:
            base, t = autos[r % 2]
            rel = int(rng.integers(0, t.shape[0]))
            tb.abase[s], tb.astate[s] = base, base + rel
            ok = np.nonzero(t[rel] >= 0)[0]
            bad = np.nonzero(t[rel] < 0)[0]
            tokens[r] = -1 if mode == "auto_no_token" else int(bad[r % bad.size] if mode == "auto_fault" else
                                                               ok[r % ok.size])
        elif r % 3 == 0:
            tokens[r] = int(rng.integers(0, V))       # a token without an automaton changes nothing
        if mode in ("bias", "bias_auto_minp", "eos_bias"):
            set_bias(tb, s, few, few_val)
        if mode == "bias_all":
            toks = np.concatenate([few[:2], [tail_col(V)], 3 + rng.permutation(V - 12)[:K.BIAS_MAX - 3]])
            vals = (3.0 * rng.standard_normal(K.BIAS_MAX)).astype(np.float32)
            vals[5::7] = NINF
            set_bias(tb, s, toks, vals)
        if mode in ("eos_on", "eos_bias"):
            tb.min_until[s] = c + 1                   # c is the last masked position
        if mode == "eos_off":
            tb.min_until[s] = c                       # c is the first free position: the row is skipped
        if mode in ("auto_minp", "bias_auto_minp", "minp"):
            tb.minp_delta[s] = np.float32(0.8 * np.log(0.1))
        if mode == "minp_zero":
            tb.minp_delta[s] = 0.0
            logits[r, [5, V - 2]] = bf16_bits([30.0])[0]   # a tie at the top: both survive
        if mode == "minp_max_only":
            tb.minp_delta[s] = -1e-6
    # slots no row names keep a live configuration that must not be touched
    for s in np.setdiff1d(np.arange(n_slots), slot)[:2]:
        tb.abase[s], tb.astate[s] = 3, 4
        set_bias(tb, int(s), few, few_val)
    return Case(rows, V, ld, logits, slot, tokens, ctr, ctr_add, tb, modes)


@functools.lru_cache(maxsize=None)
def reference(rows: int, V: int, ld: int, n_slots: int):
    """(logits uint16 [rows, ld], astate int32 [n_slots], fault int32 [n_slots]) after one launch."""
    c = make_case(rows, V, ld, n_slots)
    return K.logit_process_reference(c.logits, V, c.tables, c.slot, c.tokens, c.ctr, c.ctr_add)


def chain_automaton(S: int = K.MAX_STATES, V: int = 64) -> np.ndarray:
    """State i allows only token i % V and leads to i + 1; the last state loops on token 0."""
    t = np.full((S, V), -1, dtype=np.int16)
    i = np.arange(S - 1)
    t[i, i % V] = i + 1
    t[S - 1, 0] = S - 1
    return t


def to_bf16(bits: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16).copy()).view(torch.bfloat16)
