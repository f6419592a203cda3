"""Shared builders of the penalty tests (tests/test_penalties.py, tests/test_penalties_gpu.py):
deterministic kernel cases (bf16 logits as bit patterns, a sparse token-statistics table, per-row
slots / input tokens / parameters), their reference results, and a direct per-element
implementation of the contract that shares no code with ``ops.penalties``."""
import functools
from dataclasses import dataclass

import numpy as np
import torch

from llm_sharding_amd.ops import penalties as P

LOGIT_PAD = 0x42C8   # bf16 100.0: the sentinel of logits columns [V, ld)
STATE_PAD = 0xABCD   # the sentinel of state columns [V, ld_state)

# (rep, pres, freq) per row, cycled: all-off, rho > 1, rho < 1, alpha only, beta only, all three,
# negative alpha / beta
PARAM_MIX = ((1.0, 0.0, 0.0), (1.2, 0.0, 0.0), (0.8, 0.0, 0.0), (1.0, 0.5, 0.0), (1.0, 0.0, 0.3),
             (1.3, 0.7, 0.25), (1.7, -0.4, -0.15))

# (rows, V, ld, n_slots): an odd ld (rows and state rows start unaligned, except row 0 / slot 0:
# vector body + the V % 8 tail), an aligned ld with a tail, one row and more rows than one pass of
# anything at the Llama-2 vocabulary with a 160-slot table, and the Llama-3 vocabulary
KERNEL_CASES = ((3, 1003, 1008 + 5, 5), (4, 1003, 1008, 6), (1, 32000, 32000, 160), (129, 32000, 32000, 160),
                (2, 128256, 128256, 3))


@dataclass(frozen=True)
class Case:
    rows: int
    V: int
    ld: int
    n_slots: int
    logits: np.ndarray     # uint16 [rows, ld] bf16 bit patterns
    state: np.ndarray      # uint16 [n_slots, ld]
    slot: np.ndarray       # int32 [rows], distinct, not the identity
    tokens: np.ndarray     # int32 [rows], -1 = none
    rep: np.ndarray        # fp32 [rows]
    pres: np.ndarray
    freq: np.ndarray


def bf16_bits(a: np.ndarray) -> np.ndarray:
    return P.bf16_rne_bits(np.asarray(a, dtype=np.float32))


def token_choices(V: int) -> tuple:
    """Column 0, V - 1, inside the vector body, in the V % 8 tail (the last vector's start when
    there is no tail) and none."""
    tail = (V & ~7) + (V % 8) // 2 if V % 8 else V - 8
    return (0, V - 1, 8 * 37 + 3, tail, -1)


@functools.lru_cache(maxsize=None)
def make_case(rows: int, V: int, ld: int, n_slots: int, mix_offset: int = 0) -> Case:
    rng = np.random.default_rng(1000 * rows + V + ld + mix_offset)
    logits = np.full((rows, ld), LOGIT_PAD, dtype=np.uint16)
    logits[:, :V] = bf16_bits(4.0 * rng.standard_normal((rows, V)))
    state = np.full((n_slots, ld), STATE_PAD, dtype=np.uint16)
    st = np.zeros((n_slots, V), dtype=np.uint16)
    hot = rng.random((n_slots, V)) < 0.02          # about 2 % non-zero: counts 1..5 and / or the prompt bit
    cnt = rng.integers(0, 6, (n_slots, V)).astype(np.uint16)
    bit = (rng.random((n_slots, V)) < 0.5).astype(np.uint16) * np.uint16(P.PROMPT_BIT)
    st[hot] = (cnt | bit)[hot]
    if rows == 1:
        slot = np.array([n_slots - 3], dtype=np.int32)
    elif rows < 8:   # row 0 -> slot 0: with an aligned base both take the 16-byte path
        slot = np.concatenate([[0], 1 + rng.permutation(n_slots - 1)[:rows - 1]]).astype(np.int32)
    else:
        slot = rng.permutation(n_slots)[:rows].astype(np.int32)
        assert (slot != np.arange(rows)).any()
    tc = token_choices(V)
    tokens = np.array([tc[(r + 3 + mix_offset) % len(tc)] for r in range(rows)], dtype=np.int32)
    kinds = [(r + (5 if rows < 7 else 0) + mix_offset) % len(PARAM_MIX) for r in range(rows)]
    rep, pres, freq = (np.array([PARAM_MIX[k][j] for k in kinds], dtype=np.float32) for j in range(3))
    special = np.array([0.0, -0.0, 2.0 ** -20, -(2.0 ** -20)], dtype=np.float32)
    for r in range(rows):
        s, t = int(slot[r]), int(tokens[r])
        # +0, -0 and +-2^-20 on columns whose state is non-zero (and on some whose state is zero)
        cols = rng.choice(V, 8, replace=False)
        logits[r, cols] = bf16_bits(np.tile(special, 2))
        st[s, cols[:4]] = np.array([2, P.PROMPT_BIT, P.PROMPT_BIT | 1, 5], dtype=np.uint16)
        st[s, cols[4:]] = 0
        if t >= 0:   # the count at t: one below saturation, saturated (with the prompt bit), or as drawn
            if r % 4 == 1:
                st[s, t] = P.COUNT_MAX - 1
            elif r % 4 == 2:
                st[s, t] = P.PROMPT_BIT | P.COUNT_MAX
    state[:, :V] = st
    return Case(rows, V, ld, n_slots, logits, state, slot, tokens, rep, pres, freq)


@functools.lru_cache(maxsize=None)
def reference(rows: int, V: int, ld: int, n_slots: int, mix_offset: int = 0):
    """(logits uint16 [rows, ld], state uint16 [n_slots, ld]) of the case after one launch."""
    c = make_case(rows, V, ld, n_slots, mix_offset)
    return P.penalize_reference(c.logits, V, c.state, c.slot, c.tokens, c.rep, c.pres, c.freq)


def direct(l_bits, st, t, rho, alpha, beta):
    """The contract, one column at a time in numpy float32 scalars (independent of
    ``ops.penalties``): bf16 bit patterns [V] and states [V] -> (bits, states)."""
    rho, alpha, beta = np.float32(rho), np.float32(alpha), np.float32(beta)
    out_l, out_s = np.array(l_bits, dtype=np.uint16), np.array(st, dtype=np.uint16)
    if rho == 1 and alpha == 0 and beta == 0:
        return out_l, out_s
    for v in range(out_l.size):
        s = int(out_s[v])
        c = min((s & 0x7FFF) + (1 if v == t else 0), 0x7FFF)
        out_s[v] = (s & 0x8000) | c
        x = torch.tensor([int(out_l[v]) - (1 << 16 if out_l[v] >= 0x8000 else 0)], dtype=torch.int16)
        x = np.float32(x.view(torch.bfloat16).float().item())
        done = False
        if rho != 1 and ((s & 0x8000) or c > 0):
            x = np.float32(x * rho) if x < 0 else np.float32(x / rho)
            done = True
        if c > 0:
            pen = np.float32(np.float32(c) * beta)
            pen = np.float32(pen + alpha)
            x = np.float32(x - pen)
            done = True
        if done:
            b = torch.tensor([float(x)], dtype=torch.float32).to(torch.bfloat16).view(torch.int16).item()
            out_l[v] = b & 0xFFFF
    return out_l, out_s


def to_bf16(bits: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16).copy()).view(torch.bfloat16)


def to_i16(bits: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16).copy())
