"""Repetition / presence / frequency penalties: the ctypes binding of csrc/sampling/penalty.hip
and the numpy float32 reference of the same contract (the CPU implementation and the tests'
oracle).

Per sequence slot one ``uint16`` per vocabulary entry, ``state[slot, v]``: bit 15 = "v occurs in
the prompt", bits 0..14 = the number of times v has been generated, saturating at 32767.

Contract per row with slot ``s``, input token ``t`` (the token the previous step generated and
this step embeds; ``t < 0`` or no ``tokens_in``: none) and parameters ``rho`` (repetition, finite
and > 0, 1 = off), ``alpha`` (presence, finite, 0 = off), ``beta`` (frequency, finite, 0 = off):

``rho == 1 and alpha == 0 and beta == 0``: the row is skipped - logits and state stay
bit-identical and nothing is counted. Otherwise, for every column ``v < V``:

1. ``c = min((state & 0x7fff) + (v == t), 0x7fff)``; the new count is stored, the prompt bit kept;
2. ``x = fp32(l_v)``;
3. ``rho != 1`` and (prompt bit set or ``c > 0``): ``x = x * rho if x < 0 else x / rho`` (the set
   semantics of HF's ``RepetitionPenaltyLogitsProcessor`` over prompt + generated tokens; a
   correctly rounded fp32 division);
4. ``c > 0``: ``pen = fp32(c) * beta``, ``pen = pen + alpha``, ``x = x - pen`` (three separately
   rounded fp32 operations; generated tokens only, as OpenAI / vLLM define the two penalties);
5. ``l_v = bf16_rne(x)``, written only where step 3 or 4 applied.

Columns ``>= V`` (the lm_head padding) are never read or written.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch

PROMPT_BIT = 0x8000
COUNT_MAX = 0x7FFF


# ------------------------------------------------------------------------------ reference
def bf16_rne_bits(x: np.ndarray) -> np.ndarray:
    """float32 -> bf16 bit patterns (uint16), round to nearest even (finite values)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)


def bf16_bits_to_f32(b: np.ndarray) -> np.ndarray:
    return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def _bits_of(logits) -> np.ndarray:
    """bf16 torch tensor or uint16 array -> a fresh uint16 [rows, ld] array of bit patterns."""
    if isinstance(logits, torch.Tensor):
        if logits.dtype != torch.bfloat16:
            raise ValueError("penalize_reference takes bf16 logits (or their uint16 bit patterns)")
        a = logits.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16).copy()
    else:
        a = np.array(logits, dtype=np.uint16)
    return a[None] if a.ndim == 1 else a


def _state_of(state) -> np.ndarray:
    if isinstance(state, torch.Tensor):
        state = state.detach().cpu().contiguous().view(torch.int16).numpy()
    a = np.array(state).view(np.uint16)
    if a.ndim != 2:
        raise ValueError("penalty state is a [n_slots, >= V] table")
    return a


def penalized_values(l32: np.ndarray, st: np.ndarray, t: int, rho, alpha, beta):
    """Steps 1-4 on one row: fp32 logits ``l32`` [V], states ``st`` uint16 [V] -> (x fp32 [V]
    before the bf16 rounding, new states uint16 [V], applied bool [V])."""
    rho, alpha, beta = np.float32(rho), np.float32(alpha), np.float32(beta)
    cnt = (st & np.uint16(COUNT_MAX)).astype(np.int64)
    if 0 <= t < cnt.size:
        cnt[t] = min(cnt[t] + 1, COUNT_MAX)
    prompt = (st & np.uint16(PROMPT_BIT)) != 0
    new = ((st & np.uint16(PROMPT_BIT)) | cnt.astype(np.uint16)).astype(np.uint16)
    x = np.array(l32, dtype=np.float32)
    applied = np.zeros(cnt.size, dtype=bool)
    if rho != np.float32(1.0):
        m = prompt | (cnt > 0)
        x = np.where(m, np.where(x < 0, x * rho, x / rho), x).astype(np.float32)
        applied |= m
    m = cnt > 0
    pen = (cnt.astype(np.float32) * beta).astype(np.float32)
    pen = (pen + alpha).astype(np.float32)
    x = np.where(m, (x - pen).astype(np.float32), x).astype(np.float32)
    applied |= m
    return x, new, applied


def penalize_reference(logits_bf16, V: int, state_u16, slot, tokens_in, rep, pres, freq):
    """The contract in numpy float32, operation by operation. ``logits_bf16``: [rows, >= V] bf16
    tensor (or uint16 bit patterns); ``state_u16``: [n_slots, >= V] (uint16 / int16, numpy or
    torch); ``slot``: per row; ``tokens_in``: per row or None; ``rep / pres / freq``: per row.
    The inputs are not modified. Returns ``(logits, state)``: a bf16 tensor (a uint16 array when
    bit patterns were given) and a uint16 array, both of the inputs' full shapes."""
    was_tensor = isinstance(logits_bf16, torch.Tensor)
    one_row = (logits_bf16.dim() if was_tensor else np.ndim(logits_bf16)) == 1
    bits = _bits_of(logits_bf16)
    state = _state_of(state_u16).copy()
    rows = bits.shape[0]
    slot = [int(s) for s in (slot.tolist() if hasattr(slot, "tolist") else slot)]
    if tokens_in is None:
        tokens_in = [-1] * rows
    tokens_in = [int(t) for t in (tokens_in.tolist() if hasattr(tokens_in, "tolist") else tokens_in)]

    def per_row(x):
        x = x.tolist() if hasattr(x, "tolist") else x
        x = list(x) if isinstance(x, (list, tuple)) else [x] * rows
        return np.asarray(x, dtype=np.float32)

    rep, pres, freq = per_row(rep), per_row(pres), per_row(freq)
    if not (len(slot) == len(tokens_in) == rep.size == pres.size == freq.size == rows):
        raise ValueError(f"penalize_reference: per-row arguments do not match {rows} rows")
    if bits.shape[1] < V or state.shape[1] < V:
        raise ValueError("penalize_reference: a row is shorter than V")
    for r in range(rows):
        if rep[r] == 1.0 and pres[r] == 0.0 and freq[r] == 0.0:
            continue
        s = slot[r]
        if not 0 <= s < state.shape[0]:
            raise ValueError(f"penalize_reference: slot {s} outside the table of {state.shape[0]}")
        x, new, applied = penalized_values(bf16_bits_to_f32(bits[r, :V]), state[s, :V], tokens_in[r],
                                           rep[r], pres[r], freq[r])
        state[s, :V] = new
        bits[r, :V] = np.where(applied, bf16_rne_bits(x), bits[r, :V])
    if one_row:
        bits = bits[0]
    if was_tensor:
        return torch.from_numpy(bits.view(np.int16).copy()).view(torch.bfloat16), state
    return bits, state


# ------------------------------------------------------------------------------ HIP binding
_declared = None


def _lib() -> ctypes.CDLL:
    """The kernel library (``hip.lib()``) with the penalty entry points declared."""
    global _declared
    from . import hip
    L = hip.lib()
    if _declared is not L:
        vp, i, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
        if not hasattr(L, "lsa_penalize"):
            raise RuntimeError("the kernel library has no lsa_penalize: rebuild it (python csrc/build.py)")
        L.lsa_penalize.argtypes = [vp, ll, i, i, vp, vp, vp, ll, i, vp, vp, vp, vp]
        L.lsa_penalize.restype = i
        L.lsa_penalize_calls.argtypes = []
        L.lsa_penalize_calls.restype = ll
        _declared = L
    return L


def penalize_calls() -> int:
    """How often this process has enqueued ``lsa_penalize`` (a captured graph counts at capture)."""
    return int(_lib().lsa_penalize_calls())


def penalize(logits: torch.Tensor, V: int, rows: int, slot: torch.Tensor, tokens_in: Optional[torch.Tensor],
             state: torch.Tensor, rep: torch.Tensor, pres: torch.Tensor, freq: torch.Tensor) -> None:
    """``lsa_penalize``: count ``tokens_in`` (int32 [rows] or None) into ``state`` (int16 / uint16
    [n_slots, >= V], the rows ``slot`` int32 [rows], distinct) and penalise the first ``rows`` rows
    of bf16 ``logits`` [>= rows, ld >= V] in place; ``rep / pres / freq``: fp32 [rows]. No host
    reads: graph-capturable."""
    from .hip import _check, _p, _req, _stream
    from .sampling import _chk
    _req(logits.is_cuda and logits.dtype == torch.bfloat16 and logits.dim() == 2 and logits.stride(1) == 1,
         "penalize: logits must be a row-major bf16 cuda matrix")
    _req(1 <= rows <= logits.shape[0] and 1 <= V <= logits.shape[1] and rows <= 65535,
         f"penalize: rows={rows}, V={V} outside logits {tuple(logits.shape)}")
    _req(rows == 1 or logits.stride(0) >= V, "penalize: row stride below V")
    _req(state.is_cuda and state.dtype in (torch.int16, torch.uint16) and state.dim() == 2 and state.stride(1) == 1
         and state.shape[1] >= V and (state.shape[0] == 1 or state.stride(0) >= V) and state.device == logits.device,
         "penalize: state must be a row-major 16-bit cuda table [n_slots, >= V] on the logits' device")
    _chk(slot, torch.int32, rows, "slot")
    if tokens_in is not None:
        _chk(tokens_in, torch.int32, rows, "tokens_in")
    _chk(rep, torch.float32, rows, "rep")
    _chk(pres, torch.float32, rows, "pres")
    _chk(freq, torch.float32, rows, "freq")
    ld = logits.stride(0) if rows > 1 else max(logits.stride(0), V)
    lds = state.stride(0) if state.shape[0] > 1 else max(state.stride(0), V)
    rc = _lib().lsa_penalize(_p(logits), ld, V, rows, _p(slot), _p(tokens_in), _p(state), lds, state.shape[0],
                             _p(rep), _p(pres), _p(freq), _stream())
    _check(rc, "lsa_penalize")


__all__ = ["PROMPT_BIT", "COUNT_MAX", "bf16_rne_bits", "bf16_bits_to_f32", "penalized_values", "penalize_reference",
           "penalize", "penalize_calls"]
