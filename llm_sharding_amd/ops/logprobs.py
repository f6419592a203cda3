"""Per-token log-probabilities and top-N alternatives: the ctypes binding of
csrc/sampling/logprobs.hip and the numpy fp64 reference of the same contract (the CPU
implementation and the tests' oracle).

Contract per row (bf16 logits ``l[0..V)`` in a row of ``ld >= V`` columns, ``n_top`` and a
``target`` token):

1. columns ``>= V`` are never read; ``n_top < 0``: the row is skipped, none of its outputs written;
2. ``lse = max + ln(sum over v < V of exp(l_v - max))``; a ``-inf`` logit contributes nothing
   (``+inf`` and NaN logits are outside the contract);
3. ``tok_lp = l_target - lse`` and ``tok_rank = 1 +`` the number of ``v < V`` with
   ``l_v > l_target`` (strictly, on the bf16 values); ``target < 0`` or ``>= V``: neither is written;
4. ``top_id[0..n)``, ``n = min(n_top, TOP_MAX, V)``: the ``n`` largest logits in descending order,
   equal logits by ascending index; ``top_lp`` their log-probabilities; entries ``[n, TOP_MAX)``
   are ``-1`` / ``-inf``.

The device sums the exponentials as 32-bit fixed point in 64-bit integers, so its values are
bitwise reproducible and within 1e-4 of this reference for ``V <= 2^17`` (derivation in the
kernel's header); ids and ranks are exact.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional

import numpy as np
import torch

from .sampling import _as_f64_logits, _per_row

TOP_MAX = 20


class Logprobs(NamedTuple):
    """``lse`` / ``tok_lp`` fp [rows], ``tok_rank`` int [rows], ``top_id`` int [rows, TOP_MAX],
    ``top_lp`` fp [rows, TOP_MAX] (numpy from the reference, torch from the device)."""
    lse: object
    tok_lp: object
    tok_rank: object
    top_id: object
    top_lp: object


# ------------------------------------------------------------------------------ reference
def logprobs_reference(logits, V: int, n_top, target) -> Logprobs:
    """The contract in numpy fp64. ``logits``: [rows, >= V] (torch or numpy; values are taken as
    given, pass bf16-rounded values to mirror the device); ``n_top`` / ``target``: per row (or
    one value for all rows). What the device leaves unwritten is NaN (``lse``, ``tok_lp``), 0
    (``tok_rank``) and -1 / -inf (``top_id`` / ``top_lp``) here."""
    L = _as_f64_logits(logits, V)
    rows = L.shape[0]
    n_top = _per_row(n_top, rows, np.int64)
    target = _per_row(target, rows, np.int64)
    lse = np.full(rows, np.nan)
    tok_lp = np.full(rows, np.nan)
    tok_rank = np.zeros(rows, dtype=np.int64)
    top_id = np.full((rows, TOP_MAX), -1, dtype=np.int64)
    top_lp = np.full((rows, TOP_MAX), -np.inf)
    for r in range(rows):
        if n_top[r] < 0:
            continue
        l = L[r]
        m = l.max()
        with np.errstate(divide="ignore"):
            lse[r] = m + np.log(np.exp(l - m).sum())
        t = int(target[r])
        if 0 <= t < V:
            tok_lp[r] = l[t] - lse[r]
            tok_rank[r] = 1 + int((l > l[t]).sum())
        n = int(min(n_top[r], TOP_MAX, V))
        if n > 0:
            order = np.argsort(-l, kind="stable")[:n]  # descending value, ascending index on ties
            top_id[r, :n] = order
            top_lp[r, :n] = l[order] - lse[r]
    return Logprobs(lse, tok_lp, tok_rank, top_id, top_lp)


# ------------------------------------------------------------------------------ HIP binding
_declared = None


def _lib() -> ctypes.CDLL:
    """The kernel library (``hip.lib()``) with ``lsa_logprobs`` declared."""
    global _declared
    from . import hip
    L = hip.lib()
    if _declared is not L:
        vp, i, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
        if not hasattr(L, "lsa_logprobs"):
            raise RuntimeError("the kernel library has no lsa_logprobs: rebuild it (python csrc/build.py)")
        L.lsa_logprobs.argtypes = [vp, ll, i, i, vp, vp, vp, vp, vp, vp, vp, vp, i, i, vp, vp]
        L.lsa_logprobs.restype = i
        _declared = L
    return L


def alloc_outputs(rows: int, device) -> Logprobs:
    """Output buffers of :func:`logprobs` for ``rows`` rows, prefilled with what the reference
    reports for an unwritten entry."""
    return Logprobs(torch.full((rows,), float("nan"), dtype=torch.float32, device=device),
                    torch.full((rows,), float("nan"), dtype=torch.float32, device=device),
                    torch.zeros(rows, dtype=torch.int32, device=device),
                    torch.full((rows, TOP_MAX), -1, dtype=torch.int32, device=device),
                    torch.full((rows, TOP_MAX), float("-inf"), dtype=torch.float32, device=device))


def logprobs(logits: torch.Tensor, V: int, rows: int, n_top: torch.Tensor, target: torch.Tensor,
             out: Logprobs, lp_history: Optional[torch.Tensor] = None,
             step_ctr: Optional[torch.Tensor] = None) -> None:
    """``lsa_logprobs`` on the first ``rows`` rows of bf16 ``logits`` [>= rows, ld >= V] (row bases
    need not be 16-byte aligned). ``n_top`` int32 [rows] (-1: skip the row, 0..TOP_MAX), ``target``
    int32 [rows]; ``out``: ``lse`` / ``tok_lp`` fp32 [rows], ``tok_rank`` int32 [rows], ``top_id``
    int32 / ``top_lp`` fp32 [rows, TOP_MAX], all contiguous. ``lp_history`` (fp32 [len, rows]) with
    ``step_ctr`` (int32 [1], the step counter ``argmax_finalize`` has just advanced): ``tok_lp`` is
    also stored at ``lp_history[step_ctr - 1]`` (counters outside 1..len: not stored).
    No host reads: graph-capturable."""
    from .hip import _check, _p, _req, _stream
    from .sampling import _chk
    _req(logits.is_cuda and logits.dtype == torch.bfloat16 and logits.dim() == 2 and logits.stride(1) == 1,
         "logprobs: logits must be a row-major bf16 cuda matrix")
    _req(1 <= rows <= logits.shape[0] and 1 <= V <= logits.shape[1] and rows <= 65535,
         f"logprobs: rows={rows}, V={V} outside logits {tuple(logits.shape)}")
    _req(rows == 1 or logits.stride(0) >= V, "logprobs: row stride below V")
    _chk(n_top, torch.int32, rows, "n_top")
    _chk(target, torch.int32, rows, "target")
    _chk(out.lse, torch.float32, rows, "lse")
    _chk(out.tok_lp, torch.float32, rows, "tok_lp")
    _chk(out.tok_rank, torch.int32, rows, "tok_rank")
    _chk(out.top_id, torch.int32, rows * TOP_MAX, "top_id")
    _chk(out.top_lp, torch.float32, rows * TOP_MAX, "top_lp")
    hist = (None, 0, 0, None)
    if lp_history is not None:
        _req(lp_history.dim() == 2 and lp_history.shape[1] >= rows and lp_history.shape[0] >= 1,
             "logprobs: lp_history must be [len >= 1, >= rows]")
        _chk(lp_history, torch.float32, rows, "lp_history")
        _chk(step_ctr, torch.int32, 1, "step_ctr")
        hist = (lp_history, lp_history.stride(0), lp_history.shape[0], step_ctr)
    for t in (n_top, target, *out, *(x for x in (hist[0], hist[3]) if x is not None)):
        _req(t.device == logits.device, "logprobs: every argument lives on the logits' device")
    ld = logits.stride(0) if rows > 1 else max(logits.stride(0), V)
    rc = _lib().lsa_logprobs(_p(logits), ld, V, rows, _p(n_top), _p(target), _p(out.lse), _p(out.tok_lp),
                             _p(out.tok_rank), _p(out.top_id), _p(out.top_lp), _p(hist[0]), hist[1], hist[2],
                             _p(hist[3]), _stream())
    _check(rc, "lsa_logprobs")


__all__ = ["TOP_MAX", "Logprobs", "logprobs_reference", "alloc_outputs", "logprobs"]
