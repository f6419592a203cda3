"""Speculative decoding's two kernels: the ctypes bindings of csrc/spec/spec_decode.hip and the
numpy references of the same contracts (what CPU engines run and the tests' oracle).

State of ``n_seq`` sequences verified ``k`` drafts at a time (``rows = n_seq * (k + 1)``; row
``r0 + j``, ``r0 = s * (k + 1)``, belongs to sequence ``s``):

* ``hist`` int32 ``[n_seq, ld]`` (``ld >= max_seq``): the known tokens, prompt + accepted;
* ``hlen`` / ``limit`` / ``done`` int32 ``[n_seq]``: their number, the absolute cap on it (prompt
  length + ``max_new_tokens``), the finished flag;
* ``eos`` int32 ``[8]``: end-of-sequence ids, padded with -1;
* ``tokens`` / ``pos`` / ``cand`` int32 ``[rows]``: what the step is fed and the model's token per row;
* ``script`` int32 ``[n_seq, ld]`` (optional): a proposed token per absolute position.

Invariant: the slot's KV cache holds positions ``[0, hlen - 1)``; the last known token has not
been fed yet (``DecodeGraph.tokens`` / ``pos``' convention).

Both operations take ``L = min(max(hlen[s], 1), ld)`` - ``hlen[s]`` itself in every state the
contract allows. The caller guarantees ``limit[s] + k <= max_seq``; ``hlen`` never passes ``limit``,
so no row carries a position outside the slot.

**Draft.** Row 0: ``tokens = hist[L-1]``, ``pos = L-1``; row ``j`` (1..k): draft ``d[j-1]`` at
``pos = L-1+j``. Lookup mode (``1 <= nmin <= nmax <= 8``): for every end ``e`` in ``[0, L-2]``,
``m(e)`` = the largest ``m <= nmax`` with ``e - t >= 0`` and ``hist[e-t] == hist[L-1-t]`` for all
``t < m``; among ``e`` with ``m(e) >= nmin`` the largest ``(m(e) << 32) | e`` wins; with
``c = e + 1``, ``d[j] = hist[c+j]`` if ``c + j < L`` else ``d[c+j-L]``. No match: ``d[j] = hist[L-1]``.
``matched[s]`` = the winning ``m`` (0: none). Script mode: ``d[j] = script[s, L+j]`` if
``L + j < ld`` else 0, ``matched[s] = 1``. ``match_ctr[s]`` counts the steps of a sequence that is
not done whose ``matched`` is non-zero.

**Accept.** ``done[s]``: ``n_acc[s] = 0``, nothing else written. Otherwise ``a`` = the leading
``j < k`` with ``tokens[r0+j+1] == cand[r0+j]``; ``m = min(a + 1, limit[s] - L, ld - L)``; the first
``j < m`` with ``cand[r0+j]`` an EOS id gives ``m = j + 1``, ``done = 1``; ``L + m == limit[s]`` (or
``m <= 0``, then ``m = 0``) gives ``done = 1``; ``hist[s, L:L+m] = cand[r0:r0+m]``, ``hlen[s] = L + m``,
``n_acc[s] = m``, ``acc_history[step, s] = m`` (``step = step_ctr[0] < len(acc_history)``);
``step_ctr[0] += 1`` per call. Nothing else is written.

**Draft model** (csrc/spec/spec_draft_model.hip; :func:`draft_model_reference`). The drafts come
from a second, smaller engine of the same vocabulary, run greedily inside the step; accept is
unchanged. ``dmax`` is the draft engine's ``max_seq`` (``>= max_seq``).

1. Invariant: before a step the draft engine's slot holds valid K/V for positions ``[0, L - 2)`` at
   least (``admit`` prefills it with ``hist[0:L-1]``).
2. Iteration 0, two draft rows per sequence: ``hist[pa]`` at ``pa = max(L - 2, 0)`` and ``hist[L-1]``
   at ``L - 1`` (``L == 1``: the same row twice); ``d[0]`` = the arg-max of the second row. Two rows
   are always enough: the previous step (length ``L'``) fed the draft positions ``L' - 2 .. L' + k - 2``
   and ``L <= L' + a + 1`` after ``a <= k`` accepted drafts, so only position ``L - 2`` can be missing,
   and only when ``a == k``; rewriting a valid cell is harmless.
3. Iterations ``j = 1 .. k-1``, one draft row per sequence: ``d[j-1]`` at ``L - 1 + j``; its arg-max
   is ``d[j]``. Draft positions are clamped into ``[0, dmax)`` (a no-op while ``limit + k <= max_seq``).
4. Target rows as in script mode: row 0 ``hist[L-1]`` at ``L - 1``, row ``j + 1`` ``d[j]`` at ``L + j``,
   ``matched[s] = 1``, ``match_ctr[s] += 1`` unless done. A done sequence is drafted like any other.

``lsa_spec_dm_begin`` writes iteration 0's draft rows (token, position, slot), the target's row-0
token and all ``k + 1`` target positions; ``lsa_spec_dm_chain(j)`` writes ``d[j]`` into the target's
row ``j + 1`` and, while ``j + 1 < k``, the draft's next row (token and position).
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch

MAX_K = 15
MAX_NGRAM = 8
MAX_ROWS = 128  # the decode path's row limit (StageEngine.DECODE_MAX_ROWS), as the launchers check it
N_EOS = 8


def check_shape(n_seq: int, k: int, ld: int, max_seq: int, ngram=None) -> None:
    """The launchers' own refusals, as ``ValueError``."""
    if not 1 <= k <= MAX_K:
        raise ValueError(f"speculative: k must be in [1, {MAX_K}], got {k}")
    if n_seq < 1 or n_seq * (k + 1) > MAX_ROWS:
        raise ValueError(f"speculative: {n_seq} sequences x (k + 1 = {k + 1}) rows exceed the decode path's {MAX_ROWS} rows")
    if max_seq < 1 or ld < max_seq:
        raise ValueError(f"speculative: ld {ld} must be >= max_seq {max_seq} >= 1")
    if ngram is not None:
        nmin, nmax = ngram
        if not 1 <= nmin <= nmax <= MAX_NGRAM:
            raise ValueError(f"speculative: n-gram lengths must satisfy 1 <= min <= max <= {MAX_NGRAM}, got {ngram}")


def eos_array(eos_ids) -> np.ndarray:
    ids = [int(t) for t in (eos_ids or ())]
    if len(ids) > N_EOS or any(t < 0 for t in ids):
        raise ValueError(f"speculative: at most {N_EOS} non-negative end-of-sequence ids, got {ids}")
    return np.array(ids + [-1] * (N_EOS - len(ids)), dtype=np.int32)


def _np(x) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.asarray(x)


def _clamp_len(L: int, ld: int) -> int:
    return min(max(int(L), 1), ld)


# ------------------------------------------------------------------------------ references
def draft_reference(hist, hlen, k: int, max_seq: int, ngram=(1, 3), script=None, done=None, match_ctr=None):
    """The draft contract in numpy. ``hist`` [n_seq, ld], ``hlen`` [n_seq] (read only); returns
    ``(tokens, pos, matched)``: int32 [n_seq * (k + 1)] twice and int32 [n_seq]. ``match_ctr``
    (an int32 numpy array) is updated in place."""
    hist, hlen = _np(hist), _np(hlen)
    n_seq, ld = hist.shape
    check_shape(n_seq, k, ld, max_seq, None if script is not None else ngram)
    script = None if script is None else _np(script)
    tokens = np.zeros(n_seq * (k + 1), dtype=np.int32)
    pos = np.zeros_like(tokens)
    matched = np.zeros(n_seq, dtype=np.int32)
    for s in range(n_seq):
        h = hist[s]
        L = _clamp_len(hlen[s], ld)
        r0 = s * (k + 1)
        tokens[r0], pos[r0] = h[L - 1], L - 1
        if script is not None:
            d = [int(script[s, L + j]) if L + j < ld else 0 for j in range(k)]
            matched[s] = 1
        else:
            nmin, nmax = ngram
            best = -1
            if L >= 2:  # m(e) of every end position at once: t-th comparison of all e per pass
                e = np.arange(L - 1, dtype=np.int64)
                m = np.zeros(L - 1, dtype=np.int64)
                go = np.ones(L - 1, dtype=bool)
                for t in range(nmax):
                    go &= e - t >= 0
                    go[go] = h[e[go] - t] == h[L - 1 - t]
                    m += go
                best = int(np.where(m >= nmin, (m << 32) | e, -1).max())
            d = []
            if best < 0:
                d = [int(h[L - 1])] * k
            else:
                c = (best & 0xFFFFFFFF) + 1
                for j in range(k):
                    d.append(int(h[c + j]) if c + j < L else d[c + j - L])
                matched[s] = best >> 32
        for j in range(k):
            tokens[r0 + 1 + j], pos[r0 + 1 + j] = d[j], L + j
        if match_ctr is not None and matched[s] and not (done is not None and _np(done)[s]):
            match_ctr[s] += 1
    return tokens, pos, matched


def accept_reference(hist, hlen, limit, done, eos, tokens, cand, k: int, max_seq: int, acc_history=None,
                     step_ctr=None) -> np.ndarray:
    """The accept contract in numpy, in place on the int32 numpy arrays ``hist``, ``hlen``, ``done``
    (and ``acc_history`` [steps, >= n_seq], ``step_ctr`` [1]). Returns ``n_acc`` int32 [n_seq]."""
    n_seq, ld = hist.shape
    check_shape(n_seq, k, ld, max_seq)
    tokens, cand, eos, limit = _np(tokens), _np(cand), _np(eos), _np(limit)
    eos_set = {int(t) for t in eos if t >= 0}
    step = 0 if step_ctr is None else int(step_ctr[0])
    n_acc = np.zeros(n_seq, dtype=np.int32)
    for s in range(n_seq):
        if done[s]:
            continue
        L = _clamp_len(hlen[s], ld)
        r0 = s * (k + 1)
        a = 0
        while a < k and tokens[r0 + a + 1] == cand[r0 + a]:
            a += 1
        m = min(a + 1, int(limit[s]) - L, ld - L)
        fin = m <= 0
        m = max(m, 0)
        for j in range(m):
            if int(cand[r0 + j]) in eos_set:
                m, fin = j + 1, True
                break
        if L + m == int(limit[s]):
            fin = True
        hist[s, L:L + m] = cand[r0:r0 + m]
        hlen[s] = L + m
        n_acc[s] = m
        if fin:
            done[s] = 1
        if acc_history is not None and step < acc_history.shape[0]:
            acc_history[step, s] = m
    if step_ctr is not None:
        step_ctr[0] = step + 1
    return n_acc


def check_draft_shape(n_seq: int, k: int, ld: int, max_seq: int, draft_max_seq: int) -> None:
    check_shape(n_seq, k, ld, max_seq)
    if draft_max_seq < max_seq:
        raise ValueError(f"speculative: the draft engine's max_seq {draft_max_seq} is below the target's {max_seq}")


def _draft_pos(p: int, dmax: int) -> int:
    return min(max(int(p), 0), dmax - 1)


def dm_begin_reference(hist, hlen, slots, k: int, max_seq: int, draft_max_seq: int, done=None, match_ctr=None) -> dict:
    """``lsa_spec_dm_begin`` in numpy: ``d_tokens`` / ``d_pos`` / ``d_slot`` int32 [2 * n_seq] (the
    draft engine's catch-up rows), ``tokens`` / ``pos`` int32 [n_seq * (k + 1)] (of ``tokens`` only
    row 0 of every sequence is written: the others are returned as 0) and ``matched`` int32
    [n_seq]. ``match_ctr`` (an int32 numpy array) is updated in place."""
    hist, hlen, slots = _np(hist), _np(hlen), _np(slots)
    n_seq, ld = hist.shape
    check_draft_shape(n_seq, k, ld, max_seq, draft_max_seq)
    out = {"d_tokens": np.zeros(2 * n_seq, dtype=np.int32), "d_pos": np.zeros(2 * n_seq, dtype=np.int32),
           "d_slot": np.zeros(2 * n_seq, dtype=np.int32), "tokens": np.zeros(n_seq * (k + 1), dtype=np.int32),
           "pos": np.zeros(n_seq * (k + 1), dtype=np.int32), "matched": np.ones(n_seq, dtype=np.int32)}
    for s in range(n_seq):
        L = _clamp_len(hlen[s], ld)
        pa, r0 = max(L - 2, 0), s * (k + 1)
        out["d_tokens"][2 * s:2 * s + 2] = hist[s, pa], hist[s, L - 1]
        out["d_pos"][2 * s:2 * s + 2] = _draft_pos(pa, draft_max_seq), _draft_pos(L - 1, draft_max_seq)
        out["d_slot"][2 * s:2 * s + 2] = slots[s]
        out["tokens"][r0] = hist[s, L - 1]
        out["pos"][r0:r0 + k + 1] = L - 1 + np.arange(k + 1)
        if match_ctr is not None and not (done is not None and _np(done)[s]):
            match_ctr[s] += 1
    return out


def dm_chain_reference(amax, hlen, ld: int, k: int, j: int, max_seq: int, draft_max_seq: int, tokens: np.ndarray):
    """``lsa_spec_dm_chain`` in numpy: iteration ``j``'s arg-max tokens ``amax`` [n_seq] go into
    ``tokens`` (in place, row ``j + 1`` of every sequence); returns the draft engine's next rows
    ``(d_tokens1, d_pos1)`` int32 [n_seq], or None when ``j + 1 == k``."""
    amax, hlen = _np(amax), _np(hlen)
    n_seq = amax.shape[0]
    check_draft_shape(n_seq, k, ld, max_seq, draft_max_seq)
    if not 0 <= j < k:
        raise ValueError(f"speculative: draft iteration {j} outside [0, {k})")
    tokens[np.arange(n_seq) * (k + 1) + j + 1] = amax
    if j + 1 == k:
        return None
    d_pos1 = np.array([_draft_pos(_clamp_len(hlen[s], ld) + j, draft_max_seq) for s in range(n_seq)], dtype=np.int32)
    return amax.astype(np.int32), d_pos1


def draft_model_reference(hist, hlen, k: int, max_seq: int, draft_max_seq: int, draft_step, slots=None, done=None,
                          match_ctr=None):
    """The draft-model contract in numpy (module docstring, **Draft model**). ``draft_step(tokens,
    pos, slot, out_rows)`` runs the draft engine on the given rows (int32 arrays of one length: two
    rows per sequence on iteration 0, then one) and returns the greedy token of each row of
    ``out_rows``, one per sequence. ``slots`` (default ``0 .. n_seq - 1``): the KV slot per sequence.
    Returns ``(tokens, pos, matched, fed)``: the target's rows as :func:`draft_reference` returns
    them and ``fed``, the ``(tokens, pos, slot)`` of every draft iteration in order."""
    n_seq = _np(hist).shape[0]
    ld = _np(hist).shape[1]
    slots = np.arange(n_seq, dtype=np.int32) if slots is None else _np(slots).astype(np.int32)
    b = dm_begin_reference(hist, hlen, slots, k, max_seq, draft_max_seq, done, match_ctr)
    tokens, fed = b["tokens"], []
    d_tok, d_pos, d_slot, out_rows = b["d_tokens"], b["d_pos"], b["d_slot"], np.arange(n_seq) * 2 + 1
    for j in range(k):
        fed.append((d_tok.copy(), d_pos.copy(), d_slot.copy()))
        amax = np.asarray(draft_step(d_tok, d_pos, d_slot, out_rows), dtype=np.int32).reshape(n_seq)
        nxt = dm_chain_reference(amax, hlen, ld, k, j, max_seq, draft_max_seq, tokens)
        if nxt is not None:
            (d_tok, d_pos), d_slot, out_rows = nxt, slots, np.arange(n_seq)
    return tokens, b["pos"], b["matched"], fed


# ------------------------------------------------------------------------------ HIP bindings
_declared = None


def _lib() -> ctypes.CDLL:
    """The kernel library (``hip.lib()``) with the two entry points declared."""
    global _declared
    from . import hip
    L = hip.lib()
    if _declared is not L:
        vp, i, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
        if not hasattr(L, "lsa_spec_draft"):
            raise RuntimeError("the kernel library has no lsa_spec_draft: rebuild it (python csrc/build.py)")
        L.lsa_spec_draft.argtypes = [vp, ll, vp, i, i, i, i, vp, i, vp, vp, vp, vp, vp, vp]
        L.lsa_spec_draft.restype = i
        L.lsa_spec_accept.argtypes = [vp, ll, vp, vp, vp, vp, vp, vp, i, i, i, vp, vp, i, i, vp, vp]
        L.lsa_spec_accept.restype = i
        if not hasattr(L, "lsa_spec_dm_begin"):
            raise RuntimeError("the kernel library has no lsa_spec_dm_begin: rebuild it (python csrc/build.py)")
        L.lsa_spec_dm_begin.argtypes = [vp, ll, vp, vp, i, i, i, i, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.lsa_spec_dm_begin.restype = i
        L.lsa_spec_dm_chain.argtypes = [vp, vp, ll, i, i, i, i, i, vp, vp, vp, vp]
        L.lsa_spec_dm_chain.restype = i
        _declared = L
    return L


def _chk(t: Optional[torch.Tensor], n: int, what: str, optional: bool = False) -> None:
    if t is None and optional:
        return
    if t is None or not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.numel() >= n):
        raise ValueError(f"speculative: {what} must be a contiguous cuda int32 tensor of >= {n} entries")


def _chk_rows(t: Optional[torch.Tensor], n_seq: int, what: str, optional: bool = False) -> int:
    """``hist`` / ``script``: int32 [n_seq, >= 1] with unit column stride (any row stride and base)."""
    if t is None and optional:
        return 0
    if t is None or not (t.is_cuda and t.dtype == torch.int32 and t.dim() == 2 and t.shape[0] == n_seq
                         and t.stride(1) == 1 and (n_seq == 1 or t.stride(0) >= t.shape[1])):
        raise ValueError(f"speculative: {what} must be a cuda int32 [n_seq, ld] matrix with contiguous rows")
    return t.stride(0) if n_seq > 1 else max(t.stride(0), t.shape[1])


def _status(rc: int, what: str) -> None:
    from .hip import _check
    if rc == 1:  # LSA_BAD_SHAPE: the launcher's own refusal
        raise ValueError(f"{what}: bad shape")
    _check(rc, what)


def spec_draft(hist: torch.Tensor, hlen: torch.Tensor, k: int, max_seq: int, tokens: torch.Tensor, pos: torch.Tensor,
               ngram=(1, 3), script: Optional[torch.Tensor] = None, matched: Optional[torch.Tensor] = None,
               done: Optional[torch.Tensor] = None, match_ctr: Optional[torch.Tensor] = None) -> None:
    """``lsa_spec_draft`` on the current stream. The row stride of ``hist`` is ``ld``; ``script``
    shares it. No host reads: graph-capturable. The launcher's refusals arrive as ``ValueError``."""
    from .hip import _p, _stream
    n_seq = hist.shape[0] if hist is not None and hist.dim() == 2 else 0
    ld = _chk_rows(hist, n_seq, "hist")
    if script is not None and _chk_rows(script, n_seq, "script") != ld:
        raise ValueError("speculative: script must have hist's row stride")
    rows = n_seq * (k + 1)
    _chk(hlen, n_seq, "hlen")
    _chk(tokens, rows, "tokens")
    _chk(pos, rows, "pos")
    _chk(matched, n_seq, "matched", True)
    _chk(done, n_seq, "done", True)
    _chk(match_ctr, n_seq, "match_ctr", True)
    nmin, nmax = (1, 1) if script is not None else ngram
    rc = _lib().lsa_spec_draft(_p(hist), ld, _p(hlen), n_seq, int(k), int(nmin), int(nmax), _p(script), int(max_seq),
                               _p(tokens), _p(pos), _p(matched), _p(done), _p(match_ctr), _stream())
    _status(rc, "lsa_spec_draft")


def spec_accept(hist: torch.Tensor, hlen: torch.Tensor, limit: torch.Tensor, done: torch.Tensor, eos: torch.Tensor,
                tokens: torch.Tensor, cand: torch.Tensor, k: int, max_seq: int, n_acc: torch.Tensor,
                acc_history: Optional[torch.Tensor] = None, step_ctr: Optional[torch.Tensor] = None) -> None:
    """``lsa_spec_accept`` on the current stream (in place on ``hist`` / ``hlen`` / ``done``)."""
    from .hip import _p, _stream
    n_seq = hist.shape[0] if hist is not None and hist.dim() == 2 else 0
    ld = _chk_rows(hist, n_seq, "hist")
    rows = n_seq * (k + 1)
    for t, n, what in ((hlen, n_seq, "hlen"), (limit, n_seq, "limit"), (done, n_seq, "done"), (eos, N_EOS, "eos"),
                       (tokens, rows, "tokens"), (cand, rows, "cand"), (n_acc, n_seq, "n_acc")):
        _chk(t, n, what)
    _chk(step_ctr, 1, "step_ctr", True)
    hs = hl = 0
    if acc_history is not None:
        if not (acc_history.is_cuda and acc_history.dtype == torch.int32 and acc_history.dim() == 2
                and acc_history.stride(1) == 1 and acc_history.shape[1] >= n_seq and step_ctr is not None):
            raise ValueError("speculative: acc_history must be a cuda int32 [steps, >= n_seq] matrix, with a step_ctr")
        hs, hl = acc_history.stride(0), acc_history.shape[0]
    rc = _lib().lsa_spec_accept(_p(hist), ld, _p(hlen), _p(limit), _p(done), _p(eos), _p(tokens), _p(cand), n_seq, int(k),
                                int(max_seq), _p(n_acc), _p(acc_history), hs, hl, _p(step_ctr), _stream())
    _status(rc, "lsa_spec_accept")


def spec_dm_begin(hist: torch.Tensor, hlen: torch.Tensor, slots: torch.Tensor, k: int, max_seq: int, draft_max_seq: int,
                  d_tokens: torch.Tensor, d_pos: torch.Tensor, d_slot: torch.Tensor, tokens: torch.Tensor,
                  pos: torch.Tensor, matched: Optional[torch.Tensor] = None, done: Optional[torch.Tensor] = None,
                  match_ctr: Optional[torch.Tensor] = None) -> None:
    """``lsa_spec_dm_begin`` on the current stream: the draft engine's two catch-up rows per
    sequence and the target's row 0 and positions. No host reads: graph-capturable."""
    from .hip import _p, _stream
    n_seq = hist.shape[0] if hist is not None and hist.dim() == 2 else 0
    ld = _chk_rows(hist, n_seq, "hist")
    rows = n_seq * (k + 1)
    for t, n, what in ((hlen, n_seq, "hlen"), (slots, n_seq, "slots"), (d_tokens, 2 * n_seq, "d_tokens"),
                       (d_pos, 2 * n_seq, "d_pos"), (d_slot, 2 * n_seq, "d_slot"), (tokens, rows, "tokens"),
                       (pos, rows, "pos")):
        _chk(t, n, what)
    _chk(matched, n_seq, "matched", True)
    _chk(done, n_seq, "done", True)
    _chk(match_ctr, n_seq, "match_ctr", True)
    rc = _lib().lsa_spec_dm_begin(_p(hist), ld, _p(hlen), _p(slots), n_seq, int(k), int(max_seq), int(draft_max_seq),
                                  _p(d_tokens), _p(d_pos), _p(d_slot), _p(tokens), _p(pos), _p(matched), _p(done),
                                  _p(match_ctr), _stream())
    _status(rc, "lsa_spec_dm_begin")


def spec_dm_chain(amax: torch.Tensor, hlen: torch.Tensor, ld: int, k: int, j: int, max_seq: int, draft_max_seq: int,
                  tokens: torch.Tensor, d_tokens1: Optional[torch.Tensor] = None,
                  d_pos1: Optional[torch.Tensor] = None) -> None:
    """``lsa_spec_dm_chain`` on the current stream: iteration ``j``'s arg-max tokens into the
    target's rows ``j + 1`` and (``j + 1 < k``) into the draft engine's next 1-row input."""
    from .hip import _p, _stream
    n_seq = hlen.numel() if hlen is not None else 0
    last = j + 1 >= k
    _chk(hlen, max(n_seq, 1), "hlen")
    _chk(amax, n_seq, "amax")
    _chk(tokens, n_seq * (k + 1), "tokens")
    _chk(d_tokens1, n_seq, "d_tokens1", last)
    _chk(d_pos1, n_seq, "d_pos1", last)
    rc = _lib().lsa_spec_dm_chain(_p(amax), _p(hlen), int(ld), n_seq, int(k), int(j), int(max_seq), int(draft_max_seq),
                                  _p(tokens), _p(d_tokens1), _p(d_pos1), _stream())
    _status(rc, "lsa_spec_dm_chain")


__all__ = ["MAX_K", "MAX_NGRAM", "MAX_ROWS", "N_EOS", "check_shape", "check_draft_shape", "eos_array", "draft_reference",
           "accept_reference", "dm_begin_reference", "dm_chain_reference", "draft_model_reference", "spec_draft",
           "spec_accept", "spec_dm_begin", "spec_dm_chain"]
