"""Seeded temperature / top-k / top-p sampling: ctypes bindings of csrc/sampling/sampling.hip and
the fp64 reference of the same contract (the CPU implementation and the tests' oracle).

Contract per row (bf16 logits ``l[0..V)`` in a row of ``ld >= V`` columns, temperature ``T``,
``top_k`` (0 = off), ``top_p`` (1.0 = off), a 64-bit ``seed`` and a 32-bit counter ``c`` - the
absolute position the sampled token will occupy in its sequence):

1. columns ``>= V`` are never candidates;
2. ``T == 0``: greedy, the arg-max of ``l`` (lowest index on ties), filters ignored;
3. ``z = l / T``;
4. top-k (``0 < k < V``): keep ``z_i >=`` the k-th largest value (ties at the threshold kept);
5. top-p (``p < 1``): over the softmax of the survivors, ``z*`` = the largest value with
   ``mass{z_i >= z*} >= p``; keep ``z_i >= z*``;
6. ``token = argmax over kept i of z_i + g_i`` (lowest index on exact ties) with
   ``g_i = -log(-log(u_i))``, ``u_i = ((x_i >> 9) + 0.5) * 2^-23`` and ``x_i`` = word ``i & 3`` of
   ``Philox4x32-10(counter = (i >> 2, c, 0, 0), key = (seed_lo, seed_hi))``.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_M32 = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------ reference
def philox4x32_10(ctr, key) -> np.ndarray:
    """Philox4x32-10 (numpy). ``ctr``: four uint32 words (scalars or arrays that broadcast),
    ``key``: two uint32 words. Returns uint32 ``[..., 4]``."""
    c = [np.asarray(x, dtype=np.uint64) & _M32 for x in ctr]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(PHILOX_M0) * c[0]
        p1 = np.uint64(PHILOX_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _M32,
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _M32]
        k0 = (k0 + PHILOX_W0) & 0xFFFFFFFF
        k1 = (k1 + PHILOX_W1) & 0xFFFFFFFF
    return np.stack(c, axis=-1).astype(np.uint32)


def noise_bits(seed: int, ctr: int, idx) -> np.ndarray:
    """The 32-bit Philox word ``x_i`` of every vocabulary index in ``idx``."""
    idx = np.asarray(idx, dtype=np.int64)
    blocks, inv = np.unique(idx >> 2, return_inverse=True)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = philox4x32_10((blocks, int(ctr) & 0xFFFFFFFF, 0, 0), (seed & 0xFFFFFFFF, seed >> 32))
    return w[inv.reshape(idx.shape), idx & 3]


def gumbel_from_bits(x) -> np.ndarray:
    """``g = -log(-log(u))``, ``u = ((x >> 9) + 0.5) * 2^-23``, in fp64."""
    u = ((np.asarray(x, dtype=np.uint32) >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    return -np.log(-np.log(u))


def key16(raw) -> np.ndarray:
    """Order-preserving 16-bit key of bf16 bit patterns (the kernel's threshold domain): larger
    value -> larger key; -0 counts as +0."""
    raw = np.asarray(raw).astype(np.int64) & 0xFFFF
    raw = np.where(raw == 0x8000, 0, raw)
    return np.where(raw & 0x8000, ~raw & 0xFFFF, raw | 0x8000).astype(np.int64)


def bf16_bits(t: torch.Tensor) -> np.ndarray:
    """bf16 tensor -> its uint16 bit patterns (numpy, same shape)."""
    return t.detach().to(torch.bfloat16).contiguous().cpu().view(torch.int16).numpy().view(np.uint16)


def _as_f64_logits(logits, V: int) -> np.ndarray:
    if isinstance(logits, torch.Tensor):
        logits = logits.detach().cpu()[..., :V].to(torch.float64).numpy()
    a = np.asarray(logits, dtype=np.float64)
    if a.ndim == 1:
        a = a[None]
    return a[:, :V]


def _per_row(x, rows: int, dtype) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().tolist()
    if dtype is object:  # 64-bit seeds stay Python ints: numpy turns a list that mixes values below
        x = x.tolist() if isinstance(x, np.ndarray) else x  # and above 2^63 into float64
        x = [int(v) for v in (x if isinstance(x, (list, tuple)) else [x])]
    a = np.asarray(x, dtype=dtype if dtype is object else None).reshape(-1)
    if a.size == 1 and rows > 1:
        a = np.repeat(a, rows)
    if a.size != rows:
        raise ValueError(f"per-row sampling argument has {a.size} entries for {rows} rows")
    return a.astype(dtype)


def sample_reference(logits, V: int, T, top_k, top_p, seed, ctr):
    """The sampling contract in numpy fp64. ``logits``: [rows, >= V] (torch or numpy; values are
    taken as given, pass bf16-rounded values to mirror the device); ``T``, ``top_k``, ``top_p``,
    ``seed``, ``ctr``: per row (or one value for all rows).

    Returns ``(tokens int64 [rows], kept bool [rows, V], gap fp64 [rows], p_margin fp64 [rows])``:
    ``gap`` is the distance between the two best perturbed scores of the row (the two largest
    logits on a greedy row; inf with one candidate), ``p_margin`` the distance of ``p`` from the
    nearer of the two cumulative masses around the top-p boundary (inf with top-p off)."""
    L = _as_f64_logits(logits, V)
    rows = L.shape[0]
    T = _per_row(T, rows, np.float32).astype(np.float64)  # the device holds T and p as fp32
    top_k = _per_row(top_k, rows, np.int64)
    top_p = _per_row(top_p, rows, np.float32).astype(np.float64)
    seed = _per_row(seed, rows, object)
    ctr = _per_row(ctr, rows, np.int64)
    tokens = np.zeros(rows, dtype=np.int64)
    kept_all = np.zeros((rows, V), dtype=bool)
    gap = np.full(rows, np.inf)
    pm = np.full(rows, np.inf)

    def top2_gap(v):
        if v.size < 2:
            return np.inf
        t = np.partition(v, v.size - 2)[-2:]
        return float(t[1] - t[0])

    for r in range(rows):
        l = L[r]
        if not T[r] > 0:
            tokens[r] = int(np.argmax(l))
            kept_all[r, tokens[r]] = True
            gap[r] = top2_gap(l)
            continue
        z = l / T[r]
        kept = np.ones(V, dtype=bool)
        k = int(top_k[r])
        if 0 < k < V:
            kept = z >= np.partition(z, V - k)[V - k]
        p = float(top_p[r])
        if p < 1.0:
            zs = z[kept]
            w = np.exp(zs - zs.max())
            vals, inv = np.unique(zs, return_inverse=True)  # ascending
            gm = np.bincount(inv, weights=w, minlength=vals.size)[::-1]  # group masses, descending value
            cum = np.cumsum(gm) / gm.sum()
            j = int(np.searchsorted(cum, p, side="left"))  # first group with cum >= p
            j = min(j, vals.size - 1)
            kept &= z >= vals[::-1][j]
            pm[r] = min(abs(cum[j] - p), abs(p - cum[j - 1]) if j > 0 else np.inf)
        idx = np.nonzero(kept)[0]
        score = z[idx] + gumbel_from_bits(noise_bits(seed[r], int(ctr[r]), idx))
        tokens[r] = int(idx[np.argmax(score)])  # idx ascending: first maximum = lowest index
        kept_all[r] = kept
        gap[r] = top2_gap(score)
    return tokens, kept_all, gap, pm


# ------------------------------------------------------------------------------ HIP bindings
_declared = None


def _lib() -> ctypes.CDLL:
    """The kernel library (``hip.lib()``) with the two sampling entry points declared."""
    global _declared
    from . import hip
    L = hip.lib()
    if _declared is not L:
        vp, i, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
        if not hasattr(L, "lsa_sample"):
            raise RuntimeError("the kernel library has no lsa_sample: rebuild it (python csrc/build.py)")
        L.lsa_sample.argtypes = [vp, ll, i, i, vp, vp, vp, vp, vp, i, vp, vp, vp]
        L.lsa_sample.restype = i
        L.lsa_sample_noise.argtypes = [ctypes.c_ulonglong, ctypes.c_uint, ctypes.c_uint, i, vp, vp, vp, vp]
        L.lsa_sample_noise.restype = i
        _declared = L
    return L


def _chk(t: Optional[torch.Tensor], dtype, n: int, what: str) -> None:
    from .hip import _req
    _req(t is not None and t.is_cuda and t.dtype == dtype and t.is_contiguous() and t.numel() >= n,
         f"sample: {what} must be a contiguous cuda {dtype} tensor of >= {n} entries")


def sample(logits: torch.Tensor, V: int, rows: int, temperature: torch.Tensor, top_k: torch.Tensor,
           top_p: torch.Tensor, seed: torch.Tensor, ctr: torch.Tensor, keys_out: torch.Tensor, ctr_add: int = 0,
           dbg: Optional[torch.Tensor] = None) -> None:
    """``lsa_sample``: one token per row of bf16 ``logits`` [>= rows, ld >= V], written to
    ``keys_out`` (int64) as a common.h ``argmax_key`` for ``hip.argmax_finalize``. Per-row device
    arrays: ``temperature`` / ``top_p`` fp32, ``top_k`` / ``ctr`` int32, ``seed`` int64 (the
    64-bit pattern); the row's Philox counter is ``ctr[r] + ctr_add``. ``dbg``: optional int32
    [rows, 2] receiving (16-bit threshold key, kept count). No host reads: graph-capturable."""
    from .hip import _check, _p, _req, _stream
    _req(logits.is_cuda and logits.dtype == torch.bfloat16 and logits.dim() == 2 and logits.stride(1) == 1,
         "sample: logits must be a row-major bf16 cuda matrix")
    _req(1 <= rows <= logits.shape[0] and 1 <= V <= logits.shape[1] and rows <= 65535,
         f"sample: rows={rows}, V={V} outside logits {tuple(logits.shape)}")
    _req(rows == 1 or logits.stride(0) >= V, "sample: row stride below V")
    _chk(temperature, torch.float32, rows, "temperature")
    _chk(top_p, torch.float32, rows, "top_p")
    _chk(top_k, torch.int32, rows, "top_k")
    _chk(ctr, torch.int32, rows, "ctr")
    _chk(seed, torch.int64, rows, "seed")
    _chk(keys_out, torch.int64, rows, "keys_out")
    if dbg is not None:
        _chk(dbg, torch.int32, 2 * rows, "dbg")
    ld = logits.stride(0) if rows > 1 else max(logits.stride(0), V)
    rc = _lib().lsa_sample(_p(logits), ld, V, rows, _p(temperature), _p(top_k), _p(top_p), _p(seed), _p(ctr),
                           int(ctr_add), _p(keys_out), _p(dbg), _stream())
    _check(rc, "lsa_sample")


def sample_noise(seed: int, ctr: int, idx0: int, n: int, device, bits_in: Optional[torch.Tensor] = None):
    """``lsa_sample_noise``: (Philox words int32 [n], Gumbel values fp32 [n]) of the vocabulary
    indices ``idx0 .. idx0 + n``; with ``bits_in`` (int32 [n], the 32-bit patterns) the Gumbel
    values of those words instead."""
    from .hip import _check, _p, _req, _stream
    _req(n >= 1, "sample_noise: n >= 1")
    if bits_in is not None:
        _req(bits_in.is_cuda and bits_in.dtype == torch.int32 and bits_in.is_contiguous() and bits_in.numel() >= n,
             "sample_noise: bits_in must be a contiguous cuda int32 tensor of >= n words")
        device = bits_in.device
    with torch.cuda.device(device):
        bits = torch.empty(n, dtype=torch.int32, device=device)
        g = torch.empty(n, dtype=torch.float32, device=device)
        rc = _lib().lsa_sample_noise(int(seed) & 0xFFFFFFFFFFFFFFFF, int(ctr) & 0xFFFFFFFF, int(idx0) & 0xFFFFFFFF,
                                     n, _p(bits_in), _p(bits), _p(g), _stream())
    _check(rc, "lsa_sample_noise")
    return bits, g


def seed_to_i64(seed: int) -> int:
    """A 64-bit seed as the signed value an int64 tensor stores."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed - (1 << 64) if seed >= (1 << 63) else seed


__all__ = ["philox4x32_10", "noise_bits", "gumbel_from_bits", "key16", "bf16_bits", "sample_reference", "sample",
           "sample_noise", "seed_to_i64"]
