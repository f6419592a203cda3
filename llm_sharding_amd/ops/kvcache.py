"""KV-cache fork: the ctypes binding of csrc/cache/kv_fork.hip, the plain-torch reference of the
same contract (what CPU engines run and the tests' oracle) and the engine-level helper.

A sequence's K/V live in ``k_cache[layer][slot, head, 0:len, :]``. Under causal attention the K/V
of positions ``< j`` depend only on tokens ``< j``, so a prefix computed once in one slot can be
copied into another slot and the prefill continued there from position ``j``.

Contract. ``k_cache`` / ``v_cache``: lists of tensors (one per layer), each a contiguous
``[n_slots, nkv, t_max, hd]``. ``jobs``: a list of ``(src, len, dst_0, .., dst_{f-1})`` (or
``(src, len, [dst, ..])``) with ``1 <= f <= 8``. For every tensor, head and destination ``d`` the
``len * hd`` elements of ``[src, h, 0:len, :]`` are copied bit for bit to ``[d, h, 0:len, :]``;
nothing else is written. ``len == 0`` is a no-op. Refused (``ValueError``): a slot index out of
range, ``len`` outside ``[0, t_max]``, a destination equal to its source, a slot that is a
destination twice in one call, a slot that is both a source and a destination in one call.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple

import torch

MAX_FANOUT = 8
JOB_INTS = 3 + MAX_FANOUT  # [src, len, f, dst_0 .. dst_7], as csrc/cache/kv_fork.hip reads them

# lsa_kv_fork flags: bit 0 = non-temporal loads, bit 1 = non-temporal stores. Measured
# (profiles/kv_fork.md, scripts/bench_prefix.py): with both hints the copy is 7 - 15 % faster from
# 134 MB up, and a 2048-token Llama-2-7B fork (2.1 GB) plus the suffix prefill that reads the
# destination next is 0.09 ms faster; below a few hundred MB fork + suffix is the same within the
# spread or a few us slower with them (the plain stores leave the destination in the 256 MB
# Infinity Cache for the attention launch that follows). So a call that moves at least NT_MIN_BYTES
# (read + write) takes the hints and a smaller one does not.
NT_LOADS, NT_STORES = 1, 2
NT_MIN_BYTES = 512 << 20


def default_flags(nbytes: int) -> int:
    """The measured variant for a call that reads + writes ``nbytes``."""
    return NT_LOADS | NT_STORES if nbytes >= NT_MIN_BYTES else 0


def normalize_jobs(jobs, n_slots: int, t_max: int) -> List[Tuple[int, int, Tuple[int, ...]]]:
    """Validate ``jobs`` by the contract's rules; returns ``[(src, len, (dst, ..)), ..]``."""
    out = []
    role = {}  # slot -> "src" | "dst"
    for job in jobs:
        job = tuple(job)
        if len(job) < 3:
            raise ValueError(f"kv_fork: job {job} names no destination")
        src, length = int(job[0]), int(job[1])
        dsts = job[2] if len(job) == 3 and isinstance(job[2], (list, tuple)) else job[2:]
        dsts = tuple(int(d) for d in dsts)
        if not 1 <= len(dsts) <= MAX_FANOUT:
            raise ValueError(f"kv_fork: a job has 1..{MAX_FANOUT} destinations, got {len(dsts)}")
        if not 0 <= src < n_slots:
            raise ValueError(f"kv_fork: source slot {src} outside [0, {n_slots})")
        if not 0 <= length <= t_max:
            raise ValueError(f"kv_fork: len {length} outside [0, {t_max}]")
        if role.get(src) == "dst":
            raise ValueError(f"kv_fork: slot {src} is both a source and a destination")
        role[src] = "src"
        for d in dsts:
            if not 0 <= d < n_slots:
                raise ValueError(f"kv_fork: destination slot {d} outside [0, {n_slots})")
            if d == src:
                raise ValueError(f"kv_fork: destination {d} equals its source")
            if role.get(d) == "dst":
                raise ValueError(f"kv_fork: slot {d} is a destination twice")
            if role.get(d) == "src":
                raise ValueError(f"kv_fork: slot {d} is both a source and a destination")
            role[d] = "dst"
        out.append((src, length, dsts))
    return out


def _tensors(k_cache, v_cache) -> list:
    ks = [k_cache] if isinstance(k_cache, torch.Tensor) else list(k_cache)
    vs = [v_cache] if isinstance(v_cache, torch.Tensor) else list(v_cache)
    ts = ks + vs
    if not ts:
        raise ValueError("kv_fork: no cache tensors")
    shape, dt, dev = ts[0].shape, ts[0].dtype, ts[0].device
    if len(shape) != 4:
        raise ValueError("kv_fork: cache tensors are [n_slots, nkv, t_max, hd]")
    for t in ts:
        if t.shape != shape or t.dtype != dt or t.device != dev or not t.is_contiguous():
            raise ValueError("kv_fork: cache tensors must be contiguous and agree in shape, dtype and device")
    return ts


def kv_fork_reference(k_cache, v_cache, jobs) -> None:
    """The contract in plain torch slicing, in place (any device and dtype)."""
    ts = _tensors(k_cache, v_cache)
    n_slots, _, t_max, _ = ts[0].shape
    for src, length, dsts in normalize_jobs(jobs, n_slots, t_max):
        if length == 0:
            continue
        for t in ts:
            for d in dsts:
                t[d, :, :length, :] = t[src, :, :length, :]


# ------------------------------------------------------------------------------ HIP binding
_declared = None


def _lib() -> ctypes.CDLL:
    """The kernel library (``hip.lib()``) with the fork entry points declared."""
    global _declared
    from . import hip
    L = hip.lib()
    if _declared is not L:
        vp, i, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
        if not hasattr(L, "lsa_kv_fork"):
            raise RuntimeError("the kernel library has no lsa_kv_fork: rebuild it (python csrc/build.py)")
        L.lsa_kv_fork.argtypes = [vp, i, vp, i, i, i, i, i, i, vp]
        L.lsa_kv_fork.restype = i
        L.lsa_kv_fork_calls.argtypes = []
        L.lsa_kv_fork_calls.restype = ll
        _declared = L
    return L


def kv_fork_calls() -> int:
    """How many ``lsa_kv_fork`` launches this process has enqueued."""
    return int(_lib().lsa_kv_fork_calls())


def kv_fork_raw(ptrs: Sequence[int], jobs_flat: Sequence[int], n_jobs: int, n_slots: int, nkv: int, t_max: int,
                hd: int, flags: int = 0) -> int:
    """``lsa_kv_fork`` without the Python validation: returns the launcher's status code (the
    tests call the kernel's own host-side checks through this)."""
    from .hip import _stream
    pa = (ctypes.c_void_p * len(ptrs))(*ptrs)
    ja = (ctypes.c_int * max(1, len(jobs_flat)))(*jobs_flat)
    return int(_lib().lsa_kv_fork(pa, len(ptrs), ja, n_jobs, n_slots, nkv, t_max, hd, flags, _stream()))


def flatten_jobs(jobs) -> list:
    flat = []
    for src, length, dsts in jobs:
        flat += [src, length, len(dsts), *dsts, *([0] * (MAX_FANOUT - len(dsts)))]
    return flat


def kv_fork(k_cache, v_cache, jobs, flags: Optional[int] = None) -> None:
    """``lsa_kv_fork`` on the current stream: bf16 cuda caches, one launch for all tensors, heads
    and jobs; ``flags=None`` takes :func:`default_flags` of the call's bytes. The pointer table and
    the jobs travel in the kernel arguments (no host-to-device copy, nothing the host may not reuse
    when the call returns)."""
    from .hip import _check
    ts = _tensors(k_cache, v_cache)
    if not (ts[0].is_cuda and ts[0].dtype == torch.bfloat16):
        raise ValueError("kv_fork: the HIP kernel takes bf16 cuda caches (kv_fork_reference runs everything else)")
    n_slots, nkv, t_max, hd = ts[0].shape
    if hd % 8:
        raise ValueError(f"kv_fork: head_dim {hd} is no multiple of 8")
    norm = normalize_jobs(jobs, n_slots, t_max)
    if not norm:
        return
    if flags is None:
        flags = default_flags(len(ts) * nkv * hd * 2 * sum(n * (1 + len(d)) for _, n, d in norm))
    rc = kv_fork_raw([t.data_ptr() for t in ts], flatten_jobs(norm), len(norm), n_slots, nkv, t_max, hd, flags)
    _check(rc, "lsa_kv_fork")


# ------------------------------------------------------------------------------ engine level
def fork_jobs(eng, jobs) -> None:
    """Run fork ``jobs`` over every layer of ``eng`` (the HIP kernel on a GPU engine, the reference
    elsewhere) and set the destinations' host-side lengths."""
    if getattr(eng, "kv8", False):
        raise NotImplementedError("KV fork on an fp8 KV cache: the fork kernel copies bf16 tensors")
    if getattr(eng, "paged", False):
        raise NotImplementedError("KV fork on a paged KV cache: the fork kernel copies static tensors")
    if not eng.k_cache:
        return
    n_slots, _, t_max, _ = eng.k_cache[0].shape
    norm = normalize_jobs(jobs, n_slots, t_max)
    if eng.gpu:
        kv_fork(eng.k_cache, eng.v_cache, norm)
    else:
        kv_fork_reference(eng.k_cache, eng.v_cache, norm)
    for _, length, dsts in norm:
        for d in dsts:
            eng.seq_len[d] = length


def fork_slots(eng, src: int, dsts, length: int) -> None:
    """Copy the first ``length`` positions of slot ``src`` into every slot of ``dsts`` on all of
    the engine's layers; ``eng.seq_len[d] = length`` afterwards."""
    dsts = [int(d) for d in dsts]
    fork_jobs(eng, [(src, length, dsts[i:i + MAX_FANOUT]) for i in range(0, len(dsts), MAX_FANOUT)])


__all__ = ["MAX_FANOUT", "NT_LOADS", "NT_STORES", "NT_MIN_BYTES", "default_flags", "normalize_jobs", "kv_fork_reference", "kv_fork",
           "kv_fork_raw", "kv_fork_calls", "flatten_jobs", "fork_jobs", "fork_slots"]
