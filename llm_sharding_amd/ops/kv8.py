"""FP8 KV cache (kv_dtype="fp8"): the format, its torch references and the bindings of
csrc/cache/kv8.hip.

A layer's cache is four tensors: ``k8`` / ``v8`` uint8 ``[slots, n_kv, max_seq, hd]`` holding OCP
e4m3fn codes and ``ks`` / ``vs`` fp32 ``[slots, n_kv, max_seq]``, one scale per cached vector (the
``hd`` values of one (slot, kv-head, position), K and V separately). For a vector ``x`` of finite
bf16 values:

1. ``a = max |x_d|`` (exact);
2. ``a == 0``: ``s = 1``; else ``e = floor(log2 a)`` read from the fp32 exponent field of ``a``,
   clamped below to -119 (biased 8) so that ``s`` and ``1 / s`` are fp32 normals, ``s = 2 ** (e - 7)``;
3. ``code_d = e4m3_rne(fp32(x_d) * (1 / s))``.

The product is exact, the conversion is the only rounding; ``|x_d / s| < 256`` and a code rounds up
to 256 at most, so nothing saturates and the NaN code never appears. Dequantisation is
``bf16(code_d * s)``, exact wherever the product is a bf16 normal. (One corner overflows: a vector
whose maximum is at least 248 * 2^120 - the top sixteenth of bf16's last octave - rounds to the code
256 at scale 2^120 and reads back as infinity. Activations are some 36 orders of magnitude below.)
Power-of-two scales cost a floating-point format no relative precision and make the kernel and
these references comparable bit for bit.

This module stands beside ops/hip.py rather than inside it, as ops/int4.py does: hip.py is a
recorded input of the bf16 decode path's full-depth fixture (tests/fixture_hash.py)."""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import hip

KV8_MIN_EXP = 8          # smallest biased fp32 exponent of a vector maximum that sets the scale
KV8_SCALE_SHIFT = 7      # s = 2 ** (e - 7): the largest |code| of a non-zero vector lies in [128, 256]
KV8_HEAD_DIMS = (64, 128)
KV8_GROUPS = (1, 2, 3, 4, 6, 8)  # GQA group sizes the decode attention is built for
KV8_MAX_SPLIT = 16


def kv8_token_bytes(n_kv: int, hd: int) -> int:
    """Bytes one cached token costs per layer: K and V codes plus their two fp32 scales."""
    return n_kv * (2 * hd + 8)


# ------------------------------------------------------------------------------ references (any device)
def quantize_reference(x: torch.Tensor) -> tuple:
    """``x`` bf16 [..., hd] (finite) -> (codes uint8 [..., hd], scale fp32 [...]): the contract
    above in torch (``torch.float8_e4m3fn``'s cast is round-to-nearest-even)."""
    if x.dtype != torch.bfloat16:
        raise ValueError(f"quantize_reference takes bf16 vectors, got {x.dtype}")
    xf = x.float()
    a = xf.abs().amax(dim=-1)
    if not bool(torch.isfinite(a).all()):
        raise ValueError("quantize_reference: non-finite values")
    e = (a.contiguous().view(torch.int32) >> 23).clamp(min=KV8_MIN_EXP) - KV8_SCALE_SHIFT
    e = torch.where(a == 0, torch.full_like(e, 127), e)
    s = (e << 23).view(torch.float32)
    inv = ((254 - e) << 23).view(torch.float32)
    codes = (xf * inv[..., None]).to(torch.float8_e4m3fn).view(torch.uint8)
    return codes, s


def dequantize_reference(codes: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """bf16 [..., hd] = bf16(code * s): one fp32 multiply, one rounding."""
    if codes.dtype != torch.uint8 or scale.dtype != torch.float32 or tuple(codes.shape[:-1]) != tuple(scale.shape):
        raise ValueError("dequantize_reference: codes uint8 [..., hd], scale fp32 [...]")
    return (codes.view(torch.float8_e4m3fn).float() * scale[..., None]).to(torch.bfloat16)


def attn_decode_reference(q: torch.Tensor, k8: torch.Tensor, v8: torch.Tensor, ks: torch.Tensor, vs: torch.Tensor,
                          slot, lens, n_heads: int, scale: Optional[float] = None) -> torch.Tensor:
    """fp64 softmax attention of row r over keys [0, lens[r]) of slot[r] of the DEQUANTISED cache:
    [rows, n_heads * hd]. ``q`` [rows, >= n_heads * hd]."""
    n_kv, hd = k8.shape[1], k8.shape[3]
    g = n_heads // n_kv
    slot = [int(s) for s in (slot.tolist() if torch.is_tensor(slot) else slot)]
    lens = [int(t) for t in (lens.tolist() if torch.is_tensor(lens) else lens)]
    sc = hd ** -0.5 if scale is None else scale
    out = torch.zeros(len(slot), n_heads, hd, dtype=torch.float64, device=q.device)
    for r, (s, T) in enumerate(zip(slot, lens)):
        k = dequantize_reference(k8[s, :, :T], ks[s, :, :T]).double().repeat_interleave(g, 0)  # [nh, T, hd]
        v = dequantize_reference(v8[s, :, :T], vs[s, :, :T]).double().repeat_interleave(g, 0)
        w = torch.einsum("hd,htd->ht", q[r, :n_heads * hd].double().view(n_heads, hd), k) * sc
        out[r] = torch.einsum("ht,htd->hd", torch.softmax(w, -1), v)
    return out.reshape(len(slot), n_heads * hd)


# ------------------------------------------------------------------------------ bindings
_L = None


def _lib():
    """The kernel library with the kv8 entry points' signatures declared."""
    global _L
    if _L is None:
        L = hip.lib()
        if not hasattr(L, "lsa_attn_decode_kv8"):
            raise RuntimeError("the kernel library has no lsa_attn_decode_kv8: rebuild it (python csrc/build.py)")
        vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
        L.lsa_attn_decode_kv8.argtypes = [vp, i, vp, vp, vp, vp, vp, vp, vp, i, i, i, i, i, f, i, i, vp, vp, vp, i, vp, vp]
        L.lsa_kv8_append.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i, i, i, i, i, vp]
        L.lsa_kv8_dequant.argtypes = [vp, vp, vp, vp, vp, vp, vp, i, i, i, i, i, vp]
        L.lsa_attn_kv8_kpi.argtypes = [i]
        for name in ("lsa_attn_decode_kv8", "lsa_kv8_append", "lsa_kv8_dequant", "lsa_attn_kv8_kpi"):
            getattr(L, name).restype = i
        _L = L
    return _L


def _check_cache(k8, v8, ks, vs, what: str) -> tuple:
    hip._req(all(t.is_cuda and t.is_contiguous() for t in (k8, v8, ks, vs)), f"{what}: contiguous cuda cache tensors")
    hip._req(k8.dtype == torch.uint8 and v8.dtype == torch.uint8 and k8.dim() == 4 and k8.shape == v8.shape,
             f"{what}: k8 / v8 uint8 [slots, n_kv, T, hd]")
    hip._req(ks.dtype == torch.float32 and vs.dtype == torch.float32 and tuple(ks.shape) == tuple(k8.shape[:3])
             and tuple(vs.shape) == tuple(k8.shape[:3]), f"{what}: ks / vs fp32 [slots, n_kv, T]")
    hip._req(k8.shape[3] in KV8_HEAD_DIMS, f"{what}: head_dim {k8.shape[3]} not built (64 / 128)")
    return tuple(k8.shape)


def _check_stage(k_stage, v_stage, shape: tuple, what: str) -> None:
    hip._req(hip._is_bf16_cuda(k_stage, v_stage) and k_stage.is_contiguous() and v_stage.is_contiguous(),
             f"{what}: contiguous bf16 cuda staging tensors")
    hip._req(tuple(k_stage.shape) == shape and tuple(v_stage.shape) == shape,
             f"{what}: the staging layer has the cache's shape {shape}")


def kv8_append(k_stage: torch.Tensor, v_stage: torch.Tensor, k8: torch.Tensor, v8: torch.Tensor, ks: torch.Tensor,
               vs: torch.Tensor, slot: torch.Tensor, pos: torch.Tensor, rows: int) -> None:
    """Quantise the K / V vectors at (slot[m], h, pos[m], :) of the bf16 staging layer into the fp8
    tensors at the same cell, m < rows. A row with pos outside [0, max_seq) writes nothing. The
    rows of one call name distinct cells. ``slot`` / ``pos`` are read on the device (capturable)."""
    shape = _check_cache(k8, v8, ks, vs, "kv8_append")
    _check_stage(k_stage, v_stage, shape, "kv8_append")
    hip._req(slot.is_cuda and pos.is_cuda and slot.dtype == torch.int32 and pos.dtype == torch.int32,
             "kv8_append: int32 cuda slot/pos")
    hip._req(1 <= rows <= slot.numel() and rows <= pos.numel(), "kv8_append: rows")
    rc = _lib().lsa_kv8_append(hip._p(k_stage), hip._p(v_stage), hip._p(k8), hip._p(v8), hip._p(ks), hip._p(vs),
                               hip._p(slot), hip._p(pos), rows, shape[0], shape[1], shape[3], shape[2], hip._stream())
    hip._check(rc, "lsa_kv8_append")


def kv8_dequant(k8: torch.Tensor, v8: torch.Tensor, ks: torch.Tensor, vs: torch.Tensor, k_stage: torch.Tensor,
                v_stage: torch.Tensor, jobs) -> None:
    """``jobs``: host pairs (slot, len). Writes bf16(code * s) for positions [0, len) of every
    kv-head of those slots into the staging layer, nothing else."""
    shape = _check_cache(k8, v8, ks, vs, "kv8_dequant")
    _check_stage(k_stage, v_stage, shape, "kv8_dequant")
    jobs = [(int(s), int(n)) for s, n in jobs]
    for s, n in jobs:
        hip._req(0 <= s < shape[0] and 0 <= n <= shape[2], f"kv8_dequant: job {(s, n)} outside the cache {shape}")
    hip._req(len({s for s, _ in jobs}) == len(jobs), "kv8_dequant: a slot named twice")
    if not jobs:
        return
    arr = (ctypes.c_int * (2 * len(jobs)))(*[x for j in jobs for x in j])
    rc = _lib().lsa_kv8_dequant(hip._p(k8), hip._p(v8), hip._p(ks), hip._p(vs), hip._p(k_stage), hip._p(v_stage),
                                ctypes.cast(arr, ctypes.c_void_p), len(jobs), shape[0], shape[1], shape[3], shape[2],
                                hip._stream())
    hip._check(rc, "lsa_kv8_dequant")


def attn_kv8(q: torch.Tensor, k8: torch.Tensor, v8: torch.Tensor, ks: torch.Tensor, vs: torch.Tensor,
             slot: torch.Tensor, pos: torch.Tensor, rows: int, n_heads: int, n_kv: int, head_dim: int, nsplit: int,
             part_o: Optional[torch.Tensor], part_lse: Optional[torch.Tensor], out: torch.Tensor,
             kv_len: Optional[torch.Tensor] = None, min_chunk: int = 64, scale: Optional[float] = None,
             counters: Optional[torch.Tensor] = None) -> None:
    """:func:`hip.attn` over an fp8 cache (csrc/cache/kv8.hip): same arguments and semantics, with
    (k8, v8, ks, vs) in place of the bf16 caches. ``counters``: >= rows * n_kv zeroed int32, left
    zeroed (default: the stream's coop workspace); the partial buffers are needed for nsplit > 1."""
    shape = _check_cache(k8, v8, ks, vs, "attn_kv8")
    hip._req(hip._is_bf16_cuda(q, out), "attn_kv8: bf16 cuda q / out")
    hip._req(shape[1] == n_kv and shape[3] == head_dim, "attn_kv8: cache dims")
    hip._req(n_kv >= 1 and n_heads % n_kv == 0 and (n_heads // n_kv) in KV8_GROUPS,
             f"attn_kv8: GQA group {n_heads}/{n_kv} not built {KV8_GROUPS}")
    hip._req(rows >= 1 and q.dim() == 2 and q.shape[0] >= rows and q.shape[1] >= n_heads * head_dim
             and q.stride(1) == 1 and q.stride(0) % 8 == 0, "attn_kv8: q shape")
    hip._req(out.dim() == 2 and out.shape[0] >= rows and out.shape[1] >= n_heads * head_dim and out.stride(1) == 1,
             "attn_kv8: out shape")
    hip._req(1 <= nsplit <= KV8_MAX_SPLIT and min_chunk >= 1, "attn_kv8: nsplit 1..16, min_chunk >= 1")
    hip._req(slot.is_cuda and pos.is_cuda and slot.dtype == torch.int32 and pos.dtype == torch.int32
             and slot.numel() >= rows and pos.numel() >= rows, "attn_kv8: int32 cuda slot/pos")
    hip._req(kv_len is None or (kv_len.is_cuda and kv_len.dtype == torch.int32 and kv_len.numel() >= rows),
             "attn_kv8: int32 cuda kv_len")
    if nsplit > 1:
        hip._req(part_o is not None and part_lse is not None and part_o.dtype == torch.float32
                 and part_lse.dtype == torch.float32 and part_o.numel() >= rows * n_heads * nsplit * head_dim
                 and part_lse.numel() >= rows * n_heads * nsplit, "attn_kv8: fp32 workspace too small")
        if counters is None:
            counters = hip.default_workspace(q.device).counters
        hip._req(counters.dtype == torch.int32 and counters.numel() >= rows * n_kv, "attn_kv8: counters too small")
    sc = head_dim ** -0.5 if scale is None else scale
    rc = _lib().lsa_attn_decode_kv8(hip._p(q), q.stride(0), hip._p(k8), hip._p(v8), hip._p(ks), hip._p(vs), hip._p(slot),
                                    hip._p(pos), hip._p(kv_len), rows, n_heads, n_kv, head_dim, shape[2], float(sc),
                                    nsplit, min_chunk, hip._p(part_o), hip._p(part_lse), hip._p(out), out.stride(0),
                                    hip._p(counters) if nsplit > 1 else None, hip._stream())
    hip._check(rc, "lsa_attn_decode_kv8")


attn = attn_kv8  # (the engine's call reads as hip.attn's: runtime/engine_kv8.py)


def attn_kv8_kpi(head_dim: int) -> int:
    """Keys per workgroup iteration of :func:`attn_kv8` for a head size: split chunks are rounded up
    to it (what tests/contract_cases.py ``split_chunk`` is for the bf16 kernel)."""
    k = _lib().lsa_attn_kv8_kpi(head_dim)
    if k < 1:
        raise ValueError(f"attn_kv8: no kernel for head_dim {head_dim}")
    return k


def split_chunk_kv8(T: int, nsplit: int, kpi: int, min_chunk: int = 64) -> int:
    """Keys per split: ceil(T / nsplit), at least ``min_chunk``, rounded up to ``kpi``."""
    chunk = max(-(-T // nsplit), min_chunk)
    return -(-chunk // kpi) * kpi
