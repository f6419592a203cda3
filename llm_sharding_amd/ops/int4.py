"""Int4 weights (W4A16): the symmetric group-128 format, its packed layout for the gfx950 decode
kernel (csrc/quant/gemv_int4.hip), the kernel's configs and its bindings.

The format is the ModelSharder's ``torch.int4`` one: ``w[n, k] ~= q[n, k] * scale[n, k // 128]``,
``|q| <= 7``, fp32 scales. On the device a projection is

* ``Wq4[nt][K/128][lane][16 B]`` (:func:`pack_b_int4`): one 16-byte load per lane holds the 32
  nibbles of the four consecutive 32-k MFMA B fragments of one scale group (dword h = fragment
  h, in ``packing.pack_b``'s element order), and
* ``S[nt][K/128][16]`` fp32 (:func:`pack_scales_int4`): a lane's fragments belong to one output
  column, so one scale covers the whole load.

This module stands beside ops/packing.py and ops/hip.py rather than inside them: those two, the
engine and csrc/kernels/ are the recorded inputs of the bf16 decode path's full-depth fixture
(tests/fixture_hash.py), which an added weight format leaves untouched."""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import hip
from .packing import N_CU, row_blocks

INT4_GROUP = 128  # k per scale group: fixed (one 16-B load per lane of the int4 kernel = one group)


def _check_int4_shape(N: int, K: int, what: str) -> None:
    if N % 16 or K % INT4_GROUP or K < INT4_GROUP:
        raise ValueError(f"{what} needs N%16==0 and K%{INT4_GROUP}==0, got {(N, K)}")


def quantize_int4_groups(w: torch.Tensor) -> tuple:
    """Symmetric group-128 int4: w[n, k] ~= q[n, k] * scale[n, k // 128]. Returns (q int8 [N, K]
    in [-7, 7], scale fp32 [N, K/128]): the ModelSharder's ``quantize_int4`` arithmetic at group
    128 (its nibbles unpacked), without its gcd fallback for narrow matrices."""
    from ..utils.model_sharder import dequantize_int4, quantize_int4
    N, K = w.shape
    if K % INT4_GROUP or K < INT4_GROUP:
        raise ValueError(f"int4 weights need K % {INT4_GROUP} == 0, got K={K}")
    packed, scale = quantize_int4(w, INT4_GROUP)
    q = dequantize_int4(packed, torch.ones_like(scale)).to(torch.int8)  # the signed nibbles
    return q, scale.float()


def dequantize_int4_groups(q: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """fp32 [N, K] = q * scale of its group: one fp32 multiply per weight."""
    N, K = q.shape
    return (q.float().view(N, K // INT4_GROUP, INT4_GROUP) * scale.float()[:, :, None]).reshape(N, K)


# nibble position (within a dword of 8) of fragment element j: the pair (2p, 2p + 1) sits at
# nibbles (p, p + 4), so that one rotate + one and-or of the dword gives the bf16 pair (csrc/quant/gemv_int4.hip)
_INT4_NIBBLE_POS = [0, 4, 1, 5, 2, 6, 3, 7]


def pack_b_int4(q: torch.Tensor) -> torch.Tensor:
    """int4 values [N, K] (int8 in [-7, 7], K % 128 == 0) -> uint8 [N*K/2] in the layout
    Wq4[nt][K/128][lane][16 B]: per lane and 16-B load the four dwords are the lane's 8 elements
    of MFMA B fragments 4g .. 4g+3 (pack_b's element order). Inside a dword: offset nibbles
    u = q + 8, element j at nibble ``_INT4_NIBBLE_POS[j]``, the dword rotated left by 3 bits."""
    N, K = q.shape
    _check_int4_shape(N, K, "pack_b_int4")
    if q.dtype != torch.int8 or int(q.abs().max()) > 7:
        raise ValueError("pack_b_int4 needs int8 values in [-7, 7]")
    sh = torch.tensor([4 * p for p in _INT4_NIBBLE_POS], dtype=torch.int64, device=q.device)
    out = torch.empty(N // 16, K // 128, 64, 16, dtype=torch.uint8, device=q.device)
    step = max(1, (1 << 20) // K)  # column tiles per pass: each int64 temporary stays at 128 MiB
    for t0 in range(0, N // 16, step):
        qt = q[16 * t0:16 * (t0 + step)]
        nt = qt.shape[0] // 16
        u = (qt.to(torch.int64).contiguous() + 8).view(nt, 16, K // 32, 4, 8).permute(0, 2, 3, 1, 4).reshape(nt, K // 32, 64, 8)
        d = (u << sh).sum(dim=-1)                            # [nt, kt, lane] dwords
        d = ((d << 3) | (d >> 29)) & 0xFFFFFFFF              # rotl 3
        d = d.view(nt, K // 128, 4, 64).permute(0, 1, 3, 2)  # [nt, g, lane, h]
        for i in range(4):                                   # little-endian bytes
            out[t0:t0 + nt].view(nt, K // 128, 64, 4, 4)[..., i] = ((d >> (8 * i)) & 0xFF).to(torch.uint8)
    return out.reshape(-1)


def unpack_b_int4(p: torch.Tensor, N: int, K: int) -> torch.Tensor:
    """Inverse of :func:`pack_b_int4`: int8 [N, K]."""
    _check_int4_shape(N, K, "unpack_b_int4")
    if p.dtype != torch.uint8 or p.numel() != N * K // 2:
        raise ValueError(f"unpack_b_int4: {N * K // 2} packed bytes expected")
    by = p.view(N // 16, K // 128, 64, 4, 4).to(torch.int64)
    d = sum(by[..., i] << (8 * i) for i in range(4))    # [nt, g, lane, h]
    d = ((d >> 3) | (d << 29)) & 0xFFFFFFFF              # rotr 3
    d = d.permute(0, 1, 3, 2).reshape(N // 16, K // 32, 64)
    u = torch.stack([(d >> (4 * pos)) & 0xF for pos in _INT4_NIBBLE_POS], dim=-1)  # [nt, kt, lane, j]
    q = (u - 8).to(torch.int8)
    return q.view(N // 16, K // 32, 4, 16, 8).permute(0, 3, 1, 2, 4).reshape(N, K).contiguous()


def pack_scales_int4(scale: torch.Tensor) -> torch.Tensor:
    """Group scales [N, K/128] -> fp32 S[nt][K/128][16], beside Wq4: the 16 columns of a tile
    and group are one 64-byte run."""
    N, G = scale.shape
    if N % 16:
        raise ValueError(f"pack_scales_int4 needs N%16==0, got N={N}")
    return scale.float().view(N // 16, 16, G).permute(0, 2, 1).contiguous()


def unpack_scales_int4(s: torch.Tensor) -> torch.Tensor:
    return s.permute(0, 2, 1).reshape(s.shape[0] * 16, s.shape[1]).contiguous()


def int4_bytes(n: int, k: int) -> int:
    """Bytes of an int4 projection: nibbles + fp32 group scales (4.25 bits per weight)."""
    return n * k // 2 + 4 * n * (k // INT4_GROUP)


# (tn, mb, nw, ug) instantiated in csrc/quant/gemv_int4.hip (LSA_INT4_CONFIGS) - keep in sync.
INT4_CONFIGS = [(1, 1, 4, 1), (1, 1, 8, 1), (1, 1, 4, 2), (1, 1, 8, 2), (2, 1, 4, 1), (2, 1, 8, 1), (2, 1, 4, 2),
                (4, 1, 4, 1), (1, 2, 4, 1), (1, 2, 8, 1), (2, 2, 4, 1), (2, 2, 8, 1), (1, 4, 4, 1), (1, 4, 8, 1),
                (2, 4, 4, 1), (2, 4, 8, 1)]
INT4_MAX_ROWS = 64  # rows the native int4 kernel serves; above, dequantise + the bf16 kernels


def int4_gemv_candidates(n_tiles: int, k: int, rows: int, need_even: bool = False) -> list:
    if rows > INT4_MAX_ROWS or k % INT4_GROUP:
        return []
    mb = row_blocks(rows)
    return [(tn, nw, ug) for (tn, b, nw, ug) in INT4_CONFIGS
            if b == mb and n_tiles % tn == 0 and (not need_even or tn % 2 == 0)]


def int4_config(n_tiles: int, rows: int, need_even: bool = False, k: int = 4096) -> tuple:
    """(tn, nw, ug) for the int4 GEMV (rows <= 64), by the rule of :func:`fp8_config`: at least
    256 workgroups where the shape allows, and under that the widest column tile (the activations
    and their row sums are shared by a workgroup's tiles); 8 waves when the grid is a single
    round of the 256 CUs, else 4; one scale group per chunk (two measured slower on every
    Llama-2-7B shape, profiles/int4.md)."""
    cands = int4_gemv_candidates(n_tiles, k, rows, need_even)
    if not cands:
        raise ValueError(f"no int4 GEMV config for {n_tiles} tiles, K={k}, rows={rows}")

    def cost(c):
        tn, nw, ug = c
        g = n_tiles // tn
        return (g < N_CU, -tn if g >= N_CU else tn, ug, nw != (8 if g <= N_CU else 4))
    return min(cands, key=cost)


# ------------------------------------------------------------------------------ bindings
_L = None


def _lib():
    """The kernel library with the int4 entry points' signatures declared."""
    global _L
    if _L is None:
        L = hip.lib()
        if not hasattr(L, "lsa_gemv_int4"):
            raise RuntimeError("the kernel library has no lsa_gemv_int4: rebuild it (python csrc/build.py)")
        vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
        L.lsa_gemv_int4.argtypes = [vp, i, vp, vp, vp, i, i, i, i, f, i, ctypes.POINTER(hip.EpiArgs), i, i, i, vp]
        L.lsa_dequant_int4_packed.argtypes = [vp, vp, vp, i, i, vp]
        L.lsa_gemv_int4.restype = L.lsa_dequant_int4_packed.restype = i
        _L = L
    return _L


def gemv_int4(x: torch.Tensor, wq4: torch.Tensor, scales: torch.Tensor, M: int, N: int, K: int, epi: int,
              ep: hip.EpiArgs, norm: bool = False, eps: float = 1e-5, a_rows: Optional[torch.Tensor] = None,
              cfg: Optional[tuple] = None) -> None:
    """W4A16 decode projection (csrc/quant/gemv_int4.hip), M <= 64: ``wq4`` = pack_b_int4(q) (uint8 [N*K/2]),
    ``scales`` = pack_scales_int4(scale) (fp32 [N*K/128]; the RMSNorm weight folded into W
    before quantisation). No arg-max epilogue: the lm_head stays bf16."""
    hip._req(1 <= M <= 64, f"gemv_int4 supports 1..64 rows, got {M}")
    hip._req(epi in (hip.EPI_STORE, hip.EPI_RESID, hip.EPI_SWIGLU, hip.EPI_QKV), f"gemv_int4: epilogue {epi} not built")
    hip._check_epi(epi, ep, N)
    hip._req(hip._is_bf16_cuda(x), "gemv_int4: bf16 cuda activations")
    hip._req(N >= 16 and N % 16 == 0 and K >= 128 and K % 128 == 0, "gemv_int4: N % 16, K % 128")
    hip._req(wq4.is_cuda and wq4.dtype == torch.uint8 and wq4.numel() == N * K // 2,
         "gemv_int4: packed int4 weights [N*K/2] uint8")
    hip._req(scales.is_cuda and scales.dtype == torch.float32 and scales.numel() == N * (K // 128)
         and scales.is_contiguous(), "gemv_int4: packed fp32 group scales [N*K/128]")
    hip._req(x.dim() == 2 and x.shape[1] >= K and x.stride(1) == 1, "gemv_int4: x must be [rows, >=K] row-major")
    if a_rows is None:
        hip._req(x.shape[0] >= M, "gemv_int4: x has fewer rows than M")
    else:
        hip._req(a_rows.dtype == torch.int32 and a_rows.is_cuda and a_rows.numel() >= M, "gemv_int4: a_rows")
    tn, nw, ug = cfg if cfg is not None else int4_config(N // 16, M, need_even=(epi == hip.EPI_SWIGLU), k=K)
    hip._req((tn, row_blocks(M), nw, ug) in INT4_CONFIGS, f"gemv_int4: config {(tn, nw, ug)} not built for {M} rows")
    hip._req((N // 16) % tn == 0, f"gemv_int4: N={N} is not a multiple of {16 * tn}")
    rc = _lib().lsa_gemv_int4(hip._p(x), x.stride(0), hip._p(a_rows), hip._p(wq4), hip._p(scales), M, N, K, int(norm), float(eps), epi,
                             ctypes.byref(ep), tn, nw, ug, hip._stream())
    hip._check(rc, "lsa_gemv_int4")


def dequant_int4_packed(wq4: torch.Tensor, scales: torch.Tensor, out: torch.Tensor, N: int, K: int) -> torch.Tensor:
    """Packed int4 (+ packed group scales) -> packed bf16 (pack_b layout) in ``out`` (>= N*K bf16)."""
    hip._req(N >= 16 and N % 16 == 0 and K >= 128 and K % 128 == 0, "dequant_int4: N % 16, K % 128")
    hip._req(wq4.is_cuda and wq4.dtype == torch.uint8 and wq4.numel() == N * K // 2, "dequant_int4: weights")
    hip._req(scales.is_cuda and scales.dtype == torch.float32 and scales.numel() == N * (K // 128)
         and scales.is_contiguous(), "dequant_int4: scales")
    hip._req(hip._is_bf16_cuda(out) and out.numel() >= N * K and out.is_contiguous(), "dequant_int4: out")
    hip._check(_lib().lsa_dequant_int4_packed(hip._p(wq4), hip._p(scales), hip._p(out), N, K, hip._stream()), "lsa_dequant_int4_packed")
    return out.view(-1)[:N * K].view(N // 16, K // 32, 64, 8)
