"""Int4 weights (W4A16): the symmetric group-128 format, its packed layout for the gfx950 decode
kernels, their configs and bindings, and the dispatcher between them (:func:`proj_int4`):
csrc/quant/gemv_int4.hip for 1..64 rows (every workgroup reads all of A) and the cooperative
csrc/quant/gemv_coop_int4.hip for 17..128 rows (a workgroup's waves share A through LDS, K split
over workgroups), and csrc/quant/gemm_int4.hip for prefill chunks and decode batches above 128 rows
(:func:`proj_gemm_int4`), all on the same operands with the same arithmetic.

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
import os
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


# (mb, tnw, nw, d) instantiated in csrc/quant/gemv_coop_int4.hip (LSA_INT4_COOP_CONFIGS) - keep in sync.
# nw waves of tnw 16-column tiles each share a workgroup's A chunks; d = register-ring depth.
INT4_COOP_CONFIGS = [(2, 1, 8, 4), (2, 1, 4, 4), (2, 2, 4, 4), (4, 1, 8, 4), (4, 1, 4, 4), (4, 2, 4, 3), (8, 1, 8, 3),
                     (8, 1, 4, 3)]
INT4_COOP_MIN_ROWS, INT4_COOP_MAX_ROWS = 17, 128  # rows the cooperative int4 kernel serves
INT4_COOP_SPLITS = (1, 2, 4, 8, 16)
INT4_COOP_SLAB_FLOATS = 1 << 24  # the smallest slab an engine's CoopWorkspace has (runtime/engine.py)


def int4_coop_slab_floats(n: int, rows: int, tnw: int, nw: int, sk: int) -> int:
    """fp32 workspace a cooperative int4 launch needs: sk partial tiles + partial sums of squares
    (0 when sk == 1)."""
    if sk <= 1:
        return 0
    mr = 16 * row_blocks(rows)
    return sk * n * mr + sk * (n // 16 // (tnw * nw)) * mr


def int4_coop_candidates(n_tiles: int, k: int, rows: int, need_even: bool = False) -> list:
    """(tnw, nw, d, sk) for the cooperative int4 GEMV (17..128 rows): the workgroup's nw * tnw
    tiles divide the tile count (need_even, SwiGLU: an even number of them), and every K split
    keeps at least one 128-k group."""
    if not INT4_COOP_MIN_ROWS <= rows <= INT4_COOP_MAX_ROWS or k % INT4_GROUP or k < INT4_GROUP:
        return []
    mb = row_blocks(rows)
    out = []
    for (b, tnw, nw, d) in INT4_COOP_CONFIGS:
        tg = tnw * nw
        if b != mb or n_tiles % tg or (need_even and tg % 2):
            continue
        out += [(tnw, nw, d, sk) for sk in INT4_COOP_SPLITS
                if sk <= k // INT4_GROUP and (n_tiles // tg) * sk <= 4 * N_CU]
    return out


INT4_COOP_MIN_GRID = 160   # workgroups from which a wider grid measured no faster than a lesser K split
INT4_COOP_MIN_CHUNKS = 8   # 128-k groups a K split keeps (shorter pipelines lost to their own ramp and epilogue)


def int4_coop_config(n_tiles: int, k: int, rows: int, need_even: bool = False,
                     slab_floats: int = INT4_COOP_SLAB_FLOATS, counters: Optional[int] = None) -> Optional[tuple]:
    """(tnw, nw, d, sk) or None when no built config divides the tile count (or fits a workspace
    of ``slab_floats`` floats and, if given, ``counters`` arrival counters). The rule that reproduces the winners of profiles/int4.md "Cooperative
    kernel": a grid of at least INT4_COOP_MIN_GRID workgroups whose K splits keep
    INT4_COOP_MIN_CHUNKS groups each (every split writes and re-reads an fp32 tile of all rows
    and pays the pipeline's ramp); among those the widest workgroup (A is staged once per column
    group), one tile per wave, the fewest splits. Where no config reaches that: the largest grid
    up to one workgroup per CU, then the fewest splits."""
    cands = [c for c in int4_coop_candidates(n_tiles, k, rows, need_even)
             if int4_coop_slab_floats(16 * n_tiles, rows, c[0], c[1], c[3]) <= slab_floats
             and (counters is None or n_tiles // (c[0] * c[1]) <= counters)]
    if not cands:
        return None

    def cost(c):
        tnw, nw, d, sk = c
        grid = n_tiles // (tnw * nw) * sk
        ok = grid >= INT4_COOP_MIN_GRID and (sk == 1 or k // INT4_GROUP // sk >= INT4_COOP_MIN_CHUNKS)
        return (not ok, 0 if ok else -min(grid, N_CU), -tnw * nw, -nw, sk)
    return min(cands, key=cost)


# Rows 17..64: the (N, K, row blocks) classes where the cooperative kernel measured faster than
# gemv_int4 by more than the two windows' spread, each with the table that measured it (2 row
# blocks: at 32 rows, 4: at 64 rows). Rows 65..128 always take the cooperative kernel: the
# alternative there is dequantise + bf16, which it beat on every measured shape.
_COOP_TABLE = 'profiles/int4.md "Cooperative kernel, Llama-2-7B shapes"'
INT4_COOP_ROUTE = {(n, k, mb): _COOP_TABLE
                   for n, k in ((12288, 4096), (4096, 4096), (22016, 4096), (4096, 11008)) for mb in (2, 4)}


# (bn, depth) instantiated in csrc/quant/gemm_int4.hip (lsa_gemm_int4) - keep in sync. 128-row x bn
# tiles, depth = groups in the A ring. bn 256 is not built: its accumulators, group partials and
# rings spilled (the kernel's header comment has the compiler's report).
INT4_GEMM_CONFIGS = [(128, 4)]
INT4_GEMM_SPLITS = (1, 2, 4, 8)
INT4_GEMM_ROWS = 128          # rows of an output tile
INT4_GEMM_MIN_GRID = 192      # workgroups from which a further K split measured no faster
INT4_GEMM_MIN_CHUNKS = 4      # 128-k groups a K split keeps: the depth of the A ring
# output tiles (ceil(M/128) * N/bn) up to which the native GEMM measured ahead of dequantise + bf16
# GEMM by more than the windows' spread: the o and down projections at 256 rows (64 tiles); from 128
# tiles on it was level or behind on every shape (profiles/int4.md "GEMM, Llama-2-7B shapes")
INT4_GEMM_MAX_TILES = 64


def _row_tiles(M: int) -> int:
    return -(-M // INT4_GEMM_ROWS)


def int4_gemm_slab_floats(M: int, N: int, sk: int) -> int:
    """fp32 workspace a split int4 GEMM launch needs: sk partial tiles of whole 128-row tiles
    (0 when sk == 1)."""
    return 0 if sk <= 1 else sk * _row_tiles(M) * INT4_GEMM_ROWS * N


def int4_gemm_candidates(M: int, N: int, K: int, epi: int = 0) -> list:
    """(bn, sk) the int4 GEMM can run: bn divides N, every K split keeps a 128-k group, the
    partial slab stays under 2 GiB."""
    if M < 1 or N < 1 or K < INT4_GROUP or K % INT4_GROUP or epi not in (hip.EPI_STORE, hip.EPI_RESID, hip.EPI_SWIGLU, hip.EPI_QKV):
        return []
    return [(bn, sk) for bn, _ in INT4_GEMM_CONFIGS if N % bn == 0 for sk in INT4_GEMM_SPLITS
            if sk <= K // INT4_GROUP and 4 * int4_gemm_slab_floats(M, N, sk) < 1 << 31]


def int4_gemm_config(M: int, N: int, K: int, epi: int = 0, slab_floats: int = INT4_COOP_SLAB_FLOATS,
                     counters: Optional[int] = None) -> Optional[tuple]:
    """(bn, sk) or None when no built tile divides N (or nothing fits a workspace of
    ``slab_floats`` floats and, if given, ``counters`` arrival counters). The rule that reproduces
    the winners of profiles/int4.md "GEMM, Llama-2-7B shapes": the fewest K splits that give at
    least INT4_GEMM_MIN_GRID workgroups (ceil(M/128) * N/bn tiles x sk) while every split keeps
    INT4_GEMM_MIN_CHUNKS groups (each split writes and the last arriver re-reads an fp32 tile, and
    pays the ring's ramp); where no split reaches that grid, the most splits that keep the chunks."""
    cands = [(bn, sk) for bn, sk in int4_gemm_candidates(M, N, K, epi)
             if int4_gemm_slab_floats(M, N, sk) <= slab_floats
             and (counters is None or sk == 1 or _row_tiles(M) * (N // bn) <= counters)]
    if not cands:
        return None

    def cost(c):
        bn, sk = c
        grid = _row_tiles(M) * (N // bn) * sk
        deep = sk == 1 or K // INT4_GROUP // sk >= INT4_GEMM_MIN_CHUNKS
        return (not deep, grid < INT4_GEMM_MIN_GRID, sk if grid >= INT4_GEMM_MIN_GRID else -sk)
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
        if not hasattr(L, "lsa_gemv_coop_int4"):
            raise RuntimeError("the kernel library has no lsa_gemv_coop_int4: rebuild it (python csrc/build.py)")
        L.lsa_gemv_coop_int4.argtypes = [vp, i, vp, vp, vp, i, i, i, i, f, i, ctypes.POINTER(hip.EpiArgs), i, i, i, i, vp, vp, vp]
        L.lsa_gemv_coop_int4.restype = i
        if not hasattr(L, "lsa_gemm_int4"):
            raise RuntimeError("the kernel library has no lsa_gemm_int4: rebuild it (python csrc/build.py)")
        L.lsa_gemm_int4.argtypes = [vp, i, vp, vp, i, i, i, i, ctypes.POINTER(hip.EpiArgs), i, i, i, vp, ctypes.c_longlong, vp, i, vp]
        L.lsa_gemm_int4.restype = i
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


def gemv_coop_int4(x: torch.Tensor, wq4: torch.Tensor, scales: torch.Tensor, M: int, N: int, K: int, epi: int,
                   ep: hip.EpiArgs, norm: bool = False, eps: float = 1e-5, ws: Optional[hip.CoopWorkspace] = None,
                   a_rows: Optional[torch.Tensor] = None, cfg: Optional[tuple] = None) -> None:
    """Cooperative W4A16 decode projection (csrc/quant/gemv_coop_int4.hip), 17 <= M <= 128, on
    :func:`gemv_int4`'s operands. ``cfg`` = (tnw, nw, d, sk), default :func:`int4_coop_config`;
    ``ws``: the split-K slab and arrival counters (default: the process-wide workspace)."""
    hip._req(INT4_COOP_MIN_ROWS <= M <= INT4_COOP_MAX_ROWS, f"gemv_coop_int4 supports 17..128 rows, got {M}")
    hip._req(epi in (hip.EPI_STORE, hip.EPI_RESID, hip.EPI_SWIGLU, hip.EPI_QKV), f"gemv_coop_int4: epilogue {epi} not built")
    hip._check_epi(epi, ep, N)
    hip._req(hip._is_bf16_cuda(x), "gemv_coop_int4: bf16 cuda activations")
    hip._req(N >= 16 and N % 16 == 0 and K >= 128 and K % 128 == 0, "gemv_coop_int4: N % 16, K % 128")
    hip._req(wq4.is_cuda and wq4.dtype == torch.uint8 and wq4.numel() == N * K // 2,
             "gemv_coop_int4: packed int4 weights [N*K/2] uint8")
    hip._req(scales.is_cuda and scales.dtype == torch.float32 and scales.numel() == N * (K // 128)
             and scales.is_contiguous(), "gemv_coop_int4: packed fp32 group scales [N*K/128]")
    hip._req(x.dim() == 2 and x.shape[1] >= K and x.stride(1) == 1, "gemv_coop_int4: x must be [rows, >=K] row-major")
    if a_rows is None:
        hip._req(x.shape[0] >= M, "gemv_coop_int4: x has fewer rows than M")
    else:
        hip._req(a_rows.dtype == torch.int32 and a_rows.is_cuda and a_rows.numel() >= M, "gemv_coop_int4: a_rows")
    if ws is None:
        ws = hip.default_workspace(x.device)
    if cfg is None:
        cfg = int4_coop_config(N // 16, K, M, epi == hip.EPI_SWIGLU, ws.slab.numel())
        hip._req(cfg is not None, f"gemv_coop_int4: no config for N={N} K={K} M={M}")
    cfg = tuple(cfg)
    hip._req(cfg in int4_coop_candidates(N // 16, K, M, epi == hip.EPI_SWIGLU),
             f"gemv_coop_int4: config {cfg} not built or invalid for N={N} K={K} M={M}")
    tnw, nw, d, sk = cfg
    need = int4_coop_slab_floats(N, M, tnw, nw, sk)
    hip._req(ws.slab.numel() >= need, f"gemv_coop_int4: workspace too small ({ws.slab.numel()} < {need} floats)")
    hip._req(ws.counters.numel() >= N // 16 // (tnw * nw), "gemv_coop_int4: workspace counters too small")
    rc = _lib().lsa_gemv_coop_int4(hip._p(x), x.stride(0), hip._p(a_rows), hip._p(wq4), hip._p(scales), M, N, K, int(norm),
                                  float(eps), epi, ctypes.byref(ep), tnw, nw, d, sk, hip._p(ws.slab), hip._p(ws.counters),
                                  hip._stream())
    hip._check(rc, "lsa_gemv_coop_int4")


def proj_int4(x: torch.Tensor, wq4: torch.Tensor, scales: torch.Tensor, M: int, N: int, K: int, epi: int,
              ep: hip.EpiArgs, norm: bool = False, eps: float = 1e-5, ws: Optional[hip.CoopWorkspace] = None,
              a_rows: Optional[torch.Tensor] = None) -> bool:
    """The int4 decode projection of ``M`` rows on its native kernel: :func:`gemv_int4` up to 64
    rows, :func:`gemv_coop_int4` from 65 to 128 and, from 17 to 64, for the classes of
    ``INT4_COOP_ROUTE``. False (nothing launched) where no native kernel serves the shape: the
    caller dequantises and runs the bf16 kernels."""
    coop = None
    if INT4_COOP_MIN_ROWS <= M <= INT4_COOP_MAX_ROWS and (M > INT4_MAX_ROWS or (N, K, row_blocks(M)) in INT4_COOP_ROUTE):
        w = ws if ws is not None else hip.default_workspace(x.device)
        coop = int4_coop_config(N // 16, K, M, epi == hip.EPI_SWIGLU, w.slab.numel(), w.counters.numel())
    if coop is not None:
        gemv_coop_int4(x, wq4, scales, M, N, K, epi, ep, norm=norm, eps=eps, ws=ws, a_rows=a_rows, cfg=coop)
    elif M <= INT4_MAX_ROWS:
        gemv_int4(x, wq4, scales, M, N, K, epi, ep, norm=norm, eps=eps, a_rows=a_rows)
    else:
        return False
    return True


def gemm_int4(x: torch.Tensor, wq4: torch.Tensor, scales: torch.Tensor, M: int, N: int, K: int, epi: int,
              ep: hip.EpiArgs, ws: Optional[hip.CoopWorkspace] = None, cfg: Optional[tuple] = None) -> None:
    """W4A16 GEMM (csrc/quant/gemm_int4.hip), any M >= 1, on :func:`gemv_int4`'s operands; the
    rows of ``x`` 16-byte aligned. ``cfg`` = (bn, sk), default :func:`int4_gemm_config`; ``ws``: the
    split-K slab and arrival counters (default: the process-wide workspace). The fused-RMSNorm
    fields of ``ep`` as in ``hip.gemm_sk``: ``ss_in`` (QKV / SWIGLU, K == 64 ss_n), ``ss_out`` (RESID)."""
    hip._req(M >= 1, f"gemm_int4 needs at least one row, got {M}")
    hip._req(epi in (hip.EPI_STORE, hip.EPI_RESID, hip.EPI_SWIGLU, hip.EPI_QKV), f"gemm_int4: epilogue {epi} not built")
    hip._check_epi(epi, ep, N)
    hip._req(hip._is_bf16_cuda(x), "gemm_int4: bf16 cuda activations")
    hip._req(N >= 16 and N % 16 == 0 and K >= 128 and K % 128 == 0, "gemm_int4: N % 16, K % 128")
    hip._req(wq4.is_cuda and wq4.dtype == torch.uint8 and wq4.numel() == N * K // 2,
             "gemm_int4: packed int4 weights [N*K/2] uint8")
    hip._req(scales.is_cuda and scales.dtype == torch.float32 and scales.numel() == N * (K // 128)
             and scales.is_contiguous(), "gemm_int4: packed fp32 group scales [N*K/128]")
    hip._req(x.dim() == 2 and x.shape[1] >= K and x.stride(1) == 1 and x.shape[0] >= M,
             "gemm_int4: x must be [>=M, >=K] row-major")
    hip._req(x.data_ptr() % 16 == 0 and x.stride(0) % 8 == 0 and M * x.stride(0) < 1 << 30,
             "gemm_int4: rows of x must be 16-byte aligned")
    hip._req(not ep.ss_in or (epi in (hip.EPI_QKV, hip.EPI_SWIGLU) and K == 64 * ep.ss_n and ep.ss_n % 4 == 0),
             "gemm_int4: ss_in needs a QKV / SWIGLU epilogue and K == 64 ss_n")
    hip._req(not ep.ss_out or (epi == hip.EPI_RESID and N == 64 * ep.ss_n), "gemm_int4: ss_out needs a RESID epilogue and N == 64 ss_n")
    hip._req(epi != hip.EPI_SWIGLU or not ep.bias, "gemm_int4: no bias on the SwiGLU epilogue")
    if ws is None:
        ws = hip.default_workspace(x.device)
    if cfg is None:
        cfg = int4_gemm_config(M, N, K, epi, ws.slab.numel(), ws.counters.numel())
        hip._req(cfg is not None, f"gemm_int4: no config for N={N} K={K} M={M}")
    cfg = tuple(cfg)
    hip._req(cfg in int4_gemm_candidates(M, N, K, epi), f"gemm_int4: config {cfg} not built or invalid for N={N} K={K} M={M}")
    bn, sk = cfg
    depth = dict(INT4_GEMM_CONFIGS)[bn]
    need = int4_gemm_slab_floats(M, N, sk)
    hip._req(ws.slab.numel() >= need, f"gemm_int4: workspace too small ({ws.slab.numel()} < {need} floats)")
    hip._req(sk == 1 or ws.counters.numel() >= _row_tiles(M) * (N // bn), "gemm_int4: workspace counters too small")
    rc = _lib().lsa_gemm_int4(hip._p(x), x.stride(0), hip._p(wq4), hip._p(scales), M, N, K, epi, ctypes.byref(ep), bn, depth, sk,
                             hip._p(ws.slab), ws.slab.numel(), hip._p(ws.counters), ws.counters.numel(), hip._stream())
    hip._check(rc, "lsa_gemm_int4")


def int4_gemm_enabled() -> bool:
    """The run-time switch, read at every call: ``LSA_INT4_GEMM=1`` routes to the native GEMM. Off
    by default: above 128 rows an int4 engine is pinned to the bits of the bf16 kernels on the
    dequantised (bf16-rounded) weights (tests/test_engine_edges_gpu.py), which a kernel that never
    rounds the weights cannot give, and the kernel is ahead on small tile counts only."""
    return os.environ.get("LSA_INT4_GEMM", "0") == "1"


def proj_gemm_int4(x: torch.Tensor, wq4: torch.Tensor, scales: Optional[torch.Tensor], M: int, N: int, K: int, epi: int,
                   ep: hip.EpiArgs, ws: Optional[hip.CoopWorkspace] = None) -> bool:
    """A prefill chunk or a decode batch above 128 rows on the native int4 GEMM, for shapes of up
    to ``INT4_GEMM_MAX_TILES`` output tiles. False (nothing launched) where the weights are not
    int4, the switch is off, no config serves the shape or it has more tiles (there the bf16 GEMM
    on dequantised weights measured level or faster): the caller dequantises."""
    if scales is None or not int4_gemm_enabled():
        return False
    w = ws if ws is not None else hip.default_workspace(x.device)
    cfg = int4_gemm_config(M, N, K, epi, w.slab.numel(), w.counters.numel())
    if cfg is None or _row_tiles(M) * (N // cfg[0]) > INT4_GEMM_MAX_TILES:
        return False
    gemm_int4(x, wq4, scales, M, N, K, epi, ep, ws=w, cfg=cfg)
    return True


def int4_gemm_serves(shapes, rows: int, slab_floats: int = INT4_COOP_SLAB_FLOATS, counters: Optional[int] = None) -> bool:
    """Whether :func:`proj_gemm_int4` takes every (N, K) of ``shapes`` at ``rows`` rows."""
    cfgs = [int4_gemm_config(rows, n, k, hip.EPI_STORE, slab_floats, counters) for n, k in shapes]
    return int4_gemm_enabled() and all(c is not None and _row_tiles(rows) * (n // c[0]) <= INT4_GEMM_MAX_TILES
                                       for c, (n, _) in zip(cfgs, shapes))


def dequant_int4_packed(wq4: torch.Tensor, scales: torch.Tensor, out: torch.Tensor, N: int, K: int) -> torch.Tensor:
    """Packed int4 (+ packed group scales) -> packed bf16 (pack_b layout) in ``out`` (>= N*K bf16)."""
    hip._req(N >= 16 and N % 16 == 0 and K >= 128 and K % 128 == 0, "dequant_int4: N % 16, K % 128")
    hip._req(wq4.is_cuda and wq4.dtype == torch.uint8 and wq4.numel() == N * K // 2, "dequant_int4: weights")
    hip._req(scales.is_cuda and scales.dtype == torch.float32 and scales.numel() == N * (K // 128)
         and scales.is_contiguous(), "dequant_int4: scales")
    hip._req(hip._is_bf16_cuda(out) and out.numel() >= N * K and out.is_contiguous(), "dequant_int4: out")
    hip._check(_lib().lsa_dequant_int4_packed(hip._p(wq4), hip._p(scales), hip._p(out), N, K, hip._stream()), "lsa_dequant_int4_packed")
    return out.view(-1)[:N * K].view(N // 16, K // 32, 64, 8)
