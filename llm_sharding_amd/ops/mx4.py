"""MXFP4 weights (W4A8 decode): the OCP microscaling format, its packed layout for the gfx950
block-scaled MFMA, the activation quantiser's contract, the kernel's configs and bindings
(csrc/quant/gemv_mx4.hip) and the dispatcher :func:`proj_mx4`; at the end, the activation image,
configs and bindings of the opt-in GEMM for more than 128 rows (csrc/quant/gemm_mx4.hip,
:func:`proj_gemm_mx4`).

Weights. Each fused, norm-folded projection ``W[N, K]`` is cut along K into blocks of 32; a block
is one e8m0 exponent byte ``e`` (scale ``2^(e - 127)``) and 32 e2m1 codes (sign bit 8, magnitudes
0, 0.5, 1, 1.5, 2, 3, 4, 6): 4.25 bits per weight. The scale follows OCP,
``eb = floor(log2(amax)) - 2``, codes are ``e2m1_rne(w * 2^-eb)`` saturated at +-6, an all-zero
block has scale 1, and ``eb`` is clamped to [-125, 125] so that every ``code * 2^eb`` is a bf16
normal: dequantisation to bf16 is exact. On the device a projection is

* ``Wq[nt][K/128][lane][16 B]`` (:func:`pack_b_mx4`): the B fragment of
  ``v_mfma_scale_f32_16x16x128_f8f6f4``. Lane ``l`` holds column ``l & 15`` and the 32-block
  ``l >> 4`` of the 128-k step, element ``j`` at nibble ``j`` (the lower k in a byte's low nibble):
  one 16-byte load per lane and MFMA;
* ``S[nt][ceil(K/512)][lane][4 B]`` (:func:`pack_scales_mx4`): byte ``i`` of the dword of lane
  ``16 b + column`` is the exponent of 32-block ``b`` of K-step ``4 g + i``, which the MFMA picks
  with ``op_sel`` - one dword load per lane covers four K-steps (the tail padded with 127).

Activations (:func:`quantize_act_mx8`). Per row and 32-block, the fp8 KV cache's convention
(``kv8.quantize_reference``): ``E`` the fp32 exponent field of the block's largest magnitude
(clamped to >= 8; 134 for an all-zero block), scale ``2^(E - 134)`` as e8m0 byte ``E - 7``, codes
``e4m3_rne(x * 2^(134 - E))``. Nothing saturates; the NaN code and e8m0 255 never appear.

Result: ``y[m, n] = sum_blocks 2^(ea + eb) * sum_{k in block} a8[m, k] * w4[n, k]`` in fp32, then
``rstd`` (from the bf16 activations as read), bias, residual and one rounding to bf16 as in the
int4 and fp8 kernels. :func:`linear_reference` states it in fp64.

Like ops/int4.py this module stands beside ops/packing.py and ops/hip.py, the recorded inputs of
the bf16 decode path's full-depth fixture."""
from __future__ import annotations

import ctypes
import os
from typing import Optional

import torch

from . import hip, kv8
from .packing import N_CU, row_blocks

MX_BLOCK = 32    # k per scale block (OCP MX)
MX_STEP = 128    # k per MFMA K-step: one 16-byte fp4 load per lane
MX_GROUP = 512   # k per scale dword (4 K-steps)
E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
MX_EB_MIN, MX_EB_MAX = -125, 125  # block exponents at which every code * 2^eb is a bf16 normal


def _check_shape(N: int, K: int, what: str) -> None:
    if N % 16 or K % MX_STEP or K < MX_STEP:
        raise ValueError(f"{what} needs N%16==0 and K%{MX_STEP}==0, got {(N, K)}")


def quantize_mx4(w: torch.Tensor) -> tuple:
    """``w`` [N, K] (K % 32 == 0, finite) -> (codes uint8 [N, K] in 0..15, e uint8 [N, K/32] e8m0)."""
    N, K = w.shape
    if K % MX_BLOCK:
        raise ValueError(f"mxfp4 weights need K % {MX_BLOCK} == 0, got K={K}")
    wf = w.float().view(N, K // MX_BLOCK, MX_BLOCK)
    amax = wf.abs().amax(dim=-1)
    eb = ((amax.contiguous().view(torch.int32) >> 23) - 127 - 2).clamp(MX_EB_MIN, MX_EB_MAX)
    eb = torch.where(amax == 0, torch.zeros_like(eb), eb)
    a = (wf * ((127 - eb) << 23).view(torch.float32)[..., None]).abs()  # exact: a power of two
    # round to nearest, ties to the even code; above 6 saturates at code 7
    code = ((a > 0.25).int() + (a >= 0.75).int() + (a > 1.25).int() + (a >= 1.75).int() + (a > 2.5).int()
            + (a >= 3.5).int() + (a > 5.0).int())
    code = code + 8 * (wf < 0).int()
    return code.view(N, K).to(torch.uint8), (eb + 127).to(torch.uint8)


def dequantize_mx4(q: torch.Tensor, e: torch.Tensor) -> torch.Tensor:
    """bf16 [N, K] = code * 2^(e - 127), exact."""
    N, K = q.shape
    lut = torch.tensor(E2M1 + tuple(-v for v in E2M1), dtype=torch.float32, device=q.device)
    sc = (e.to(torch.int32) << 23).view(torch.float32)
    return (lut[q.long()].view(N, K // MX_BLOCK, MX_BLOCK) * sc[..., None]).view(N, K).to(torch.bfloat16)


def pack_b_mx4(q: torch.Tensor) -> torch.Tensor:
    """Codes [N, K] -> uint8 [N*K/2] as Wq[nt][K/128][lane][16 B]: lane = 16 * block + column,
    byte p = code[2p] | code[2p + 1] << 4."""
    N, K = q.shape
    _check_shape(N, K, "pack_b_mx4")
    if q.dtype != torch.uint8 or int(q.max()) > 15:
        raise ValueError("pack_b_mx4 needs uint8 codes in 0..15")
    v = q.view(N // 16, 16, K // MX_STEP, 4, 16, 2).permute(0, 2, 3, 1, 4, 5)
    return (v[..., 0] | (v[..., 1] << 4)).reshape(-1)


def unpack_b_mx4(p: torch.Tensor, N: int, K: int) -> torch.Tensor:
    """Inverse of :func:`pack_b_mx4`: codes uint8 [N, K]."""
    _check_shape(N, K, "unpack_b_mx4")
    if p.dtype != torch.uint8 or p.numel() != N * K // 2:
        raise ValueError(f"unpack_b_mx4: {N * K // 2} packed bytes expected")
    by = p.view(N // 16, K // MX_STEP, 4, 16, 16)
    v = torch.stack([by & 15, by >> 4], dim=-1)
    return v.permute(0, 3, 1, 2, 4, 5).reshape(N, K).contiguous()


def scale_groups(K: int) -> int:
    return -(-K // MX_GROUP)


def pack_scales_mx4(e: torch.Tensor) -> torch.Tensor:
    """e8m0 bytes [N, K/32] -> uint8 [N/16 * ceil(K/512) * 64 * 4] as S[nt][g][lane][i]: byte i of
    lane 16 * block + column is the exponent of that block in K-step 4 g + i (127 past the end)."""
    N, B = e.shape
    if N % 16 or B % 4 or e.dtype != torch.uint8:
        raise ValueError(f"pack_scales_mx4 needs uint8 [N%16==0, K/32 with K%128==0], got {tuple(e.shape)}")
    ks, ng = B // 4, scale_groups(B * MX_BLOCK)
    pad = torch.full((N, 4 * ng, 4), 127, dtype=torch.uint8, device=e.device)
    pad[:, :ks] = e.view(N, ks, 4)
    return pad.view(N // 16, 16, ng, 4, 4).permute(0, 2, 4, 1, 3).reshape(-1)


def unpack_scales_mx4(s: torch.Tensor, N: int, K: int) -> torch.Tensor:
    ng = scale_groups(K)
    v = s.view(N // 16, ng, 4, 16, 4).permute(0, 3, 1, 4, 2).reshape(N, 4 * ng, 4)
    return v[:, :K // MX_STEP].reshape(N, K // MX_BLOCK).contiguous()


def mx4_bytes(n: int, k: int) -> int:
    """Bytes of an mxfp4 projection: nibbles + one exponent byte per 32 (4.25 bits per weight)."""
    return n * k // 2 + n * (k // MX_BLOCK)


def quantize_act_mx8(x: torch.Tensor) -> tuple:
    """bf16 [M, K] -> (e4m3 codes uint8 [M, K], e8m0 bytes uint8 [M, K/32])."""
    M, K = x.shape
    codes, s = kv8.quantize_reference(x.contiguous().view(M, K // MX_BLOCK, MX_BLOCK))
    return codes.view(M, K), (s.contiguous().view(torch.int32) >> 23).to(torch.uint8)


def dequantize_act_mx8(codes: torch.Tensor, e: torch.Tensor) -> torch.Tensor:
    """fp64 [M, K] = code * 2^(e - 127)."""
    M, K = codes.shape
    sc = (e.to(torch.int32) << 23).view(torch.float32).double()
    return (codes.view(torch.float8_e4m3fn).double().view(M, K // MX_BLOCK, MX_BLOCK) * sc[..., None]).view(M, K)


def linear_reference(x: torch.Tensor, q: torch.Tensor, e: torch.Tensor) -> torch.Tensor:
    """fp64 [M, N]: the W4A8 product of bf16 activations ``x`` [M, K] and mxfp4 weights (q, e)."""
    return dequantize_act_mx8(*quantize_act_mx8(x)) @ dequantize_mx4(q, e).double().t()


# (mb, tnw, nw) instantiated in csrc/quant/gemv_mx4.hip (LSA_MX4_CONFIGS) - keep in sync. nw waves
# of tnw 16-column tiles each share a workgroup's quantised A; mb row blocks of 16.
MX4_CONFIGS = [(1, 1, 4), (1, 2, 4), (2, 1, 4), (2, 2, 4), (2, 1, 8), (4, 1, 4), (4, 2, 4), (4, 1, 8), (8, 1, 4),
               (8, 1, 8)]
MX4_MAX_ROWS = 128
MX4_SPLITS = (1, 2, 4, 8)
# workgroups from which the chooser stops splitting K: one per CU for 4-wave workgroups, 160 for
# 8-wave ones (profiles/mx4.md "Per kernel": the fastest 8-wave grids were 172..256)
MX4_MIN_GRID, MX4_MIN_GRID_8 = N_CU, 160


def _col_groups(n_tiles: int, tnw: int, nw: int) -> int:
    return -(-n_tiles // (tnw * nw))


def mx4_slab_floats(n_tiles: int, rows: int, tnw: int, nw: int, sk: int) -> int:
    """fp32 workspace a launch needs: sk partial tiles of whole column groups + partial sums of
    squares (0 when sk == 1)."""
    if sk <= 1:
        return 0
    mr, cg = 16 * row_blocks(rows), _col_groups(n_tiles, tnw, nw)
    return sk * cg * tnw * nw * 16 * mr + sk * cg * mr


def mx4_candidates(n_tiles: int, k: int, rows: int, need_even: bool = False) -> list:
    """(tnw, nw, sk): any tile count (a workgroup's last waves may own no tile; SwiGLU needs an
    even tile count and an even workgroup), every K split keeps a 512-k scale group."""
    if not 1 <= rows <= MX4_MAX_ROWS or k % MX_STEP or k < MX_STEP or (need_even and n_tiles % 2):
        return []
    mb = row_blocks(rows)
    return [(tnw, nw, sk) for (b, tnw, nw) in MX4_CONFIGS if b == mb and not (need_even and (tnw * nw) % 2)
            for sk in MX4_SPLITS if sk <= scale_groups(k) and _col_groups(n_tiles, tnw, nw) * sk <= 8 * N_CU]


def mx4_config(n_tiles: int, k: int, rows: int, need_even: bool = False, slab_floats: Optional[int] = None,
               counters: Optional[int] = None) -> Optional[tuple]:
    """(tnw, nw, sk) or None. The rule that reproduces the winners of profiles/mx4.md "Per kernel"
    to within 10 %: from 17 rows on, 8 waves per workgroup (A is quantised once per column group
    and the waves' MFMAs hide one another's loads); the fewest K splits that reach the minimum grid
    (every split writes and the last arriver re-reads an fp32 tile), among those the widest
    workgroup; where nothing reaches that grid, the largest grid."""
    cands = [c for c in mx4_candidates(n_tiles, k, rows, need_even)
             if (slab_floats is None or mx4_slab_floats(n_tiles, rows, *c) <= slab_floats)
             and (counters is None or _col_groups(n_tiles, c[0], c[1]) <= counters)]
    if not cands:
        return None
    want8 = row_blocks(rows) >= 2

    def cost(c):
        tnw, nw, sk = c
        grid, need = _col_groups(n_tiles, tnw, nw) * sk, MX4_MIN_GRID_8 if nw == 8 else MX4_MIN_GRID
        return (want8 and nw != 8, grid < need, sk if grid >= need else -grid, -tnw * nw, -nw)
    return min(cands, key=cost)


# ------------------------------------------------------------------------------ bindings
_L = None


def _lib():
    global _L
    if _L is None:
        L = hip.lib()
        if not hasattr(L, "lsa_gemv_mx4"):
            raise RuntimeError("the kernel library has no lsa_gemv_mx4: rebuild it (python csrc/build.py)")
        vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
        L.lsa_gemv_mx4.argtypes = [vp, i, vp, vp, vp, i, i, i, i, f, i, ctypes.POINTER(hip.EpiArgs), i, i, i, vp, vp, vp]
        L.lsa_dequant_mx4_packed.argtypes = [vp, vp, vp, i, i, vp]
        L.lsa_gemv_mx4.restype = L.lsa_dequant_mx4_packed.restype = i
        if not hasattr(L, "lsa_gemm_mx4"):
            raise RuntimeError("the kernel library has no lsa_gemm_mx4: rebuild it (python csrc/build.py)")
        L.lsa_quant_act_mx8.argtypes = [vp, i, vp, vp, vp, i, i, vp]
        L.lsa_gemm_mx4.argtypes = [vp, vp, vp, vp, i, i, i, i, ctypes.POINTER(hip.EpiArgs), i, i, vp, ctypes.c_longlong, vp,
                                   i, vp]
        L.lsa_quant_act_mx8.restype = L.lsa_gemm_mx4.restype = i
        _L = L
    return _L


def _check_weights(wq: torch.Tensor, scales: torch.Tensor, N: int, K: int, what: str) -> None:
    hip._req(N >= 16 and N % 16 == 0 and K >= MX_STEP and K % MX_STEP == 0 and N * K // 2 < 1 << 31,
             f"{what}: N % 16, K % {MX_STEP}")
    hip._req(wq.is_cuda and wq.dtype == torch.uint8 and wq.numel() == N * K // 2 and wq.is_contiguous(),
             f"{what}: packed fp4 weights [N*K/2] uint8")
    hip._req(scales.is_cuda and scales.dtype == torch.uint8 and scales.numel() == N * scale_groups(K) * 16
             and scales.is_contiguous() and scales.data_ptr() % 4 == 0, f"{what}: packed e8m0 scales (pack_scales_mx4)")


def gemv_mx4(x: torch.Tensor, wq: torch.Tensor, scales: torch.Tensor, M: int, N: int, K: int, epi: int,
             ep: hip.EpiArgs, norm: bool = False, eps: float = 1e-5, ws: Optional[hip.CoopWorkspace] = None,
             a_rows: Optional[torch.Tensor] = None, cfg: Optional[tuple] = None) -> None:
    """W4A8 decode projection (csrc/quant/gemv_mx4.hip), 1 <= M <= 128: ``wq`` = pack_b_mx4(codes),
    ``scales`` = pack_scales_mx4(e). ``cfg`` = (tnw, nw, sk), default :func:`mx4_config`; ``ws``: the
    split-K slab and arrival counters (default: the process-wide workspace)."""
    hip._req(1 <= M <= MX4_MAX_ROWS, f"gemv_mx4 supports 1..{MX4_MAX_ROWS} rows, got {M}")
    hip._req(epi in (hip.EPI_STORE, hip.EPI_RESID, hip.EPI_SWIGLU, hip.EPI_QKV), f"gemv_mx4: epilogue {epi} not built")
    hip._check_epi(epi, ep, N)
    hip._req(hip._is_bf16_cuda(x), "gemv_mx4: bf16 cuda activations")
    _check_weights(wq, scales, N, K, "gemv_mx4")
    hip._req(x.dim() == 2 and x.shape[1] >= K and x.stride(1) == 1 and x.data_ptr() % 16 == 0 and x.stride(0) % 8 == 0,
             "gemv_mx4: x must be [rows, >=K] row-major with 16-byte aligned rows")
    if a_rows is None:
        hip._req(x.shape[0] >= M, "gemv_mx4: x has fewer rows than M")
    else:
        hip._req(a_rows.dtype == torch.int32 and a_rows.is_cuda and a_rows.numel() >= M, "gemv_mx4: a_rows")
    if ws is None:
        ws = hip.default_workspace(x.device)
    even = epi == hip.EPI_SWIGLU
    if cfg is None:
        cfg = mx4_config(N // 16, K, M, even, ws.slab.numel(), ws.counters.numel())
        hip._req(cfg is not None, f"gemv_mx4: no config for N={N} K={K} M={M}")
    cfg = tuple(cfg)
    hip._req(cfg in mx4_candidates(N // 16, K, M, even), f"gemv_mx4: config {cfg} not built or invalid for N={N} K={K} M={M}")
    tnw, nw, sk = cfg
    need = mx4_slab_floats(N // 16, M, tnw, nw, sk)
    hip._req(ws.slab.numel() >= need, f"gemv_mx4: workspace too small ({ws.slab.numel()} < {need} floats)")
    hip._req(sk == 1 or ws.counters.numel() >= _col_groups(N // 16, tnw, nw), "gemv_mx4: workspace counters too small")
    rc = _lib().lsa_gemv_mx4(hip._p(x), x.stride(0), hip._p(a_rows), hip._p(wq), hip._p(scales), M, N, K, int(norm),
                            float(eps), epi, ctypes.byref(ep), tnw, nw, sk, hip._p(ws.slab), hip._p(ws.counters),
                            hip._stream())
    hip._check(rc, "lsa_gemv_mx4")


def proj_mx4(x: torch.Tensor, wq: torch.Tensor, scales: torch.Tensor, M: int, N: int, K: int, epi: int,
             ep: hip.EpiArgs, norm: bool = False, eps: float = 1e-5, ws: Optional[hip.CoopWorkspace] = None,
             a_rows: Optional[torch.Tensor] = None) -> bool:
    """The mxfp4 decode projection of ``M`` <= 128 rows on :func:`gemv_mx4`. False (nothing
    launched) where no config serves the shape: the caller dequantises and runs the bf16 kernels."""
    w = ws if ws is not None else hip.default_workspace(x.device)
    cfg = mx4_config(N // 16, K, M, epi == hip.EPI_SWIGLU, w.slab.numel(), w.counters.numel()) if M <= MX4_MAX_ROWS else None
    if cfg is None:
        return False
    gemv_mx4(x, wq, scales, M, N, K, epi, ep, norm=norm, eps=eps, ws=w, a_rows=a_rows, cfg=cfg)
    return True


def dequant_mx4_packed(wq: torch.Tensor, scales: torch.Tensor, out: torch.Tensor, N: int, K: int) -> torch.Tensor:
    """Packed fp4 (+ packed exponents) -> packed bf16 (pack_b layout) in ``out`` (>= N*K bf16), exact."""
    _check_weights(wq, scales, N, K, "dequant_mx4")
    hip._req(hip._is_bf16_cuda(out) and out.numel() >= N * K and out.is_contiguous() and out.data_ptr() % 16 == 0,
             "dequant_mx4: out")
    hip._check(_lib().lsa_dequant_mx4_packed(hip._p(wq), hip._p(scales), hip._p(out), N, K, hip._stream()),
               "lsa_dequant_mx4_packed")
    return out.view(-1)[:N * K].view(N // 16, K // 32, 64, 8)


# ------------------------------------------------------------------------------ the GEMM (prefill, > 128 rows)
# csrc/quant/gemm_mx4.hip. The activations are quantised ONCE per projection input by a pre-pass
# (lsa_quant_act_mx8, exactly quantize_act_mx8) into the image the MFMA's A operand wants:
# * codes ``A8[ceil(M/16)][K/128][2 halves][64 lanes][16 B]``: element k of a K-step sits in half
#   ``k // 64``, lane ``16 * ((k % 64) // 16) + row``, byte ``k % 16`` - a row block's K-step is
#   2 KiB contiguous, and two ds_read_b128 per lane are the operand;
# * exponents ``EA[ceil(M/16)][ceil(K/512)][64 lanes]`` dwords: byte ``i`` of lane ``16 b + row`` is
#   the e8m0 byte of 32-block ``b`` in K-step ``4 g + i`` (127 past K), picked by ``op_sel`` as the
#   weight scales are: the GEMM reads one dword per row block and FOUR K-steps, straight into a
#   register (the ISA takes scale_a from a VGPR byte, so the exponents never pass through LDS);
# * rows >= M of the last row block: zero codes, exponent 127.
# (bn, depth) instantiated in gemm_mx4.hip - keep in sync. bn 256 is not built: its SwiGLU and QKV
# instantiations needed 36 bytes of scratch per lane (the kernel's header has the compiler's report).
MX4_GEMM_CONFIGS = [(128, 4)]
MX4_GEMM_SPLITS = (1, 2, 4, 8)
MX4_GEMM_ROWS = 128       # rows of an output tile
# workgroups from which a further K split measured no faster: 192 reproduces the fastest split of
# every shape and row count of profiles/mx4.md "GEMM above 128 rows" (qkv at 256 rows, 192 tiles,
# is fastest unsplit; 64 / 128 tiles want 4 / 2 splits). Every measured shape beat dequantise + bf16
# by more than the spread, so with the switch on no shape is routed back.
MX4_GEMM_MIN_GRID = 192


def a_image_bytes(M: int, K: int) -> tuple:
    """(code bytes, exponent bytes) of the MXFP8 image of ``M`` rows x ``K``."""
    rb = -(-M // 16)
    return rb * 16 * K, rb * scale_groups(K) * 256


def pack_a_mx8(x: torch.Tensor) -> tuple:
    """bf16 [M, K] (K % 128 == 0) -> (A8 uint8 flat, EA uint8 flat): :func:`quantize_act_mx8` in the
    pre-pass's layout, the padded rows included."""
    M, K = x.shape
    if K % MX_STEP or K < MX_STEP:
        raise ValueError(f"pack_a_mx8 needs K % {MX_STEP} == 0, got K={K}")
    codes, e = quantize_act_mx8(x)
    rb, ks, ng = -(-M // 16), K // MX_STEP, scale_groups(K)
    cp = torch.zeros(rb * 16, K, dtype=torch.uint8, device=x.device)
    cp[:M] = codes
    ep = torch.full((rb * 16, 4 * ng, 4), 127, dtype=torch.uint8, device=x.device)
    ep[:M, :ks] = e.view(M, ks, 4)
    a8 = cp.view(rb, 16, ks, 2, 4, 16).permute(0, 2, 3, 4, 1, 5).reshape(-1)  # [rb][step][half][group][row][byte]
    ea = ep.view(rb, 16, ng, 4, 4).permute(0, 2, 4, 1, 3).reshape(-1)        # [rb][g][block][row][i]
    return a8, ea


def _row_tiles(M: int) -> int:
    return -(-M // MX4_GEMM_ROWS)


def mx4_gemm_slab_floats(M: int, N: int, sk: int) -> int:
    """fp32 workspace a split mxfp4 GEMM launch needs: sk partial tiles of whole 128-row tiles
    (0 when sk == 1)."""
    return 0 if sk <= 1 else sk * _row_tiles(M) * MX4_GEMM_ROWS * N


def mx4_gemm_candidates(M: int, N: int, K: int, epi: int = 0) -> list:
    """(bn, sk) the mxfp4 GEMM can run: bn divides N, every K split keeps a 512-k scale group, the
    partial slab stays under 2 GiB."""
    if M < 1 or N < 1 or K < MX_STEP or K % MX_STEP or N * K // 2 >= 1 << 31 \
            or epi not in (hip.EPI_STORE, hip.EPI_RESID, hip.EPI_SWIGLU, hip.EPI_QKV):
        return []
    return [(bn, sk) for bn, _ in MX4_GEMM_CONFIGS if N % bn == 0 for sk in MX4_GEMM_SPLITS
            if sk <= scale_groups(K) and 4 * mx4_gemm_slab_floats(M, N, sk) < 1 << 31]


def mx4_gemm_config(M: int, N: int, K: int, epi: int = 0, slab_floats: Optional[int] = None,
                    counters: Optional[int] = None) -> Optional[tuple]:
    """(bn, sk) or None when no built tile divides N or nothing fits the workspace. The fewest K
    splits that give at least MX4_GEMM_MIN_GRID workgroups (every split writes and the last
    arriver re-reads an fp32 tile); where no split reaches that grid, the most splits."""
    cands = [(bn, sk) for bn, sk in mx4_gemm_candidates(M, N, K, epi)
             if (slab_floats is None or mx4_gemm_slab_floats(M, N, sk) <= slab_floats)
             and (counters is None or sk == 1 or _row_tiles(M) * (N // bn) <= counters)]
    if not cands:
        return None

    def cost(c):
        bn, sk = c
        grid = _row_tiles(M) * (N // bn) * sk
        return (grid < MX4_GEMM_MIN_GRID, sk if grid >= MX4_GEMM_MIN_GRID else -sk)
    return min(cands, key=cost)


def quant_act_mx8(x: torch.Tensor, M: int, K: int, scratch: torch.Tensor, a_rows: Optional[torch.Tensor] = None) -> tuple:
    """The pre-pass: rows of bf16 ``x`` [>=M, >=K] (16-byte aligned; gathered through ``a_rows`` if
    given) -> (A8, EA) views of the uint8 ``scratch``, which must hold ``sum(a_image_bytes(M, K))``."""
    nc, ne = a_image_bytes(M, K)
    hip._req(M >= 1 and K >= MX_STEP and K % MX_STEP == 0, f"quant_act_mx8: K % {MX_STEP}")
    hip._req(hip._is_bf16_cuda(x) and x.dim() == 2 and x.shape[1] >= K and x.stride(1) == 1 and x.data_ptr() % 16 == 0
             and x.stride(0) % 8 == 0, "quant_act_mx8: x must be bf16 [rows, >=K] row-major with 16-byte aligned rows")
    if a_rows is None:
        hip._req(x.shape[0] >= M, "quant_act_mx8: x has fewer rows than M")
    else:
        hip._req(a_rows.dtype == torch.int32 and a_rows.is_cuda and a_rows.numel() >= M, "quant_act_mx8: a_rows")
    hip._req(scratch.is_cuda and scratch.dtype == torch.uint8 and scratch.is_contiguous() and scratch.numel() >= nc + ne
             and scratch.data_ptr() % 16 == 0, f"quant_act_mx8: scratch of {nc + ne} uint8 bytes, 16-byte aligned")
    a8, ea = scratch.view(-1)[:nc], scratch.view(-1)[nc:nc + ne]
    hip._check(_lib().lsa_quant_act_mx8(hip._p(x), x.stride(0), hip._p(a_rows), hip._p(a8), hip._p(ea), M, K, hip._stream()),
               "lsa_quant_act_mx8")
    return a8, ea


def gemm_mx4(a8: torch.Tensor, ea: torch.Tensor, wq: torch.Tensor, scales: torch.Tensor, M: int, N: int, K: int,
             epi: int, ep: hip.EpiArgs, ws: Optional[hip.CoopWorkspace] = None, cfg: Optional[tuple] = None) -> None:
    """W4A8 GEMM (csrc/quant/gemm_mx4.hip), any M >= 1: (``a8``, ``ea``) the pre-pass image of the
    activations, ``wq`` / ``scales`` as for :func:`gemv_mx4`. ``cfg`` = (bn, sk), default
    :func:`mx4_gemm_config`; ``ws``: the split-K slab and arrival counters. The fused-RMSNorm fields
    of ``ep`` as in ``hip.gemm_sk``: ``ss_in`` (QKV / SWIGLU, K == 64 ss_n), ``ss_out`` (RESID)."""
    hip._req(M >= 1, f"gemm_mx4 needs at least one row, got {M}")
    hip._req(epi in (hip.EPI_STORE, hip.EPI_RESID, hip.EPI_SWIGLU, hip.EPI_QKV), f"gemm_mx4: epilogue {epi} not built")
    hip._check_epi(epi, ep, N)
    _check_weights(wq, scales, N, K, "gemm_mx4")
    nc, ne = a_image_bytes(M, K)
    hip._req(a8.is_cuda and a8.dtype == torch.uint8 and a8.is_contiguous() and a8.numel() >= nc and a8.data_ptr() % 16 == 0
             and ea.is_cuda and ea.dtype == torch.uint8 and ea.is_contiguous() and ea.numel() >= ne and ea.data_ptr() % 4 == 0,
             f"gemm_mx4: the activation image needs {nc} code and {ne} exponent bytes, 16-byte aligned (quant_act_mx8)")
    hip._req(not ep.ss_in or (epi in (hip.EPI_QKV, hip.EPI_SWIGLU) and K == 64 * ep.ss_n and ep.ss_n % 4 == 0),
             "gemm_mx4: ss_in needs a QKV / SWIGLU epilogue and K == 64 ss_n")
    hip._req(not ep.ss_out or (epi == hip.EPI_RESID and N == 64 * ep.ss_n), "gemm_mx4: ss_out needs a RESID epilogue and N == 64 ss_n")
    hip._req(epi != hip.EPI_SWIGLU or not ep.bias, "gemm_mx4: no bias on the SwiGLU epilogue")
    if ws is None:
        ws = hip.default_workspace(wq.device)
    if cfg is None:
        cfg = mx4_gemm_config(M, N, K, epi, ws.slab.numel(), ws.counters.numel())
        hip._req(cfg is not None, f"gemm_mx4: no config for N={N} K={K} M={M}")
    cfg = tuple(cfg)
    hip._req(cfg in mx4_gemm_candidates(M, N, K, epi), f"gemm_mx4: config {cfg} not built or invalid for N={N} K={K} M={M}")
    bn, sk = cfg
    need = mx4_gemm_slab_floats(M, N, sk)
    hip._req(ws.slab.numel() >= need, f"gemm_mx4: workspace too small ({ws.slab.numel()} < {need} floats)")
    hip._req(sk == 1 or ws.counters.numel() >= _row_tiles(M) * (N // bn), "gemm_mx4: workspace counters too small")
    rc = _lib().lsa_gemm_mx4(hip._p(a8), hip._p(ea), hip._p(wq), hip._p(scales), M, N, K, epi, ctypes.byref(ep), bn, sk,
                            hip._p(ws.slab), ws.slab.numel(), hip._p(ws.counters), ws.counters.numel(), hip._stream())
    hip._check(rc, "lsa_gemm_mx4")


def mx4_gemm_enabled() -> bool:
    """The run-time switch, read at every call: ``LSA_MX4_GEMM=1`` routes prefill chunks and decode
    batches above 128 rows to the native GEMM. Off by default: it makes those rows W4A8 (MXFP8
    activations), a numerics change a user chooses; the default keeps the bits of the bf16 kernels
    on the dequantised weights (tests/test_mx4_gpu.py)."""
    return os.environ.get("LSA_MX4_GEMM", "0") == "1"


def proj_gemm_mx4(x: torch.Tensor, wq: torch.Tensor, scales: Optional[torch.Tensor], M: int, N: int, K: int, epi: int,
                  ep: hip.EpiArgs, ws: Optional[hip.CoopWorkspace] = None, a_scratch: Optional[torch.Tensor] = None) -> bool:
    """A prefill chunk or a decode batch above 128 rows on the native mxfp4 GEMM: the pre-pass into
    ``a_scratch``, then :func:`gemm_mx4`. False (nothing launched) where the weights are not mxfp4,
    the switch is off, there is no scratch for the image or no config serves the shape: the caller
    dequantises."""
    if scales is None or a_scratch is None or not mx4_gemm_enabled() or sum(a_image_bytes(M, K)) > a_scratch.numel():
        return False
    w = ws if ws is not None else hip.default_workspace(x.device)
    cfg = mx4_gemm_config(M, N, K, epi, w.slab.numel(), w.counters.numel())
    if cfg is None:
        return False
    a8, ea = quant_act_mx8(x, M, K, a_scratch)
    gemm_mx4(a8, ea, wq, scales, M, N, K, epi, ep, ws=w, cfg=cfg)
    return True


def mx4_gemm_serves(shapes, rows: int, slab_floats: Optional[int] = None, counters: Optional[int] = None) -> bool:
    """Whether :func:`proj_gemm_mx4` takes every (N, K) of ``shapes`` at ``rows`` rows."""
    return mx4_gemm_enabled() and all(mx4_gemm_config(rows, n, k, hip.EPI_STORE, slab_floats, counters) is not None
                                      for n, k in shapes)
