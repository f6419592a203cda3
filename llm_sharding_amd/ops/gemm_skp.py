"""ctypes binding, workspace sizing and plan lookup of ``lsa_gemm_skp`` (csrc/gemm_skp/gemm_skp.hip):
gemm_sk's split-K projection with the fix-up shared by all contributors of a tile.

Every ``bm`` x ``bn`` tile is split into exactly ``contributors`` (2..8) equal K ranges, one
workgroup each, all in one round; the contributors reduce disjoint bands of the tile in parallel
instead of the last arriver reducing all of it. Results are bitwise those of ``hip.gemm_sk`` at
the same ``(bm, bn, split)``. Epilogues: EPI_STORE, EPI_RESID (with or without ``ss_out``).

The plan table is ``skp_tuning.txt`` beside this file (``LSA_GEMM_SKP_TUNING`` names another):
one measured winner per line, written by scripts/tune_gemm_skp.py and adopted per shape only
after an engine A/B run (profiles/skp_fixup.md):

    M N K bm bn contributors tile_major   # comment

A shape takes the entry with the same (N, K) and the same number of 128-row tiles whose M is
nearest; a shape without one keeps gemm_sk (``plan`` returns None). ``LSA_GEMM_SKP=0`` turns
every route off.
"""
from __future__ import annotations

import ctypes
import functools
import os
from typing import Optional

import torch

from . import hip

MAX_CONTRIBUTORS = 8   # = the counters per tile the kernel strides by
MAX_GRID = 1024
TUNING_FILE = os.environ.get("LSA_GEMM_SKP_TUNING") or os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                   "skp_tuning.txt")


def enabled() -> bool:
    """The run-time switch, read at every call: ``LSA_GEMM_SKP=0`` restores gemm_sk everywhere."""
    return os.environ.get("LSA_GEMM_SKP", "1") != "0"


def tiles(M: int, N: int, bm: int, bn: int) -> int:
    return -(-M // bm) * (N // bn)


def check_plan(M: int, N: int, K: int, bm: int, bn: int, contributors: int) -> Optional[str]:
    """Why the kernel cannot take this plan (what ``lsa_gemm_skp`` refuses), or None."""
    if bm not in (128, 256) or bn not in (128, 256):
        return f"tile {bm}x{bn}: bm and bn are 128 or 256"
    if M < 1 or K < 64 or K % 64 or N < bn or N % bn:
        return f"shape M={M} N={N} K={K} does not tile by {bm}x{bn}x64"
    if not 2 <= contributors <= MAX_CONTRIBUTORS:
        return f"{contributors} contributors: 2..{MAX_CONTRIBUTORS}"
    if contributors > K // 64:
        return f"{contributors} contributors for {K // 64} K-tiles"
    if tiles(M, N, bm, bn) * contributors > MAX_GRID:
        return f"{tiles(M, N, bm, bn)} tiles x {contributors} contributors exceed {MAX_GRID} workgroups"
    return None


def slab_floats(M: int, N: int, bm: int, bn: int, contributors: int) -> int:
    """fp32 slab elements a launch needs (gemm_sk's layout: two slots per workgroup)."""
    return 2 * tiles(M, N, bm, bn) * contributors * bm * bn


def n_counters(M: int, N: int, bm: int, bn: int) -> int:
    return tiles(M, N, bm, bn) * MAX_CONTRIBUTORS


class SkpWorkspace:
    """Partial slabs and per-(tile, band) tickets for ``gemm_skp``. Tickets reset themselves; slabs
    need no initialisation. One workspace per stream / concurrently replayed graph. ``hip.SkWorkspace``
    (same fields; 4 * grid counters) serves every plan of up to grid / 2 tiles as well."""

    def __init__(self, device, slab_floats: int, counters: int):
        self.slab = torch.empty(slab_floats, dtype=torch.float32, device=device)
        self.counters = torch.zeros(counters, dtype=torch.int32, device=device)

    @classmethod
    def for_plan(cls, device, M: int, N: int, bm: int, bn: int, contributors: int) -> "SkpWorkspace":
        return cls(device, slab_floats(M, N, bm, bn, contributors), n_counters(M, N, bm, bn))


def parse_table(text: str) -> dict:
    """(N, K) -> [(M, (bm, bn, contributors, tile_major)), ...] from the table's text."""
    out: dict = {}
    for ln, line in enumerate(text.splitlines(), 1):
        line = line.split("#", 1)[0].strip()
        if not line:
            continue
        f = line.split()
        if len(f) != 7:
            raise ValueError(f"skp tuning table line {ln}: 7 integers expected, got {line!r}")
        M, N, K, bm, bn, C, tm = (int(v) for v in f)
        why = check_plan(M, N, K, bm, bn, C)
        if why or tm not in (0, 1):
            raise ValueError(f"skp tuning table line {ln}: {why or 'tile_major is 0 or 1'}")
        out.setdefault((N, K), []).append((M, (bm, bn, C, tm)))
    return out


@functools.lru_cache(maxsize=1)
def _table() -> dict:
    if not os.path.exists(TUNING_FILE):
        return {}
    with open(TUNING_FILE) as f:
        return parse_table(f.read())


def lookup(table: dict, M: int, N: int, K: int) -> Optional[tuple]:
    """(bm, bn, contributors, tile_major) of the nearest measured M with the same number of
    128-row tiles, if the kernel can take it at this M; else None."""
    m128 = -(-M // 128)
    cands = [(abs(m - M), cfg) for m, cfg in table.get((N, K), ()) if -(-m // 128) == m128]
    if not cands:
        return None
    cfg = min(cands)[1]
    return None if check_plan(M, N, K, cfg[0], cfg[1], cfg[2]) else cfg


def plan(M: int, N: int, K: int) -> Optional[tuple]:
    """The measured gemm_skp plan of a residual projection, or None: gemm_sk keeps the shape."""
    if not enabled():
        return None
    return lookup(_table(), M, N, K)


_BOUND = False


def _lib():
    global _BOUND
    L = hip.lib()
    if not _BOUND:
        if not hasattr(L, "lsa_gemm_skp"):
            raise RuntimeError("liblsa_kernels.so has no lsa_gemm_skp: rebuild (python csrc/build.py)")
        vp, i = ctypes.c_void_p, ctypes.c_int
        L.lsa_gemm_skp.argtypes = [vp, i, vp, i, i, i, i, ctypes.POINTER(hip.EpiArgs), i, i, i, i, i, i, vp, vp,
                                   ctypes.c_longlong, i, vp]
        L.lsa_gemm_skp.restype = i
        _BOUND = True
    return L


def gemm_skp(a: torch.Tensor, wp: torch.Tensor, M: int, N: int, K: int, epi: int, ep, *, bm: int, bn: int,
             contributors: int, tile_major: int = 0, nb: int = 0, group_m: int = 8, ws=None) -> None:
    """C[M, N] = A[M, K] @ W^T (``wp`` = pack_b(W[N, K])) with every tile split ``contributors``
    ways over K and the fix-up shared by the contributors. ``ws``: a workspace with ``slab`` /
    ``counters`` (SkpWorkspace or hip.SkWorkspace; default: the stream's hip.SkWorkspace)."""
    hip._req(hip._is_bf16_cuda(a, wp), "gemm_skp: bf16 cuda tensors required")
    hip._req(wp.numel() == N * K and K % 64 == 0 and K >= 64, "gemm_skp: packed weight shape")
    hip._req(a.dim() == 2 and a.shape[0] >= M >= 1 and a.shape[1] >= K and a.stride(1) == 1 and a.stride(0) % 8 == 0
             and a.data_ptr() % 16 == 0, "gemm_skp: A must be [>=M, >=K] row-major with 16-B aligned rows")
    hip._req(epi in (hip.EPI_STORE, hip.EPI_RESID), "gemm_skp: EPI_STORE / EPI_RESID")
    hip._check_epi(epi, ep, N)
    why = check_plan(M, N, K, bm, bn, contributors)
    hip._req(why is None, f"gemm_skp: {why}")
    hip._req(tile_major in (0, 1) and nb in (0, 2, 3), "gemm_skp: tile_major 0 / 1, nb 0 / 2 / 3")
    if ws is None:
        ws = hip.default_sk_workspace(a.device)
    hip._req(ws.slab.numel() >= slab_floats(M, N, bm, bn, contributors) and
             ws.counters.numel() >= n_counters(M, N, bm, bn), f"gemm_skp: workspace too small for {bm}x{bn} x {contributors}")
    rc = _lib().lsa_gemm_skp(hip._p(a), a.stride(0), hip._p(wp), M, N, K, epi, ctypes.byref(ep), bm, bn, nb, contributors,
                             tile_major, group_m, hip._p(ws.slab), hip._p(ws.counters), ws.slab.numel(),
                             ws.counters.numel(), hip._stream())
    hip._check(rc, "lsa_gemm_skp")
