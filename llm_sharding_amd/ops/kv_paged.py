"""Paged KV cache (kv_layout="paged"): the format, its page allocator, its torch references and the
bindings of csrc/cache/kv_paged.hip.

A layer's cache is two tensors ``kp`` / ``vp`` bf16 ``[n_pages, n_kv, PAGE, hd]``; the engine holds
ONE block table for all its layers, int32 ``[max_slots, max_seq / PAGE]`` on the device. Token ``t``
of slot ``s`` lives in page ``table[s, t // PAGE]`` at offset ``t % PAGE``.

``PAGE = 64`` tokens, fixed: a multiple of every decode kernel's keys per wave-instruction (4 / 8)
and keys per workgroup iteration (16 / 32 / 64); a (page, kv-head) run is 8 / 16 KiB of contiguous
bf16, the run the static cache gives the streams; a sequence wastes 63 tokens at most.

Page 0 is the null page. Every unassigned entry is 0, :class:`PagePool` never hands page 0 out and
no kernel writes it, so it stays zero. An entry outside ``[1, n_pages)`` is read as 0 by every
kernel and every reference here, so no table can address memory outside the pool. The kernels only
read the table; all table writes are host-to-device copies.

This module stands beside ops/hip.py as ops/kv8.py does: hip.py is a recorded input of the bf16
decode path's full-depth fixture (tests/fixture_hash.py)."""
from __future__ import annotations

import ctypes
import heapq
import os
from typing import Optional

import torch

from . import hip

PAGE = 64
KVP_HEAD_DIMS = (64, 128)
KVP_GROUPS = (1, 2, 3, 4, 6, 8)  # GQA group sizes the decode attention is built for
KVP_MAX_SPLIT = 16
KVP_MAX_JOBS = 256


def pages_for(n_tokens: int) -> int:
    """Pages that hold ``n_tokens`` tokens of one sequence."""
    return -(-max(int(n_tokens), 0) // PAGE)


def check_max_seq(max_seq: int) -> None:
    if max_seq < PAGE or max_seq % PAGE:
        raise ValueError(f"kv_layout='paged' needs max_seq to be a multiple of the page ({PAGE} tokens), got {max_seq}")


# ------------------------------------------------------------------------------ allocator (pure Python)
class PagePool:
    """Allocator over a CPU int32 mirror of the block table. No device dependency: whoever owns the
    device table pushes the ``(slot, index, page)`` triples that :meth:`reserve` / :meth:`release`
    return. The lowest-numbered free pages go first, so runs reproduce."""

    def __init__(self, n_pages: int, max_slots: int, max_seq: int):
        check_max_seq(max_seq)
        if n_pages < 2:
            raise ValueError(f"a page pool needs kv_pages >= 2 (page 0 is the null page), got {n_pages}")
        if max_slots < 1:
            raise ValueError(f"a page pool needs max_slots >= 1, got {max_slots}")
        self.n_pages, self.max_slots, self.max_seq = int(n_pages), int(max_slots), int(max_seq)
        self.table = torch.zeros((self.max_slots, self.max_seq // PAGE), dtype=torch.int32)
        self._free = list(range(1, self.n_pages))  # a heap: an ascending list is one
        self._held = [0] * self.max_slots          # pages per slot: entries [0, held) are assigned

    pages_for = staticmethod(pages_for)

    @property
    def free_pages(self) -> int:
        return len(self._free)

    def pages_of(self, slot: int) -> list:
        return self.table[slot, :self._held[slot]].tolist()

    def reserve(self, slot: int, n_tokens: int) -> list:
        """Make the slot's entries cover tokens ``[0, n_tokens)``; grows only. Returns the changed
        ``(slot, index, page)`` triples. Raises ``RuntimeError`` (and changes nothing) when the pool
        is short, ``ValueError`` for a slot or length outside the table."""
        if not 0 <= slot < self.max_slots:
            raise ValueError(f"slot {slot} outside [0, {self.max_slots})")
        if n_tokens > self.max_seq:
            raise ValueError(f"{n_tokens} tokens exceed max_seq={self.max_seq}")
        have, need = self._held[slot], pages_for(n_tokens)
        if need <= have:
            return []
        if need - have > len(self._free):
            raise RuntimeError(f"page pool exhausted: slot {slot} needs {need - have} more pages for {n_tokens} "
                               f"tokens, {len(self._free)} of {self.n_pages - 1} are free")
        out = []
        for i in range(have, need):
            pg = heapq.heappop(self._free)
            self.table[slot, i] = pg
            out.append((slot, i, pg))
        self._held[slot] = need
        return out

    def release(self, slot: int) -> list:
        """Return the slot's pages to the pool and zero its row. Returns the changed triples."""
        if not 0 <= slot < self.max_slots:
            raise ValueError(f"slot {slot} outside [0, {self.max_slots})")
        n = self._held[slot]
        for pg in self.table[slot, :n].tolist():
            heapq.heappush(self._free, pg)
        self.table[slot, :n] = 0
        self._held[slot] = 0
        return [(slot, i, 0) for i in range(n)]


# ------------------------------------------------------------------------------ references (any device)
def sanitize_table(table: torch.Tensor, n_pages: int) -> torch.Tensor:
    """The table as the kernels read it: an entry outside [1, n_pages) is the null page."""
    return torch.where((table >= 1) & (table < n_pages), table, torch.zeros_like(table))


def _check_pool(kp: torch.Tensor, vp: torch.Tensor, table: torch.Tensor, what: str) -> tuple:
    if kp.dim() != 4 or kp.shape != vp.shape or kp.shape[2] != PAGE or kp.dtype != vp.dtype:
        raise ValueError(f"{what}: kp / vp [n_pages, n_kv, {PAGE}, hd]")
    if kp.shape[0] < 2:
        raise ValueError(f"{what}: a pool has at least 2 pages")
    if table.dtype != torch.int32 or table.dim() != 2 or table.shape[1] < 1:
        raise ValueError(f"{what}: table int32 [max_slots, max_seq / {PAGE}]")
    return tuple(kp.shape)


def append_reference(k_stage: torch.Tensor, v_stage: torch.Tensor, kp: torch.Tensor, vp: torch.Tensor,
                     table: torch.Tensor, slot, pos) -> None:
    """``lsa_kvp_append`` in torch: copies staging cell (slot[m], :, pos[m], :) into its page, in
    place. A row with slot / pos outside the cache or a null entry writes nothing."""
    n_pages = _check_pool(kp, vp, table, "append_reference")[0]
    S, T = table.shape[0], table.shape[1] * PAGE
    tab = sanitize_table(table, n_pages)
    for s, p in zip([int(x) for x in slot], [int(x) for x in pos]):
        if not (0 <= s < S and 0 <= p < T):
            continue
        pg = int(tab[s, p // PAGE])
        if pg == 0:
            continue
        kp[pg, :, p % PAGE] = k_stage[s, :, p]
        vp[pg, :, p % PAGE] = v_stage[s, :, p]


def gather_reference(kp: torch.Tensor, vp: torch.Tensor, table: torch.Tensor, k_stage: torch.Tensor,
                     v_stage: torch.Tensor, jobs) -> None:
    """``lsa_kvp_gather`` in torch: positions [0, len) of every (slot, len) job go from the pages
    into the staging layer, in place; a null entry restores zeros."""
    n_pages = _check_pool(kp, vp, table, "gather_reference")[0]
    tab = sanitize_table(table, n_pages)
    for s, n in jobs:
        if n == 0:
            continue
        idx = tab[s, :pages_for(n)].long().to(kp.device)
        k_stage[s, :, :n] = kp[idx].transpose(0, 1).reshape(kp.shape[1], -1, kp.shape[3])[:, :n]
        v_stage[s, :, :n] = vp[idx].transpose(0, 1).reshape(vp.shape[1], -1, vp.shape[3])[:, :n]


def to_static(kp: torch.Tensor, vp: torch.Tensor, table: torch.Tensor, lens=None) -> tuple:
    """The static ``[max_slots, n_kv, max_seq, hd]`` pair a table describes (every slot gathered in
    full, or up to ``lens[s]``): what an attention reference reads."""
    _check_pool(kp, vp, table, "to_static")
    S, T = table.shape[0], table.shape[1] * PAGE
    k = torch.zeros((S, kp.shape[1], T, kp.shape[3]), dtype=kp.dtype, device=kp.device)
    v = torch.zeros_like(k)
    gather_reference(kp, vp, table, k, v, [(s, T if lens is None else int(lens[s])) for s in range(S)])
    return k, v


# ------------------------------------------------------------------------------ bindings
_L = None


def _lib():
    """The kernel library with the paged entry points' signatures declared."""
    global _L
    if _L is None:
        L = hip.lib()
        if not hasattr(L, "lsa_attn_decode_paged"):
            raise RuntimeError("the kernel library has no lsa_attn_decode_paged: rebuild it (python csrc/build.py)")
        vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
        L.lsa_attn_decode_paged.argtypes = [vp, i, vp, vp, vp, i, vp, vp, vp, i, i, i, i, i, f, i, i, i, vp, vp, vp, i,
                                            vp, vp]
        L.lsa_kvp_append.argtypes = [vp, vp, vp, vp, vp, vp, vp, i, i, i, i, i, i, vp]
        L.lsa_kvp_gather.argtypes = [vp, vp, vp, vp, vp, vp, i, i, i, i, i, i, vp]
        for name in ("lsa_attn_decode_paged", "lsa_kvp_append", "lsa_kvp_gather"):
            getattr(L, name).restype = i
        _L = L
    return _L


def _check(rc: int, what: str) -> None:
    if rc == 1:  # LSA_BAD_SHAPE
        raise ValueError(f"{what}: shape or argument outside what the kernel is built for")
    hip._check(rc, what)


def small_max_wgs() -> int:
    """rows * n_kv up to which a one-split decode attention takes the 8-wave one-trip kernel: the
    value ops/hip.py hands the static launcher (LSA_ATTN_SMALL_MAX_WGS, default 128)."""
    return int(os.environ.get("LSA_ATTN_SMALL_MAX_WGS", "128"))


def _check_dev_pool(kp, vp, table, what: str) -> tuple:
    hip._req(hip._is_bf16_cuda(kp, vp) and kp.is_contiguous() and vp.is_contiguous(), f"{what}: contiguous bf16 cuda pages")
    hip._req(table is not None and torch.is_tensor(table) and table.is_cuda and table.is_contiguous(),
             f"{what}: a contiguous cuda block table")
    shape = _check_pool(kp, vp, table, what)
    hip._req(shape[3] in KVP_HEAD_DIMS, f"{what}: head_dim {shape[3]} not built {KVP_HEAD_DIMS}")
    return shape


def _check_stage(k_stage, v_stage, table, shape: tuple, what: str) -> tuple:
    want = (table.shape[0], shape[1], table.shape[1] * PAGE, shape[3])
    hip._req(hip._is_bf16_cuda(k_stage, v_stage) and k_stage.is_contiguous() and v_stage.is_contiguous(),
             f"{what}: contiguous bf16 cuda staging tensors")
    hip._req(tuple(k_stage.shape) == want and tuple(v_stage.shape) == want,
             f"{what}: the staging layer is [max_slots, n_kv, max_seq, hd] = {want}")
    return want


def kvp_append(k_stage: torch.Tensor, v_stage: torch.Tensor, kp: torch.Tensor, vp: torch.Tensor, table: torch.Tensor,
               slot: torch.Tensor, pos: torch.Tensor, rows: int) -> None:
    """Copy the K / V vectors at (slot[m], h, pos[m], :) of the bf16 staging layer into their pages,
    m < rows. A row with slot / pos outside the cache or a null table entry writes nothing. The rows
    of one call name distinct cells. ``slot`` / ``pos`` / ``table`` are read on the device."""
    shape = _check_dev_pool(kp, vp, table, "kvp_append")
    S, nkv, T, hd = _check_stage(k_stage, v_stage, table, shape, "kvp_append")
    hip._req(slot.is_cuda and pos.is_cuda and slot.dtype == torch.int32 and pos.dtype == torch.int32,
             "kvp_append: int32 cuda slot/pos")
    hip._req(1 <= rows <= slot.numel() and rows <= pos.numel(), "kvp_append: rows")
    rc = _lib().lsa_kvp_append(hip._p(k_stage), hip._p(v_stage), hip._p(kp), hip._p(vp), hip._p(table), hip._p(slot),
                               hip._p(pos), rows, S, nkv, hd, T, shape[0], hip._stream())
    _check(rc, "lsa_kvp_append")


def kvp_gather(kp: torch.Tensor, vp: torch.Tensor, table: torch.Tensor, k_stage: torch.Tensor, v_stage: torch.Tensor,
               jobs) -> None:
    """``jobs``: host pairs (slot, len). Copies positions [0, len) of every kv-head of those slots
    from the pages into the staging layer (zeros where an entry is null), nothing else."""
    shape = _check_dev_pool(kp, vp, table, "kvp_gather")
    S, nkv, T, hd = _check_stage(k_stage, v_stage, table, shape, "kvp_gather")
    jobs = [(int(s), int(n)) for s, n in jobs]
    for s, n in jobs:
        hip._req(0 <= s < S and 0 <= n <= T, f"kvp_gather: job {(s, n)} outside the cache {(S, T)}")
    hip._req(len({s for s, _ in jobs}) == len(jobs), "kvp_gather: a slot named twice")
    if not jobs:
        return
    arr = (ctypes.c_int * (2 * len(jobs)))(*[x for j in jobs for x in j])
    rc = _lib().lsa_kvp_gather(hip._p(kp), hip._p(vp), hip._p(table), hip._p(k_stage), hip._p(v_stage),
                               ctypes.cast(arr, ctypes.c_void_p), len(jobs), S, nkv, hd, T, shape[0], hip._stream())
    _check(rc, "lsa_kvp_gather")


def attn_paged(q: torch.Tensor, kp: torch.Tensor, vp: torch.Tensor, table: torch.Tensor, slot: torch.Tensor,
               pos: torch.Tensor, rows: int, n_heads: int, n_kv: int, head_dim: int, nsplit: int,
               part_o: Optional[torch.Tensor], part_lse: Optional[torch.Tensor], out: torch.Tensor,
               kv_len: Optional[torch.Tensor] = None, min_chunk: int = 64, scale: Optional[float] = None,
               counters: Optional[torch.Tensor] = None) -> None:
    """``lsa_attn_decode`` over pages (csrc/cache/kv_paged.hip): :func:`hip.attn`'s arguments and
    semantics with (kp, vp, table) in place of the static caches, and always the split-KV VALU
    kernels (never the MFMA GQA kernel, which does not read pages). ``counters``: >= rows * n_kv
    zeroed int32, left zeroed (default: the stream's coop workspace)."""
    hip._req(table is not None, "attn_paged: a block table")
    shape = _check_dev_pool(kp, vp, table, "attn_paged")
    hip._req(hip._is_bf16_cuda(q, out), "attn_paged: bf16 cuda q / out")
    hip._req(shape[1] == n_kv and shape[3] == head_dim, "attn_paged: page dims")
    hip._req(n_kv >= 1 and n_heads % n_kv == 0 and (n_heads // n_kv) in KVP_GROUPS,
             f"attn_paged: GQA group {n_heads}/{n_kv} not built {KVP_GROUPS}")
    hip._req(rows >= 1 and q.dim() == 2 and q.shape[0] >= rows and q.shape[1] >= n_heads * head_dim
             and q.stride(1) == 1 and q.stride(0) % 8 == 0, "attn_paged: q shape")
    hip._req(out.dim() == 2 and out.shape[0] >= rows and out.shape[1] >= n_heads * head_dim and out.stride(1) == 1,
             "attn_paged: out shape")
    hip._req(1 <= nsplit <= KVP_MAX_SPLIT and min_chunk >= 1, "attn_paged: nsplit 1..16, min_chunk >= 1")
    hip._req(slot.is_cuda and pos.is_cuda and slot.dtype == torch.int32 and pos.dtype == torch.int32
             and slot.numel() >= rows and pos.numel() >= rows, "attn_paged: int32 cuda slot/pos")
    hip._req(kv_len is None or (kv_len.is_cuda and kv_len.dtype == torch.int32 and kv_len.numel() >= rows),
             "attn_paged: int32 cuda kv_len")
    if nsplit > 1:
        hip._req(part_o is not None and part_lse is not None and part_o.dtype == torch.float32
                 and part_lse.dtype == torch.float32 and part_o.numel() >= rows * n_heads * nsplit * head_dim
                 and part_lse.numel() >= rows * n_heads * nsplit, "attn_paged: fp32 workspace too small")
        if counters is None:
            counters = hip.default_workspace(q.device).counters
        hip._req(counters.dtype == torch.int32 and counters.numel() >= rows * n_kv, "attn_paged: counters too small")
    sc = head_dim ** -0.5 if scale is None else scale
    rc = _lib().lsa_attn_decode_paged(hip._p(q), q.stride(0), hip._p(kp), hip._p(vp), hip._p(table), shape[0],
                                      hip._p(slot), hip._p(pos), hip._p(kv_len), rows, n_heads, n_kv, head_dim,
                                      table.shape[1] * PAGE, float(sc), nsplit, min_chunk, small_max_wgs(),
                                      hip._p(part_o), hip._p(part_lse), hip._p(out), out.stride(0),
                                      hip._p(counters) if nsplit > 1 else None, hip._stream())
    _check(rc, "lsa_attn_decode_paged")


attn = attn_paged  # (the engine's call reads as hip.attn's: runtime/engine_paged.py)
