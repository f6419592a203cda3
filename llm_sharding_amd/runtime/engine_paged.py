"""PagedKVStageEngine: a StageEngine whose KV cache is a pool of 64-token pages behind one block
table (ops/kv_paged.py states the format; csrc/cache/kv_paged.hip holds the kernels).

``make_stage_engine(..., kv_layout="paged", kv_pages=N)`` (what ``inference.py --kv-layout paged``,
``serve.py --kv-layout paged`` and ``PipelineStage(kv_layout="paged")`` build) keeps, per layer,
``kp`` / ``vp`` bf16 ``[N, n_kv, 64, hd]`` and, for the whole engine, one int32 table
``[max_slots, max_seq / 64]``: a slot costs the pages its tokens fill, not ``max_seq``. Beside them
stands ONE bf16 staging layer of the shape of an ordinary layer cache (the fp8 KV engine's trick,
runtime/engine_kv8.py): ``k_cache[li]`` / ``v_cache[li]`` are that pair for every ``li``, so every
projection route and every EPI_QKV epilogue runs unchanged. Then, per layer:

* ``lsa_kvp_append`` copies the step's cells from the staging layer into their pages;
* decode rows (every forward without a tile table) attend the pages with ``lsa_attn_decode_paged``,
  always the split-KV kernels: where ``hip.attn`` would take the MFMA GQA kernel (a GQA model at
  512 or more (row, kv-head) items) the paged engine does not, so bitwise equality with the bf16
  engine holds for group 1 or fewer than 512 items;
* a flash-prefill forward first gathers ``[0, p0)`` of every slot whose tiles start at ``p0 > 0``
  back into the staging layer (``lsa_kvp_gather``) and then runs ``hip.attn_prefill`` unchanged.

The kernels do no arithmetic of their own, so the engine computes the bf16 engine's bits.

Pages are reserved on the host: ``kv_reserve(slot, n_tokens)`` / ``kv_release(slot)`` drive a
``PagePool`` and push only the changed table entries, on the current stream, so a captured graph
replayed afterwards sees them. Eager ``forward`` reserves up to ``max(pos) + 1`` per slot itself;
before a graph replay the caller reserves the positions the replay will write (a row whose entry is
null appends nothing and its key reads as zeros). ``reset`` releases.

Limits: Llama-family layers only, bf16 or fp8 weights, no fp8 pages, no KV fork / prefix pool (the
fork kernel copies static tensors), no fused attention + o projection launch, and not the
385-512-row gemm_skp route (runtime/engine_skp.py). On a CPU device the option is ignored.

It is a subclass for the reason engine_int4.py gives: runtime/engine.py is a recorded input of the
bf16 decode path's full-depth fixture (tests/fixture_hash.py) and stays as it is.
"""
from __future__ import annotations

from typing import Optional

import torch

from ..ops import kv_paged, packing
from .engine import StageEngine

KV_LAYOUTS = ("static", "paged")


class PagedKVStageEngine(StageEngine):
    kv_layout = "paged"

    def __init__(self, cfg, start: int, end: int, device="cpu", dtype=torch.bfloat16, *, kv_layout: str = "paged",
                 kv_pages: Optional[int] = None, weight_dtype: str = "bf16", kv_dtype: str = "bf16", **kw):
        if kv_layout != "paged":
            raise ValueError(f"PagedKVStageEngine holds a paged KV cache, got kv_layout={kv_layout!r}")
        check_kv_layout(kv_layout, kv_pages, weight_dtype, kv_dtype)
        self.paged = torch.device(device).type == "cuda"  # before the base constructor allocates the cache
        max_seq = int(min(kw.get("max_seq", 2048), cfg.max_position_embeddings))
        max_slots = int(kw.get("max_slots", 1))
        if self.paged:
            if cfg.is_gpt2:
                raise NotImplementedError("kv_layout='paged' is built for the Llama-family layer, not GPT-2")
            kv_paged.check_max_seq(max_seq)
            g = cfg.num_attention_heads // cfg.num_key_value_heads
            if cfg.head_dim not in kv_paged.KVP_HEAD_DIMS or g not in kv_paged.KVP_GROUPS:
                raise ValueError(f"kv_layout='paged' needs head_dim in {kv_paged.KVP_HEAD_DIMS} and a GQA group in "
                                 f"{kv_paged.KVP_GROUPS}, got head_dim={cfg.head_dim}, group={g}")
        # default: every slot can fill max_seq (no saving, but no reservation can fail)
        self.kv_n_pages = int(kv_pages) if kv_pages is not None else max_slots * (max_seq // kv_paged.PAGE) + 1
        self.pool: Optional[kv_paged.PagePool] = None
        self.kv_table = None
        self.kvp: list = []  # per layer: (kp, vp, table)
        super().__init__(cfg, start, end, device, dtype, weight_dtype=weight_dtype, **kw)

    def _alloc_runtime(self) -> None:
        if not self.paged:
            return super()._alloc_runtime()
        # the base allocates n_layers bf16 layer caches and nothing else by n_layers: one staging pair
        n = self.n_layers
        self.n_layers = 1
        try:
            super()._alloc_runtime()
        finally:
            self.n_layers = n
        self.k_cache, self.v_cache = self.k_cache * n, self.v_cache * n
        dev, (S, nkv, T, hd) = self.device, self.k_cache[0].shape
        self.pool = kv_paged.PagePool(self.kv_n_pages, S, T)
        self.kv_table = torch.zeros((S, T // kv_paged.PAGE), dtype=torch.int32, device=dev)
        shape = (self.kv_n_pages, nkv, kv_paged.PAGE, hd)
        self.kvp = [(torch.zeros(shape, dtype=torch.bfloat16, device=dev),
                     torch.zeros(shape, dtype=torch.bfloat16, device=dev), self.kv_table) for _ in range(n)]

    def memory_bytes(self) -> int:
        """Weights + the pages + the one bf16 staging layer + the block table."""
        if not self.paged:
            return super().memory_bytes()
        return (super().memory_bytes() + sum(t.numel() * t.element_size() for kp, vp, _ in self.kvp for t in (kp, vp))
                + self.kv_table.numel() * self.kv_table.element_size())

    def fork_slots(self, *a, **kw):
        raise NotImplementedError("KV fork on a paged KV cache: the fork kernel copies static tensors")

    kv_fork = fork_slots

    # ------------------------------------------------------------------------- pages
    def _kv_push(self, changed: list) -> None:
        """Copy the changed table entries to the device, on the current stream."""
        spans: dict = {}
        for s, i, _ in changed:
            a, b = spans.get(s, (i, i + 1))
            spans[s] = (min(a, i), max(b, i + 1))
        for s, (a, b) in spans.items():
            self.kv_table[s, a:b].copy_(self.pool.table[s, a:b])

    def kv_reserve(self, slot: int, n_tokens: int) -> None:
        """Pages for tokens [0, n_tokens) of ``slot`` (grows only). ``RuntimeError`` when the pool
        is short; nothing changes then. A static cache (CPU device) has nothing to reserve."""
        if self.paged:
            self._kv_push(self.pool.reserve(int(slot), int(n_tokens)))

    def kv_release(self, slot: int) -> None:
        """Return the slot's pages to the pool."""
        if self.paged:
            self._kv_push(self.pool.release(int(slot)))

    @property
    def kv_free_pages(self) -> int:
        return self.pool.free_pages if self.paged else 0

    def reset(self, slots=None) -> None:
        """Forget the KV contents of ``slots`` (all by default) and release their pages."""
        slots = list(range(self.max_slots) if slots is None else slots)
        super().reset(slots)
        for s in slots:
            self.kv_release(s)

    clear_kv = reset

    def forward(self, h: torch.Tensor, slot, pos, kv_len=None) -> torch.Tensor:
        """StageEngine.forward; the pages up to ``max(pos) + 1`` of every named slot are reserved
        first. That needs the positions on the host: ``slot`` / ``pos`` given as device tensors are
        read back (a host synchronisation on every eager call), and every slot that grows costs one
        small host-to-device copy of its new table entries. The captured decode path pays neither:
        its caller reserves ahead."""
        if self.paged:
            need: dict = {}
            sl = slot.tolist() if torch.is_tensor(slot) else list(slot)
            ps = pos.tolist() if torch.is_tensor(pos) else list(pos)
            for s, p in zip(sl, ps):
                if 0 <= s < self.max_slots and 0 <= p < self.max_seq:  # (other rows write nothing)
                    need[s] = max(need.get(s, 0), int(p) + 1)
            for s, n in sorted(need.items()):
                self.kv_reserve(s, n)
        return super().forward(h, slot, pos, kv_len)

    @staticmethod
    def _kvp_prefix_jobs(tiles) -> list:
        """(slot, p0) of every slot whose flash-prefill tiles start at p0 > 0: the prefix the
        staging layer must hold before the chunk's attention (``tiles[0]``: the host tile table
        [row0, nrows, slot, pos0, kvlen, ...] of hip.build_prefill_tiles)."""
        if tiles is None:
            return []
        first = {}
        for _, _, s, p0, *_ in tiles[0].tolist():
            first[s] = min(p0, first.get(s, p0))
        return [(s, p0) for s, p0 in sorted(first.items()) if p0 > 0]

    # ------------------------------------------------------------------------- HIP path
    # _forward_hip is StageEngine's, statement for statement, except for the lines that name kv_paged
    # (the prefix gather, the append after the QKV projection, the decode attention) and the
    # attn_oproj switch. tests/test_kv_paged.py pins that the two bodies differ in those lines only,
    # so a change of the base forward fails until it is carried over.
    def _forward_hip(self, h, slot, pos, kv_len, rows, nsplit: Optional[int] = None, tiles=None) -> torch.Tensor:
        from ..ops import hip
        cfg = self.cfg
        H, I, eps = cfg.hidden_size, cfg.intermediate_size, cfg.rms_norm_eps
        nh, nkv, hd = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim
        if rows > self.max_prefill_rows and rows > self.DECODE_MAX_ROWS:
            raise ValueError(f"{rows} rows exceed max_prefill_rows={self.max_prefill_rows}")
        if h.dtype != torch.bfloat16 or not h.is_contiguous():
            h = h.to(torch.bfloat16).contiguous()
        hbuf = self.buf_h[:rows]
        if h.data_ptr() != hbuf.data_ptr():
            hbuf.copy_(h)
        decode = rows <= self.DECODE_MAX_ROWS
        if nsplit is None and tiles is None:
            kv_max = self.max_seq if decode else (int(pos.max().item()) + 1 if kv_len is None else int(kv_len.max().item()))
            nsplit = self._attn_nsplit(rows, kv_max)
        q, attn_o, act, xn = self.buf_q[:rows], self.buf_attn[:rows], self.buf_act[:rows], self.buf_xn[:rows]
        ws = self.coop_ws
        native_fp8 = self.fp8 and rows <= packing.GEMV_MAX_ROWS
        if cfg.is_gpt2:
            return self._forward_hip_gpt2(hbuf, slot, pos, kv_len, rows, nsplit, tiles, decode, native_fp8)

        def wbf(w, s, N, K):  # packed bf16 weights (fp8 -> scratch for the >64-row kernels)
            return w if s is None else hip.dequant_fp8_packed(w.view(-1), s, self.w_scratch, N, K)

        def dec(x, w, s, N, K, epi, ep, norm=False):
            if native_fp8:
                hip.proj_fp8(x, w.view(-1), s, rows, N, K, epi, ep, norm=norm, eps=eps, ws=ws)
            else:
                hip.gemv(x, wbf(w, s, N, K), rows, N, K, epi, ep, norm=norm, eps=eps, ws=ws)

        def dec_resid(x, w, s, N, K, ep):
            # 17..128 rows: split-K partials + one residual-add kernel where measured faster than
            # the coop kernel's in-kernel split reduction (ops/gemv_tuning.json "coop_partial")
            pc = None if (native_fp8 or s is not None or cfg.is_gpt2 or N not in (2048, 4096, 6144, 8192)) \
                else packing.partial_config(N // 16, rows, k=K)
            if pc is None or ws.slab.numel() < pc[3] * rows * N:
                dec(x, w, s, N, K, hip.EPI_RESID, ep)
                return
            part = ws.slab[:pc[3] * rows * N].view(pc[3], rows, N)
            hip.gemv(x, w, rows, N, K, hip.EPI_PARTIAL, hip.make_epi(out=part, ldo=N), coop=pc, ws=ws,
                     out_numel=part.numel())
            hip.resid_rmsnorm_partials(hbuf, part, pc[3], rows, eps)

        def pre(x, w, s, N, K, epi, ep):
            hip.gemm(x, wbf(w, s, N, K), rows, N, K, epi, ep, ws=ws, sk_ws=self.sk_ws)

        # residual projections as split-K partials summed by the next norm kernel, where measured
        # faster than the fused residual epilogue (ops/gemm_sk_tuning.json "partial" entries)
        # the projection kernel family: the weight-streaming GEMVs up to GEMV_MAX_ROWS rows, the
        # LDS-DMA MFMA GEMMs (gemm_sk / gemm_wr) above - independent of the attention's decode mode
        proj_gemm = (not decode) or (rows > self.GEMV_MAX_ROWS and not native_fp8 and self.sk_ws is not None)
        part_ok = proj_gemm and self.part_k is not None and rows <= self.part_k.shape[1]

        def resid_proj(x, w, s, N, K, ep):
            # returns the split count of partials left in part_k (0: residual applied in-GEMM)
            pp = hip.gemm_sk_partial_plan(rows, N, K) if part_ok else None
            if pp is None:
                pre(x, w, s, N, K, hip.EPI_RESID, ep)
                return 0
            bn, sp = pp
            hip.gemm_sk(x, wbf(w, s, N, K), rows, N, K, hip.EPI_PARTIAL, hip.make_epi(out=self.part_k, ldo=N),
                        bn=bn, grid=hip.N_CU, dp=0, split=sp, ws=self.sk_ws, out_numel=self.part_k.numel())
            return sp

        # RMSNorm fused across the GEMMs: residual GEMMs write per-64-column sums of squares of
        # their outputs (ss), the qkv / gate_up GEMMs read the raw residual stream and scale each
        # row by its rstd in the epilogue - no standalone norm kernel between projections
        fuse = proj_gemm and self.ss_buf is not None and rows <= self.ss_buf.shape[0]
        ss = self.ss_buf[:rows] if fuse else None
        # one decode row, one split: attention + o projection + residual in one launch
        ao = False  # kv_paged: attn_oproj reads a bf16 static cache
        kvp_jobs = self._kvp_prefix_jobs(tiles)
        ss_valid = False  # ss holds the partials of hbuf's current values
        pending = 0  # down-projection partials not yet added to hbuf
        for li, lw in enumerate(self.layers):
            kc, vc = self.k_cache[li], self.v_cache[li]
            if kvp_jobs:
                kv_paged.kvp_gather(*self.kvp[li], kc, vc, kvp_jobs)
            ep_qkv = hip.make_epi(out=q, k_cache=kc, v_cache=vc, slot=slot, pos=pos, cos=self.cos, sin=self.sin,
                                  ldo=q.stride(0), n_heads=nh, n_kv=nkv, head_dim=hd, t_max=self.max_seq)
            if not proj_gemm:
                dec(hbuf, lw.qkv, lw.qkv_s, cfg.qkv_size, H, hip.EPI_QKV, ep_qkv, norm=True)
            else:
                if pending and not fuse:
                    hip.resid_rmsnorm_partials(hbuf, self.part_k, pending, rows, eps, out=xn)
                    pending = 0
                    pre(xn, lw.qkv, lw.qkv_s, cfg.qkv_size, H, hip.EPI_QKV, ep_qkv)
                elif fuse:
                    if pending:  # the previous down projection left K-split partials: add them
                        hip.resid_rmsnorm_partials(hbuf, self.part_k, pending, rows, eps)
                        pending = 0
                    if not ss_valid:
                        # (also at a stage's first layer: the same partials, in the same order, as
                        # a residual GEMM epilogue writes - a layer range computes the same bits
                        # whichever stage it starts)
                        hip.row_ss(hbuf, rows, ss)
                    ep_qkv = hip.make_epi(out=q, k_cache=kc, v_cache=vc, slot=slot, pos=pos, cos=self.cos,
                                          sin=self.sin, ldo=q.stride(0), n_heads=nh, n_kv=nkv, head_dim=hd,
                                          t_max=self.max_seq, ss_in=ss, ss_eps=eps)
                    pre(hbuf, lw.qkv, lw.qkv_s, cfg.qkv_size, H, hip.EPI_QKV, ep_qkv)
                else:
                    hip.rmsnorm(hbuf, None, xn, rows, eps, H)
                    pre(xn, lw.qkv, lw.qkv_s, cfg.qkv_size, H, hip.EPI_QKV, ep_qkv)
            kv_paged.kvp_append(kc, vc, *self.kvp[li], slot, pos, rows)
            ep_o = hip.make_epi(out=hbuf, resid=hbuf, ldo=hbuf.stride(0), ldr=hbuf.stride(0))
            fused_o = ao and lw.o_s is None and hip.attn_oproj(q, kc, vc, slot, pos, nh, nkv, hd, attn_o, lw.o, H, ep_o,
                                                               self.ao_sync, kv_len=kv_len)
            if tiles is not None:
                hip.attn_prefill(q, kc, vc, tiles[1], nh, nkv, hd, attn_o, causal=kv_len is None, tiles_host=tiles[0])
            elif not fused_o:
                kv_paged.attn(q, *self.kvp[li], slot, pos, rows, nh, nkv, hd, nsplit, self.part_o, self.part_lse, attn_o,
                         kv_len=kv_len, counters=self.attn_cnt, min_chunk=self.ATTN_MIN_CHUNK)
            ep_gu = hip.make_epi(out=act, ldo=act.stride(0))
            if not proj_gemm:
                if not fused_o:
                    dec_resid(attn_o, lw.o, lw.o_s, H, cfg.q_size, ep_o)
                dec(hbuf, lw.gate_up, lw.gate_up_s, 2 * I, H, hip.EPI_SWIGLU, ep_gu, norm=True)
                dec_resid(act, lw.down, lw.down_s, H, I, ep_o)
            else:
                ep_r = hip.make_epi(out=hbuf, resid=hbuf, ldo=hbuf.stride(0), ldr=hbuf.stride(0), ss_out=ss) \
                    if fuse else ep_o
                sp = resid_proj(attn_o, lw.o, lw.o_s, H, cfg.q_size, ep_r)
                if sp:
                    hip.resid_rmsnorm_partials(hbuf, self.part_k, sp, rows, eps, out=xn)
                    pre(xn, lw.gate_up, lw.gate_up_s, 2 * I, H, hip.EPI_SWIGLU, ep_gu)
                elif fuse:
                    pre(hbuf, lw.gate_up, lw.gate_up_s, 2 * I, H, hip.EPI_SWIGLU,
                        hip.make_epi(out=act, ldo=act.stride(0), ss_in=ss, ss_eps=eps))
                else:
                    hip.rmsnorm(hbuf, None, xn, rows, eps, H)
                    pre(xn, lw.gate_up, lw.gate_up_s, 2 * I, H, hip.EPI_SWIGLU, ep_gu)
                pending = resid_proj(act, lw.down, lw.down_s, H, I, ep_r)
                ss_valid = fuse and not pending
        if pending:  # the stage's output residual stream
            hip.resid_rmsnorm_partials(hbuf, self.part_k, pending, rows, eps)
        return hbuf



def check_kv_layout(kv_layout: str, kv_pages=None, weight_dtype: str = "bf16", kv_dtype: str = "bf16") -> None:
    """The option's value check, the same on every device."""
    if kv_layout not in KV_LAYOUTS:
        raise ValueError(f"kv_layout must be one of {KV_LAYOUTS}, got {kv_layout!r}")
    if kv_layout == "static":
        if kv_pages is not None:
            raise ValueError("kv_pages needs kv_layout='paged'")
        return
    if weight_dtype == "int4":
        raise ValueError("kv_layout='paged' with weight_dtype='int4' is not built: int4 weights have a forward body "
                         "of their own (runtime/engine_int4.py)")
    if kv_dtype != "bf16":
        raise ValueError(f"kv_layout='paged' holds bf16 pages: kv_dtype={kv_dtype!r} together with paged is not built")
    if kv_pages is not None and int(kv_pages) < 2:
        raise ValueError(f"kv_layout='paged' needs kv_pages >= 2 (page 0 is the null page), got {kv_pages}")
