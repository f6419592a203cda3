"""Int4StageEngine: a StageEngine whose layer projections stay int4 on the device (W4A16).

``make_stage_engine(..., weight_dtype="int4")`` (what ``inference.py --weight-dtype int4`` and
``PipelineStage(weight_dtype="int4")`` build) keeps the four projections of every layer as
symmetric group-128 int4 with fp32 group scales - 4.25 bits per weight (ops/int4.py). Decode
batches of up to 64 rows stream them through csrc/quant/gemv_int4.hip; larger row counts
dequantise one projection at a time into ``w_scratch`` and run the bf16 kernels (the cooperative
GEMV up to ``GEMV_MAX_ROWS`` rows, the GEMMs above and for prefill, with the same fused-norm and
split-K-partial routes), as the fp8 engine does.

The lm_head, the embedding and the norms stay bf16 (``lm_head_s`` stays None), so ``head``,
``Sampler``, the logit stages and ``score_prompt`` are the bf16 engine's, unchanged. Each fused
matrix is quantised here with its RMSNorm weight folded in - which is why an int4 shard's own
nibbles cannot be passed straight through: a group's scale depends on the folded columns, so
shards are dequantised at load (models/weights.py) and re-quantised.

On a CPU device the option is ignored, as fp8 is: the engine computes with the unquantised weights.

It is a subclass, not a branch inside StageEngine: runtime/engine.py is a recorded input of the
bf16 decode path's full-depth fixture (tests/fixture_hash.py) and stays as it is.
"""
from __future__ import annotations

from typing import Optional

import torch

from ..ops import int4, packing
from .engine import StageEngine

PROJ = ("qkv", "o", "gate_up", "down")


class Int4StageEngine(StageEngine):
    def __init__(self, cfg, start: int, end: int, device="cpu", dtype=torch.bfloat16, *, weight_dtype: str = "int4",
                 **kw):
        if weight_dtype != "int4":
            raise ValueError(f"Int4StageEngine holds int4 weights, got weight_dtype={weight_dtype!r}")
        self.int4 = torch.device(device).type == "cuda"  # before the base constructor loads the weights
        if self.int4:
            for name, (n, k) in zip(PROJ, self.proj_shapes(cfg)):
                if k % int4.INT4_GROUP:
                    raise ValueError(f"weight_dtype='int4' needs K % {int4.INT4_GROUP} == 0: the {name} projection "
                                     f"has K={k}")
        super().__init__(cfg, start, end, device, dtype, weight_dtype="bf16", **kw)

    # ------------------------------------------------------------------------- loading
    def _prepare_layer(self, lw: dict):
        """The base engine's fused, norm-folded, packed bf16 matrices, re-quantised: packed
        nibbles [N*K/2] in the LayerWeights slots, packed scales S[N/16][K/128][16] beside them."""
        out = super()._prepare_layer(lw)
        if not self.int4:
            return out
        for name in PROJ:
            q, sc = int4.quantize_int4_groups(packing.unpack_b(getattr(out, name)))
            setattr(out, name, int4.pack_b_int4(q))
            setattr(out, name + "_s", int4.pack_scales_int4(sc))
        return out

    def _alloc_runtime(self) -> None:
        super()._alloc_runtime()
        if self.int4:  # one projection's bf16 weights, for the > 64-row paths
            shapes = self.proj_shapes(self.cfg)
            self.w_scratch = torch.empty(max(n * k for n, k in shapes), dtype=torch.bfloat16, device=self.device)

    # ------------------------------------------------------------------------- HIP path
    # _forward_hip / _forward_hip_gpt2 are StageEngine's, statement for statement, with the three
    # weight closures (wbf, dec, pre; GPT-2: proj) dispatching on the int4 weights: native kernel up
    # to 64 rows, else dequantise into w_scratch and the SAME bf16 route the base engine takes for
    # that row count (cooperative GEMV, gemm_sk with the fused RMSNorm sums and the split-K
    # partial residuals, gemm_wr), as its fp8 weights do. tests/test_int4.py pins that the two
    # bodies differ in those closures only, so a change of the base forward fails until it is
    # carried over.
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
        native_fp8 = False  # int4 weights: the name stays so that the rest of the body is the base engine's
        native_int4 = rows <= int4.INT4_MAX_ROWS
        if cfg.is_gpt2:
            return self._forward_hip_gpt2(hbuf, slot, pos, kv_len, rows, nsplit, tiles, decode, native_int4)
        wbf = self._weights_bf16  # packed bf16 weights (int4 -> scratch for the larger-row kernels)

        def dec(x, w, s, N, K, epi, ep, norm=False):
            if native_int4:
                int4.gemv_int4(x, w, s, rows, N, K, epi, ep, norm=norm, eps=eps)
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
        ao = (self.ATTN_OPROJ and rows == 1 and tiles is None and nsplit == 1 and not proj_gemm and not native_fp8
              and self.ao_sync is not None)
        ss_valid = False  # ss holds the partials of hbuf's current values
        pending = 0  # down-projection partials not yet added to hbuf
        for li, lw in enumerate(self.layers):
            kc, vc = self.k_cache[li], self.v_cache[li]
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
            ep_o = hip.make_epi(out=hbuf, resid=hbuf, ldo=hbuf.stride(0), ldr=hbuf.stride(0))
            fused_o = ao and lw.o_s is None and hip.attn_oproj(q, kc, vc, slot, pos, nh, nkv, hd, attn_o, lw.o, H, ep_o,
                                                               self.ao_sync, kv_len=kv_len)
            if tiles is not None:
                hip.attn_prefill(q, kc, vc, tiles[1], nh, nkv, hd, attn_o, causal=kv_len is None, tiles_host=tiles[0])
            elif not fused_o:
                hip.attn(q, kc, vc, slot, pos, rows, nh, nkv, hd, nsplit, self.part_o, self.part_lse, attn_o,
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

    def _weights_bf16(self, w, s, N, K):
        """A projection's packed bf16 weights: ``w`` itself, or the int4 tensor dequantised
        into ``w_scratch`` (one projection at a time, consumed by the next launch on the stream)."""
        return w if s is None else int4.dequant_int4_packed(w, s, self.w_scratch, N, K)

    def _forward_hip_gpt2(self, hbuf, slot, pos, kv_len, rows, nsplit, tiles, decode, native_int4) -> torch.Tensor:
        """GPT-2 layer on the HIP path: LayerNorm kernel (ln_1, with the wpe add fused in front
        of layer 0) -> QKV projection + bias + KV-cache append (no RoPE) -> attention ->
        c_proj + bias + residual -> LayerNorm (ln_2) -> c_fc + bias + GELU -> mlp.c_proj + bias
        + residual. Decode rows use the GEMV / coop / fp8 kernels, prefill rows the MFMA GEMM."""
        from ..ops import hip
        cfg = self.cfg
        H, I, eps = cfg.hidden_size, cfg.intermediate_size, cfg.rms_norm_eps
        nh, nkv, hd = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim
        q, attn_o, act, xn = self.buf_q[:rows], self.buf_attn[:rows], self.buf_act[:rows], self.buf_xn[:rows]
        ws = self.coop_ws

        def proj(x, w, s, N, K, epi, ep):
            if decode and native_int4:
                int4.gemv_int4(x, w, s, rows, N, K, epi, ep)
                return
            wb = self._weights_bf16(w, s, N, K)
            if decode:
                hip.gemv(x, wb, rows, N, K, epi, ep, ws=ws)
            else:
                hip.gemm(x, wb, rows, N, K, epi, ep, ws=ws, sk_ws=self.sk_ws)

        for li, lw in enumerate(self.layers):
            kc, vc = self.k_cache[li], self.v_cache[li]
            pe = self.pos_emb if (li == 0 and self.start == 0) else None
            hip.layernorm(hbuf, xn, lw.ln_in, lw.ln_in_b, rows, eps, pos_emb=pe, pos=pos)
            ep_qkv = hip.make_epi(out=q, k_cache=kc, v_cache=vc, slot=slot, pos=pos, ldo=q.stride(0), n_heads=nh,
                                  n_kv=nkv, head_dim=hd, t_max=self.max_seq, bias=lw.qkv_b)
            proj(xn, lw.qkv, lw.qkv_s, cfg.qkv_size, H, hip.EPI_QKV, ep_qkv)
            if tiles is not None:
                hip.attn_prefill(q, kc, vc, tiles[1], nh, nkv, hd, attn_o, causal=kv_len is None, tiles_host=tiles[0])
            else:
                hip.attn(q, kc, vc, slot, pos, rows, nh, nkv, hd, nsplit, self.part_o, self.part_lse, attn_o,
                         kv_len=kv_len, counters=self.attn_cnt, min_chunk=self.ATTN_MIN_CHUNK)
            proj(attn_o, lw.o, lw.o_s, H, cfg.q_size, hip.EPI_RESID,
                 hip.make_epi(out=hbuf, resid=hbuf, ldo=hbuf.stride(0), ldr=hbuf.stride(0), bias=lw.o_b))
            hip.layernorm(hbuf, xn, lw.ln_post, lw.ln_post_b, rows, eps)
            proj(xn, lw.gate_up, lw.gate_up_s, I, H, hip.EPI_STORE,
                 hip.make_epi(out=act, ldo=act.stride(0), bias=lw.gate_up_b, act=hip.ACT_GELU))
            proj(act, lw.down, lw.down_s, H, I, hip.EPI_RESID,
                 hip.make_epi(out=hbuf, resid=hbuf, ldo=hbuf.stride(0), ldr=hbuf.stride(0), bias=lw.down_b))
        return hbuf


def make_stage_engine(cfg, start: int, end: int, device="cpu", dtype=torch.bfloat16, *, weight_dtype: str = "bf16",
                      kv_dtype: str = "bf16", kv_layout: str = "static", kv_pages=None, **kw) -> StageEngine:
    """``StageEngine`` for ``weight_dtype`` "bf16" / "fp8" (anything else raises there),
    ``Int4StageEngine`` for "int4"; ``kv_dtype="fp8"`` on a GPU: ``Fp8KVStageEngine``
    (runtime/engine_kv8.py; bf16 or fp8 weights); ``kv_layout="paged"`` on a GPU:
    ``PagedKVStageEngine`` with a pool of ``kv_pages`` pages (runtime/engine_paged.py; bf16 or fp8
    weights, bf16 KV); the default dtypes and layout on a GPU: ``SkpStageEngine``
    (runtime/engine_skp.py, StageEngine plus the gemm_skp route). A CPU engine ignores ``kv_dtype``
    and ``kv_layout`` as it ignores ``weight_dtype``; a bad value or combination raises on every device."""
    from .engine_kv8 import Fp8KVStageEngine, check_kv_dtype
    from .engine_paged import PagedKVStageEngine, check_kv_layout
    check_kv_dtype(kv_dtype, weight_dtype)
    check_kv_layout(kv_layout, kv_pages, weight_dtype, kv_dtype)
    if kv_layout == "paged":
        from ..ops import kv_paged
        kv_paged.check_max_seq(int(min(kw.get("max_seq", 2048), cfg.max_position_embeddings)))
        if torch.device(device).type == "cuda":
            return PagedKVStageEngine(cfg, start, end, device, dtype, weight_dtype=weight_dtype, kv_pages=kv_pages, **kw)
    if kv_dtype == "fp8" and torch.device(device).type == "cuda":
        return Fp8KVStageEngine(cfg, start, end, device, dtype, weight_dtype=weight_dtype, **kw)
    if weight_dtype == "int4":
        return Int4StageEngine(cfg, start, end, device, dtype, **kw)
    if torch.device(device).type == "cuda":
        # the default dtypes on a GPU: StageEngine plus the gemm_skp route of the residual
        # projections at 385..512 decode rows (runtime/engine_skp.py; LSA_GEMM_SKP=0 turns it off)
        from .engine_skp import SkpStageEngine
        return SkpStageEngine(cfg, start, end, device, dtype, weight_dtype=weight_dtype, **kw)
    return StageEngine(cfg, start, end, device, dtype, weight_dtype=weight_dtype, **kw)
