"""Mx4StageEngine: a StageEngine whose layer projections stay MXFP4 on the device.

``make_stage_engine(..., weight_dtype="mxfp4")`` (what ``inference.py --weight-dtype mxfp4`` and
``PipelineStage(weight_dtype="mxfp4")`` build) keeps the four projections of every layer as OCP
microscaling fp4: e2m1 codes with one e8m0 exponent per 32 weights along K, 4.25 bits per weight
(ops/mx4.py). Decode batches of up to 128 rows stream them through csrc/quant/gemv_mx4.hip, which
quantises the activations to MXFP8 on the way and multiplies on the block-scaled MFMA: decode is
W4A8. Larger decode batches and prefill chunks dequantise one projection at a time into
``w_scratch`` (exactly: every ``code * 2^e`` is a bf16 value) and run the bf16 kernels on the
routes fp8 weights take: they are W4A16 on the same weights. With ``LSA_MX4_GEMM=1`` (read at
construction for the scratch, at every call for the route) those rows run csrc/quant/gemm_mx4.hip
instead: a pre-pass quantises each projection's input to MXFP8 once into ``a_mx8`` and the GEMM
multiplies on the block-scaled MFMA, so prefill becomes W4A8 too (``mx4.proj_gemm_mx4``; the
residual projections on its EPI_RESID epilogue, no ``part_k``, when all four shapes qualify).

The lm_head, the embedding and the norms stay bf16. Each fused matrix is quantised here with its
RMSNorm weight folded in. Llama-family layers only: GPT-2 raises ``NotImplementedError``. The fp8
KV cache and the paged KV layout are refused with this weight format (``check_kv_dtype``,
``check_kv_layout``). On a CPU device the option is ignored, as fp8 and int4 are.

It is a subclass for the reason engine_int4.py gives: runtime/engine.py is a recorded input of the
bf16 decode path's full-depth fixture and stays as it is.
"""
from __future__ import annotations

from typing import Optional

import torch

from ..ops import mx4, packing
from .engine import StageEngine

PROJ = ("qkv", "o", "gate_up", "down")


class Mx4StageEngine(StageEngine):
    def __init__(self, cfg, start: int, end: int, device="cpu", dtype=torch.bfloat16, *, weight_dtype: str = "mxfp4",
                 **kw):
        if weight_dtype != "mxfp4":
            raise ValueError(f"Mx4StageEngine holds mxfp4 weights, got weight_dtype={weight_dtype!r}")
        self.mx4 = torch.device(device).type == "cuda"  # before the base constructor loads the weights
        if self.mx4:
            if cfg.is_gpt2:
                raise NotImplementedError("weight_dtype='mxfp4' serves Llama-family layers only")
            for name, (n, k) in zip(PROJ, self.proj_shapes(cfg)):
                if k % mx4.MX_STEP:
                    raise ValueError(f"weight_dtype='mxfp4' needs K % {mx4.MX_STEP} == 0: the {name} projection "
                                     f"has K={k}")
        super().__init__(cfg, start, end, device, dtype, weight_dtype="bf16", **kw)

    # ------------------------------------------------------------------------- loading
    def _prepare_layer(self, lw: dict):
        """The base engine's fused, norm-folded, packed bf16 matrices, re-quantised: packed fp4
        codes [N*K/2] in the LayerWeights slots, packed e8m0 exponents beside them."""
        out = super()._prepare_layer(lw)
        if not self.mx4:
            return out
        for name in PROJ:
            q, e = mx4.quantize_mx4(packing.unpack_b(getattr(out, name)))
            setattr(out, name, mx4.pack_b_mx4(q))
            setattr(out, name + "_s", mx4.pack_scales_mx4(e))
        return out

    def _alloc_runtime(self) -> None:
        # the MXFP8 image of one projection's input (codes + exponents, ops/mx4.py) for the native
        # GEMM: allocated only when LSA_MX4_GEMM is on at construction
        self.a_mx8 = None
        R = max(self.max_prefill_rows, self.DECODE_MAX_ROWS)
        if self.mx4 and mx4.mx4_gemm_enabled() and R > mx4.MX4_MAX_ROWS:
            kmax = max(k for _, k in self.proj_shapes(self.cfg))
            self.a_mx8 = torch.empty(sum(mx4.a_image_bytes(R, kmax)), dtype=torch.uint8, device=self.device)
        super()._alloc_runtime()
        if self.mx4:  # one projection's bf16 weights, for the > 128-row and prefill paths
            shapes = self.proj_shapes(self.cfg)
            self.w_scratch = torch.empty(max(n * k for n, k in shapes), dtype=torch.bfloat16, device=self.device)

    def _alloc_part_k(self, R: int):
        """No split-K partial buffer where the native mxfp4 GEMM takes all four projections at every
        row count up to ``R``: the residual projections then run its EPI_RESID (+ ss_out) epilogue."""
        ws = self.coop_ws
        if self.a_mx8 is not None and all(
                mx4.mx4_gemm_serves(self.proj_shapes(self.cfg), m, ws.slab.numel(), ws.counters.numel())
                for m in range(mx4.MX4_GEMM_ROWS, R + 1, mx4.MX4_GEMM_ROWS)):
            return None
        return super()._alloc_part_k(R)

    # a forward pass also writes the activation image: one per concurrently running graph
    SCRATCH_ATTRS = StageEngine.SCRATCH_ATTRS + ("a_mx8",)

    def decode_scratch(self, k: int, rows: Optional[int] = None) -> dict:
        d = super().decode_scratch(k, rows)
        if "a_mx8" not in d:
            d["a_mx8"] = None if self.a_mx8 is None else torch.empty_like(self.a_mx8)
        return d

    def memory_bytes(self) -> int:
        return super().memory_bytes() + (0 if self.a_mx8 is None else self.a_mx8.numel())

    # ------------------------------------------------------------------------- HIP path
    # _forward_hip is StageEngine's, statement for statement, with the weight closures (wbf, dec)
    # dispatching on the mxfp4 weights: mx4.proj_mx4 up to 128 decode rows, else dequantise into
    # w_scratch and the SAME bf16 route the base engine takes for that row count, as its fp8
    # weights do. tests/test_mx4.py pins that the two bodies differ in those lines only.
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
        native_fp8 = False  # mxfp4 weights: the name stays so that the rest of the body is the base engine's
        native_mx4 = decode and rows <= mx4.MX4_MAX_ROWS
        if cfg.is_gpt2:
            raise NotImplementedError("mxfp4 weights: Llama-family layers only")
        wbf = self._weights_bf16  # packed bf16 weights (mxfp4 -> scratch for the larger-row kernels)

        def dec(x, w, s, N, K, epi, ep, norm=False):
            if native_mx4 and mx4.proj_mx4(x, w, s, rows, N, K, epi, ep, norm=norm, eps=eps, ws=ws):
                pass  # launched on the mxfp4 kernel; False: no config for the shape, dequantise
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
            if mx4.proj_gemm_mx4(x, w, s, rows, N, K, epi, ep, ws=ws, a_scratch=self.a_mx8): return  # else dequantise
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
        """A projection's packed bf16 weights: ``w`` itself, or the mxfp4 tensor dequantised
        into ``w_scratch`` (one projection at a time, consumed by the next launch on the stream)."""
        return w if s is None else mx4.dequant_mx4_packed(w, s, self.w_scratch, N, K)
