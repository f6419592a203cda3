"""SkpStageEngine: a StageEngine whose 385-512-row bf16 decode steps may run the two residual
projections (o and down) through ``lsa_gemm_skp`` (csrc/gemm_skp/gemm_skp.hip, ops/gemm_skp.py):
gemm_sk's split-K GEMM with the fix-up shared by all contributors of a tile.

``make_stage_engine`` builds it for the default dtypes (bf16 or fp8-stored weights, bf16 KV) on
a GPU. It overrides the HIP forward only for

* Llama-family layers with bf16 weights, no tile table (a decode step), 385..512 rows (the
  four-row-tile band of the 128-row tiles), the GEMM projection path with the fused RMSNorm, and
* a measured gemm_skp plan for at least one of the two projections (ops/skp_tuning.txt; none
  with ``LSA_GEMM_SKP=0``),

and there re-states the GEMM path's layer loop: the fused-norm ``ss`` flow, qkv and gate_up via
``hip.gemm``, o and down via gemm_skp where the table has a winner and via ``hip.gemm`` where not.
Every other forward is StageEngine's. A projection on a gemm_skp plan whose tile and split are
gemm_sk's own computes gemm_sk's bits; another tile or split changes the K ranges summed.

It is a subclass for the reason engine_int4.py gives: runtime/engine.py is a recorded input of the
bf16 decode path's full-depth fixture (tests/fixture_hash.py) and stays as it is. The fixture's
row counts (4 and 160 decode, 64 and 800 prefill) are outside the band.
"""
from __future__ import annotations

from typing import Optional

import torch

from ..ops import gemm_skp
from .engine import StageEngine

SKP_MIN_ROWS, SKP_MAX_ROWS = 385, 512


class SkpStageEngine(StageEngine):

    def skp_plans(self, rows: int, tiles=None) -> Optional[tuple]:
        """(plan of o, plan of down) when this forward takes the gemm_skp loop, else None."""
        from ..ops import hip
        cfg = self.cfg
        if not (SKP_MIN_ROWS <= rows <= SKP_MAX_ROWS) or tiles is not None or cfg.is_gpt2 or self.fp8:
            return None
        if not gemm_skp.enabled() or self.device.type != "cuda" or self.sk_ws is None:
            return None
        if rows <= self.GEMV_MAX_ROWS or self.ss_buf is None or rows > self.ss_buf.shape[0]:
            return None  # not the GEMM path with the fused RMSNorm
        H, I = cfg.hidden_size, cfg.intermediate_size
        shapes = ((H, cfg.q_size), (H, I))
        if self.part_k is not None and rows <= self.part_k.shape[1] and \
                any(hip.gemm_sk_partial_plan(rows, N, K) is not None for N, K in shapes):
            return None  # K-split partials summed by the norm kernel: StageEngine's flow
        plans = tuple(gemm_skp.plan(rows, N, K) for N, K in shapes)
        for (N, K), p in zip(shapes, plans):
            if p is not None and (self.sk_ws.slab.numel() < gemm_skp.slab_floats(rows, N, p[0], p[1], p[2]) or
                                  self.sk_ws.counters.numel() < gemm_skp.n_counters(rows, N, p[0], p[1])):
                return None
        return plans if any(p is not None for p in plans) else None

    def _forward_hip(self, h, slot, pos, kv_len, rows, nsplit: Optional[int] = None, tiles=None) -> torch.Tensor:
        plans = self.skp_plans(rows, tiles)
        if plans is None:
            return super()._forward_hip(h, slot, pos, kv_len, rows, nsplit, tiles)
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
        if nsplit is None:
            kv_max = int(pos.max().item()) + 1 if kv_len is None else int(kv_len.max().item())
            nsplit = self._attn_nsplit(rows, kv_max)
        q, attn_o, act = self.buf_q[:rows], self.buf_attn[:rows], self.buf_act[:rows]
        ws, sk_ws = self.coop_ws, self.sk_ws
        ss = self.ss_buf[:rows]

        def resid_proj(x, w, N, K, ep, p):
            if p is None:
                hip.gemm(x, w, rows, N, K, hip.EPI_RESID, ep, ws=ws, sk_ws=sk_ws)
            else:
                gemm_skp.gemm_skp(x, w, rows, N, K, hip.EPI_RESID, ep, bm=p[0], bn=p[1], contributors=p[2],
                                  tile_major=p[3], ws=sk_ws)

        ss_valid = False  # ss holds the partials of hbuf's current values
        for li, lw in enumerate(self.layers):
            kc, vc = self.k_cache[li], self.v_cache[li]
            if not ss_valid:  # a stage's first layer: the partials a residual GEMM epilogue writes
                hip.row_ss(hbuf, rows, ss)
            ep_qkv = hip.make_epi(out=q, k_cache=kc, v_cache=vc, slot=slot, pos=pos, cos=self.cos, sin=self.sin,
                                  ldo=q.stride(0), n_heads=nh, n_kv=nkv, head_dim=hd, t_max=self.max_seq,
                                  ss_in=ss, ss_eps=eps)
            hip.gemm(hbuf, lw.qkv, rows, cfg.qkv_size, H, hip.EPI_QKV, ep_qkv, ws=ws, sk_ws=sk_ws)
            hip.attn(q, kc, vc, slot, pos, rows, nh, nkv, hd, nsplit, self.part_o, self.part_lse, attn_o,
                     kv_len=kv_len, counters=self.attn_cnt, min_chunk=self.ATTN_MIN_CHUNK)
            ep_r = hip.make_epi(out=hbuf, resid=hbuf, ldo=hbuf.stride(0), ldr=hbuf.stride(0), ss_out=ss)
            resid_proj(attn_o, lw.o, H, cfg.q_size, ep_r, plans[0])
            hip.gemm(hbuf, lw.gate_up, rows, 2 * I, H, hip.EPI_SWIGLU,
                     hip.make_epi(out=act, ldo=act.stride(0), ss_in=ss, ss_eps=eps), ws=ws, sk_ws=sk_ws)
            resid_proj(act, lw.down, H, I, ep_r, plans[1])
            ss_valid = True
        return hbuf
