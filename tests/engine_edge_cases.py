"""Which kernels a forward of R rows runs, and the row counts at which that changes.

A forward picks its kernels from its row count: ops/routes.py, hip.gemm_sk_plan,
hip.gemm_sk_partial_plan, gemm_skp.plan and packing.proj_config do the picking.
``route_signature`` restates, on the CPU and without weights, what the engines' forward bodies
(runtime/engine.py and its variants) ask of those functions for one row count; ``edge_rows`` walks
the row counts and keeps both sides of every change. tests/test_engine_edge_cases.py pins the lists
of two model shapes; tests/test_engine_edges_gpu.py runs whole forwards at every row count of them.
The lists are derived, not written down: after a re-tune of the tables they move by themselves.
"""
import functools
from types import SimpleNamespace

from llm_sharding_amd.config import LlamaConfig, get_preset
from llm_sharding_amd.ops import gemm_skp, hip, int4, packing, routes
from llm_sharding_amd.runtime.engine import StageEngine
from llm_sharding_amd.runtime.engine_skp import SKP_MAX_ROWS, SKP_MIN_ROWS

KINDS = ("bf16", "fp8", "int4", "paged")
PROJ = ("qkv", "o", "gate_up", "down")
EPIS = (hip.EPI_QKV, hip.EPI_RESID, hip.EPI_SWIGLU, hip.EPI_RESID)
MAX_SEQ = 64            # the engines of tests/test_engine_edges_gpu.py
MAX_PREFILL_ROWS = 1024


def cfg_7b() -> LlamaConfig:
    """``_mid_cfg`` of tests/test_engine_gpu.py: Llama-2-7B layer shapes, 2 layers, vocab 4096."""
    return LlamaConfig(num_hidden_layers=2, vocab_size=4096, max_position_embeddings=1024, name="7b-2L")


def cfg_13b() -> LlamaConfig:
    """Llama-2-13B layer shapes cut as test_other_families_two_layers_vs_golden cuts its presets."""
    cfg = get_preset("llama2-13b")
    cfg.num_hidden_layers = 2
    cfg.vocab_size = 4096
    cfg.max_position_embeddings = 512
    return cfg


SHAPE_SETS = {"7b": cfg_7b, "13b": cfg_13b}


def gemv_max_rows(cfg) -> int:
    """StageEngine.GEMV_MAX_ROWS of an instance: the class value bounded by the route table."""
    return min(packing.GEMV_MAX_ROWS, routes.gemv_max_rows(StageEngine.proj_shapes(cfg)))


def native_limit(cfg, kind: str) -> int:
    """Rows up to which ``kind``'s own weight-streaming kernels run: the instance's GEMV_MAX_ROWS
    for bf16 weights, packing.GEMV_MAX_ROWS for fp8 weights (runtime/engine.py ``native_fp8``),
    INT4_MAX_ROWS for int4 (runtime/engine_int4.py ``native_int4``)."""
    return _native_limit(kind, gemv_max_rows(cfg))


def _native_limit(kind: str, gmax: int) -> int:
    return {"fp8": packing.GEMV_MAX_ROWS, "int4": int4.INT4_MAX_ROWS}.get(kind, gmax)


def decode_nsplit(cfg, rows: int, max_seq: int = MAX_SEQ) -> int:
    """StageEngine.decode_nsplit(rows) of an engine with ``max_seq`` (its own code, on a stand-in)."""
    top = int(min(16, max(1, -(-max_seq // StageEngine.ATTN_MIN_CHUNK))))
    return StageEngine.decode_nsplit(SimpleNamespace(cfg=cfg, max_decode_nsplit=top), rows)


def _gemm_family(gmax: int, rows: int, kind: str) -> bool:
    # fp8 weights keep their own kernels up to packing.GEMV_MAX_ROWS rows whatever the route table says
    return rows > packing.GEMV_MAX_ROWS or (rows > gmax and kind != "fp8")


def uses_gemm_family(cfg, rows: int, kind: str = "bf16") -> bool:
    """``proj_gemm`` of the forward bodies: the MFMA GEMMs, not the weight-streaming kernels."""
    return _gemm_family(gemv_max_rows(cfg), rows, kind)


@functools.lru_cache(maxsize=None)
def _signature(shapes: tuple, nkv: int, gmax: int, rows: int, kind: str, max_seq: int) -> tuple:
    cfg = SimpleNamespace(num_key_value_heads=nkv)
    gemm = _gemm_family(gmax, rows, kind)
    out = []
    for name, (N, K), epi in zip(PROJ, shapes, EPIS):
        even = epi == hip.EPI_SWIGLU
        if not gemm:
            if kind == "fp8":
                sig = packing.fp8_proj_config(N // 16, rows, need_even=even, k=K)
            elif kind == "int4" and rows <= int4.INT4_MAX_ROWS:
                sig = ("int4", int4.int4_config(N // 16, rows, need_even=even, k=K))
            else:
                sig = packing.proj_config(N // 16, rows, need_even=even, k=K)
                # dec_resid: the coop EPI_PARTIAL route of the bf16-weight residual projections
                if epi == hip.EPI_RESID and kind != "int4" and N in (2048, 4096, 6144, 8192):
                    pc = packing.partial_config(N // 16, rows, k=K)
                    if pc is not None:
                        sig = ("coop_partial", pc)
            out.append((name, sig[0], tuple(sig[1])))
            continue
        wr = hip.gemm_wr_plan(rows, N, K, epi, hip.EpiArgs()) if N % 128 == 0 and K % 64 == 0 else None
        if wr:
            out.append((name, "gemm_wr", wr))
        else:
            bn, _grid, dp, split, bm = hip.gemm_sk_plan(rows, N, K)
            out.append((name, "gemm_sk", (bn, dp, split, bm)))
    resid = [s for s, e in zip(shapes, EPIS) if e == hip.EPI_RESID]
    partial = tuple(hip.gemm_sk_partial_plan(rows, N, K) if gemm and rows <= hip.PARTIAL_MAX_ROWS else None
                    for N, K in resid)
    skp = (None, None)
    if kind == "bf16" and gemm and SKP_MIN_ROWS <= rows <= SKP_MAX_ROWS and not any(partial):
        skp = tuple(gemm_skp.plan(rows, N, K) for N, K in resid)
    limits = (rows <= gmax, rows <= _native_limit(kind, gmax))
    return (tuple(out), partial, skp, decode_nsplit(cfg, rows, max_seq), limits)


def route_signature(cfg, rows: int, kind: str = "bf16", max_seq: int = MAX_SEQ) -> tuple:
    """(projections, partial plans, skp plans, decode_nsplit, native limits) of a ``rows``-row
    forward of a ``kind`` engine (bf16 / fp8 / int4 weights, or bf16 weights on a paged KV cache):

    * projections: for qkv, o, gate_up, down a (name, family, plan) tuple - ``gemv`` / ``coop`` /
      ``coop_partial`` / ``fp8`` / ``coop_fp8`` / ``int4`` with the launch config, ``gemm_wr`` with
      bn, ``gemm_sk`` with (bn, dp, split, bm);
    * the gemm_sk K-split partial plan of o and down (None: the fused residual epilogue);
    * the gemm_skp plan of o and down (bf16 weights on the static cache, 385..512 rows);
    * the engine's ``decode_nsplit(rows)`` at ``max_seq``;
    * whether ``rows`` is within the instance's GEMV_MAX_ROWS and within the kind's native limit.
    """
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {KINDS}, got {kind!r}")
    return _signature(tuple(StageEngine.proj_shapes(cfg)), cfg.num_key_value_heads, gemv_max_rows(cfg), rows, kind,
                      max_seq)


def edge_rows(cfg, kind: str = "bf16", max_rows: int = 512) -> list:
    """1, ``max_rows`` and both sides of every change of :func:`route_signature` in between."""
    rows = {1, max_rows}
    prev = route_signature(cfg, 1, kind)
    for m in range(2, max_rows + 1):
        sig = route_signature(cfg, m, kind)
        if sig != prev:
            rows.update((m - 1, m))
        prev = sig
    return sorted(rows)


def unfuse_layer(cfg, qkv, o, gate_up, down) -> dict:
    """The reference state dict of a layer from the engine's fused [N, K] matrices (the inverse of
    packing.fuse_qkv / fuse_gate_up), with unit norm weights: the matrices hold the RMSNorm weights
    already (packing.fold_norm), so a golden model on this dict computes with the engine's
    effective weights."""
    import torch
    qs, kvs, I, H = cfg.q_size, cfg.kv_size, cfg.intermediate_size, cfg.hidden_size
    pq = packing.rope_rows_perm(cfg.num_attention_heads, cfg.head_dim).to(qkv.device)
    pk = packing.rope_rows_perm(cfg.num_key_value_heads, cfg.head_dim).to(qkv.device)
    wq, wk = torch.empty_like(qkv[:qs]), torch.empty_like(qkv[qs:qs + kvs])
    wq[pq] = qkv[:qs]
    wk[pk] = qkv[qs:qs + kvs]
    gu = gate_up.view(I // 16, 2, 16, H)
    ones = torch.ones(H, dtype=qkv.dtype, device=qkv.device)
    return {"self_attn.q_proj.weight": wq, "self_attn.k_proj.weight": wk, "self_attn.v_proj.weight": qkv[qs + kvs:],
            "self_attn.o_proj.weight": o, "mlp.gate_proj.weight": gu[:, 0].reshape(I, H),
            "mlp.up_proj.weight": gu[:, 1].reshape(I, H), "mlp.down_proj.weight": down,
            "input_layernorm.weight": ones, "post_attention_layernorm.weight": ones}


def describe(cfg, rows: int, kind: str = "bf16") -> str:
    proj, partial, skp, nsplit, limits = route_signature(cfg, rows, kind)
    return f"{rows} rows [{kind}]: " + "; ".join(f"{n} {f} {p}" for n, f, p in proj) + \
        f"; partial {partial}; skp {skp}; nsplit {nsplit}"
