"""The derived route-edge row counts (tests/engine_edge_cases.py) of the two model shapes that
tests/test_engine_edges_gpu.py runs, computed on the CPU from the route and tuning tables."""
import pytest

import engine_edge_cases as E
from llm_sharding_amd.ops import hip

# the route changes a CPU sweep of Llama-2-7B layer shapes over 1..512 rows finds: gemv -> coop
# (17), the coop row block (33), the coop configs and the fp8 / int4 native limit (65), GEMV ->
# GEMM family (129), qkv and gate_up -> gemm_wr (193), back to gemm_sk (257), qkv -> gemm_wr bn
# 192 (320), o and down -> gemm_skp (385)
EDGES_7B = {1, 16, 17, 32, 33, 64, 65, 128, 129, 192, 193, 256, 257, 319, 320, 384, 385, 512}
# ... and one the route table alone does not show: hip.gemm_wr_plan takes a shape only when its
# last 128-row tile is at least half full, so 385..447 rows keep qkv on gemm_sk and 448 returns it
# to gemm_wr (tests/test_gemm_sk_plan.py pins 447 -> None, 448 -> 192)
HALF_FULL_TILE_7B = {447, 448}


@pytest.fixture(autouse=True)
def _default_routes(monkeypatch):
    for name in ("LSA_GEMV_MAX_ROWS", "LSA_GEMM_WR", "LSA_GEMM_SKP"):
        monkeypatch.delenv(name, raising=False)


def test_7b_bf16_edges():
    cfg = E.cfg_7b()
    rows = E.edge_rows(cfg, "bf16")
    assert set(rows) == EDGES_7B | HALF_FULL_TILE_7B and rows == sorted(rows)
    # the half-full rule and nothing else makes the extra pair: the qkv family is what differs
    a, b = E.route_signature(cfg, 447), E.route_signature(cfg, 448)
    assert a[0][0] != b[0][0] and a[0][1:] == b[0][1:] and a[1:] == b[1:]
    assert a[0][0][1] == "gemm_sk" and b[0][0][1:] == ("gemm_wr", 192)
    # what the table of edges says of each
    fam = {m: [p[1] for p in E.route_signature(cfg, m)[0]] for m in rows}
    assert set(fam[16]) == {"gemv"} and "gemv" not in fam[17] and set(fam[17]) <= {"coop", "coop_partial"}
    assert E.route_signature(cfg, 32)[0] != E.route_signature(cfg, 33)[0]
    assert not E.uses_gemm_family(cfg, 128) and E.uses_gemm_family(cfg, 129)
    assert fam[192][0] == fam[192][2] == "gemm_sk" and fam[193][0] == fam[193][2] == "gemm_wr"
    assert set(fam[257]) == {"gemm_sk"}
    assert E.route_signature(cfg, 319)[0][0][1] == "gemm_sk" and E.route_signature(cfg, 320)[0][0][1:] == ("gemm_wr", 192)
    assert E.route_signature(cfg, 384)[2] == (None, None) and all(E.route_signature(cfg, 385)[2])


def test_13b_edges():
    """Llama-2-13B shapes: the 65..128-row decode goes to gemm_sk (ops/routes.py), and the route
    table itself moves qkv to gemm_wr bn 256 at 448 rows."""
    cfg = E.cfg_13b()
    rows = E.edge_rows(cfg, "bf16")
    assert {64, 65, 447, 448} <= set(rows)
    assert E.gemv_max_rows(cfg) == 64 and not E.uses_gemm_family(cfg, 64) and E.uses_gemm_family(cfg, 65)
    assert {p[1] for p in E.route_signature(cfg, 65)[0]} == {"gemm_sk"}
    assert E.route_signature(cfg, 448)[0][0][1:] == ("gemm_wr", 256)


@pytest.mark.parametrize("shape", sorted(E.SHAPE_SETS))
@pytest.mark.parametrize("kind", E.KINDS)
def test_lists_are_short_and_complete(shape, kind):
    cfg = E.SHAPE_SETS[shape]()
    rows = E.edge_rows(cfg, kind)
    assert len(rows) <= 32 and rows[0] == 1 and rows[-1] == 512
    # both sides of every change, and no change between two listed neighbours
    for lo, hi in zip(rows, rows[1:]):
        inner = [m for m in range(lo, hi) if hi > lo + 1
                 and E.route_signature(cfg, m, kind) != E.route_signature(cfg, m + 1, kind)]
        assert not inner, (lo, hi, inner)
    lim = E.native_limit(cfg, kind)
    assert lim in rows and lim + 1 in rows


def test_signature_names_the_native_limits():
    cfg = E.cfg_7b()
    assert E.native_limit(cfg, "bf16") == 128 and E.native_limit(cfg, "fp8") == 128 and E.native_limit(cfg, "int4") == 64
    assert E.route_signature(cfg, 64, "int4")[0][0][1] == "int4" and E.route_signature(cfg, 65, "int4")[0][0][1] == "coop"
    assert E.route_signature(cfg, 128, "fp8")[0][0][1] in ("fp8", "coop_fp8")
    assert E.route_signature(cfg, 129, "fp8")[0] == E.route_signature(cfg, 129, "bf16")[0]
    # int4 weights skip the coop EPI_PARTIAL route of the residual projections (runtime/engine_int4.py)
    assert "coop_partial" not in {p[1] for m in range(65, 129) for p in E.route_signature(cfg, m, "int4")[0]}
    assert E.route_signature(cfg, 512, "paged")[2] == (None, None) and E.route_signature(cfg, 512, "fp8")[2] == (None, None)
    assert E.decode_nsplit(cfg, 1) == 1 and E.decode_nsplit(cfg, 1, max_seq=2048) == 8
    with pytest.raises(ValueError):
        E.route_signature(cfg, 1, "fp16")


def test_unfuse_layer_inverts_the_engine_fusion():
    """A golden model on unfuse_layer(fused, norm-folded matrices) is the golden model of the layer."""
    import torch
    from llm_sharding_amd.config import tiny
    from llm_sharding_amd.models import weights as W
    from llm_sharding_amd.models.reference import ReferenceLlama
    from llm_sharding_amd.ops import packing
    cfg = tiny(layers=1)
    lw = {k: v.float() for k, v in W.random_layer(cfg, 0, torch.bfloat16, "cpu", 3).items()}
    qkv = packing.fuse_qkv(lw["self_attn.q_proj.weight"], lw["self_attn.k_proj.weight"], lw["self_attn.v_proj.weight"],
                           cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim)
    gu = packing.fuse_gate_up(lw["mlp.gate_proj.weight"], lw["mlp.up_proj.weight"])
    un = E.unfuse_layer(cfg, packing.fold_norm(qkv, lw["input_layernorm.weight"]), lw["self_attn.o_proj.weight"],
                        packing.fold_norm(gu, lw["post_attention_layernorm.weight"]), lw["mlp.down_proj.weight"])
    assert set(un) == set(lw)
    args = (W.random_embedding(cfg, torch.float32), )
    tail = (W.random_final_norm(cfg, torch.float32), W.random_lm_head(cfg, torch.float32))
    x = torch.randn(3, 5, cfg.hidden_size, generator=torch.Generator().manual_seed(1))
    a = ReferenceLlama(cfg, *args, [lw], *tail, max_pos=16).forward_hidden(x)
    b = ReferenceLlama(cfg, *args, [un], *tail, max_pos=16).forward_hidden(x)
    # fp32 on both sides, another order of the same products: a wrong permutation is off by O(1)
    assert torch.allclose(a, b, rtol=1e-4, atol=1e-4)


def test_704_rows_consult_the_partial_planner():
    """704 rows of the 7B down projection: two tuned row counts at the same distance."""
    ms = sorted(m for m, _ in hip._sk_partial()[(4096, 11008)] if -(-m // hip.SK_BM) == 3)
    assert any(abs(a - 704) == abs(b - 704) for a in ms for b in ms if a < b)
    E.route_signature(E.cfg_7b(), 704)
