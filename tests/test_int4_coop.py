"""CPU side of the cooperative int4 GEMV (ops/int4.py): its config list and rule over the model
shapes, the reach of the GPU sweep (tests/test_int4_coop_gpu.py), and the exact-case builders at
the row counts only this kernel serves."""
import pytest
import torch

import int4_cases as I4
import test_int4_coop_gpu as G
from llm_sharding_amd.config import get_preset
from llm_sharding_amd.ops import int4, packing
from llm_sharding_amd.runtime.engine import StageEngine

MODELS = ("llama2-7b", "llama2-13b", "llama3.2-3b", "llama2-70b", "gpt2", "gpt2-medium", "gpt2-large")


def test_config_list():
    assert len(set(int4.INT4_COOP_CONFIGS)) == len(int4.INT4_COOP_CONFIGS)
    assert {b for b, _, _, _ in int4.INT4_COOP_CONFIGS} == {2, 4, 8}
    assert {t * w for _, t, w, _ in int4.INT4_COOP_CONFIGS} == {4, 8}
    assert int4.INT4_COOP_MAX_ROWS == 128 and int4.INT4_MAX_ROWS == 64
    assert int4.int4_coop_candidates(48, 384, 16) == [] and int4.int4_coop_candidates(48, 384, 129) == []
    assert int4.int4_coop_config(3, 384, 65) is None
    for c in int4.int4_coop_candidates(48, 384, 65):            # every split keeps a group
        assert c[3] <= 3


@pytest.mark.parametrize("model", MODELS)
def test_every_model_projection_has_a_config(model):
    cfg = get_preset(model)
    shapes = StageEngine.proj_shapes(cfg)
    for i, (n, k) in enumerate(shapes):
        even = i == 2 and not cfg.is_gpt2
        for rows in (17, 64, 65, 128):
            c = int4.int4_coop_config(n // 16, k, rows, even)
            assert c is not None, (model, n, k, rows)
            tnw, nw, d, sk = c
            assert (packing.row_blocks(rows), tnw, nw, d) in int4.INT4_COOP_CONFIGS and sk <= k // 128
            assert int4.int4_coop_slab_floats(n, rows, tnw, nw, sk) <= int4.INT4_COOP_SLAB_FLOATS
            assert n // 16 // (tnw * nw) <= 4096                # the engine workspace's counters
    if model == "llama2-7b":                                    # the measured winners (profiles/int4.md) at 128 rows
        got = [int4.int4_coop_config(n // 16, k, 128, i == 2) for i, (n, k) in enumerate(shapes)]
        assert got == [(1, 8, 3, 2), (1, 4, 3, 4), (1, 8, 3, 1), (1, 8, 3, 8)]
        assert all((n, k, mb) in int4.INT4_COOP_ROUTE for n, k in shapes for mb in (2, 4))


def test_gpu_sweep_reaches_every_config():
    for mb, tnw, nw, d in int4.INT4_COOP_CONFIGS:
        got = {(M, K, sk) for M in G.ROWS if packing.row_blocks(M) == mb for K in G.KS
               for sk in G.splits(tnw, nw, d, G.n_for(tnw, nw) // 16, K, M, True)}
        assert {sk for _, _, sk in got} == {1, 2, 4, 8} and {K for _, K, _ in got} == set(G.KS)
    nh, nkv, hd = G.QKV_GEOM_16                                 # the QKV cases: 12 tiles or 16 for every workgroup width
    assert all(G.QKV_TILES % (t * w) == 0 or (nh + 2 * nkv) * hd // 16 % (t * w) == 0 for _, t, w, _ in int4.INT4_COOP_CONFIGS)
    assert int4.int4_coop_config(1024, 4096, 128, counters=64) is None   # too few arrival counters: declined


@pytest.mark.parametrize("M", [65, 128])
def test_exact_builders_at_coop_rows(M, monkeypatch):
    """tests/int4_cases.py asserts its exactness conditions while it builds; the linear reference
    also equals the group-by-group fp32 accumulation of the kernels."""
    for K in G.KS:
        c = I4.case("linear", M, 128, K)
        acc = torch.zeros(M, 128)
        for g in range(K // 128):
            sl = slice(128 * g, 128 * (g + 1))
            acc = acc + c.W.scale[:, g][None, :] * (c.a[:, sl].float() @ c.W.q[:, sl].float().T)
        assert torch.equal(acc.double(), c.y)
        if K >= I4.K_ROUND_MIN:
            I4.case("round_once", M, 128, K)
        I4.case("swiglu", M, 64, K)
        I4.case("gelu", M, 128, K)
        I4.case("norm", M, 128, K)
        for rope in (True, False):
            assert I4.case("qkv", M, K, rope).N == 16 * G.QKV_TILES
            assert G.qkv_case(8, M, K, rope, monkeypatch, "cpu").N == 256
