"""CPU side of the int4 GEMM (csrc/quant/gemm_int4.hip): the config rule of ops/int4.py."""
from llm_sharding_amd.ops import int4

LLAMA7B = ((12288, 4096), (4096, 4096), (22016, 4096), (4096, 11008))


def test_gemm_config_rule(monkeypatch):
    monkeypatch.setenv("LSA_INT4_GEMM", "1")
    assert len(set(int4.INT4_GEMM_CONFIGS)) == len(int4.INT4_GEMM_CONFIGS)
    for M in (1, 129, 256, 512, 1024, 2048):
        for n, k in LLAMA7B:
            bn, sk = int4.int4_gemm_config(M, n, k)
            assert (bn, sk) in int4.int4_gemm_candidates(M, n, k) and n % bn == 0 and sk <= k // 128
            tiles = -(-M // 128) * (n // bn)
            assert sk == 1 or (k // 128 // sk >= int4.INT4_GEMM_MIN_CHUNKS and tiles < int4.INT4_GEMM_MIN_GRID)
            assert int4.int4_gemm_slab_floats(M, n, sk) <= int4.INT4_COOP_SLAB_FLOATS
    assert int4.int4_gemm_config(512, 4096, 4096)[1] > 1              # 128 tiles: the o projection is split
    assert int4.int4_gemm_config(512, 12288, 4096) == (128, 1)        # 384 tiles fill the CUs unsplit
    # the workspace bounds the split: a slab for 2 splits only, then none; counters per output tile
    need2 = int4.int4_gemm_slab_floats(129, 4096, 2)
    assert need2 == 2 * 256 * 4096 and int4.int4_gemm_slab_floats(129, 4096, 1) == 0
    assert int4.int4_gemm_config(129, 4096, 4096, slab_floats=need2) == (128, 2)
    assert int4.int4_gemm_config(129, 4096, 4096, slab_floats=need2 - 1) == (128, 1)
    assert int4.int4_gemm_config(129, 4096, 4096, counters=63) == (128, 1)
    assert int4.int4_gemm_config(129, 192, 384) is None               # no built tile divides 192 columns
    assert int4.int4_gemm_config(129, 256, 320) is None               # K % 128
    # the dispatcher's bound: shapes of up to INT4_GEMM_MAX_TILES output tiles
    assert int4.int4_gemm_serves(((4096, 4096), (4096, 11008)), 256) and not int4.int4_gemm_serves(LLAMA7B, 256)
    assert not int4.int4_gemm_serves(((4096, 4096),), 257) and not int4.int4_gemm_serves(((192, 384),), 129)
    monkeypatch.delenv("LSA_INT4_GEMM")                                # opt-in: off by default
    assert not int4.int4_gemm_serves(((4096, 4096),), 256)
