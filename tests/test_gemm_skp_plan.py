"""The planner of ops/gemm_skp.py on the CPU: table parsing, nearest-M lookup inside one band of
128-row tiles, the refusals of check_plan, workspace sizing, the run-time switch, and that the
row counts of the full-depth fixture never reach the gemm_skp loop of runtime/engine_skp.py."""
import pytest

from llm_sharding_amd.ops import gemm_skp as S

TABLE = """
# comment line
512 4096 4096 128 128 2 0
512 4096 11008 256 256 8 1   # trailing comment
256 4096 11008 256 128 4 0
"""


def test_parse_and_lookup():
    t = S.parse_table(TABLE)
    assert t[(4096, 4096)] == [(512, (128, 128, 2, 0))]
    assert S.lookup(t, 512, 4096, 11008) == (256, 256, 8, 1)
    assert S.lookup(t, 385, 4096, 11008) == (256, 256, 8, 1)   # same four 128-row tiles
    assert S.lookup(t, 384, 4096, 11008) is None               # three tiles: not measured
    assert S.lookup(t, 200, 4096, 11008) == (256, 128, 4, 0)
    assert S.lookup(t, 512, 4096, 8192) is None
    assert S.lookup({}, 512, 4096, 4096) is None


@pytest.mark.parametrize("line", ["512 4096 4096 128 128 2", "512 4096 4096 192 128 2 0", "512 4096 4096 128 128 9 0",
                                  "512 4096 4096 128 128 2 2", "512 4096 128 128 128 3 0", "1024 4096 4096 128 128 8 0"])
def test_parse_refuses(line):
    with pytest.raises(ValueError):
        S.parse_table(line)


def test_check_plan_and_sizes():
    assert S.check_plan(512, 4096, 4096, 128, 128, 2) is None
    assert S.check_plan(512, 4096, 11008, 256, 256, 8) is None
    assert "K-tiles" in S.check_plan(129, 128, 128, 128, 128, 3)        # 2 K-tiles, 3 contributors
    assert S.check_plan(512, 4096, 4096, 128, 128, 8) is None           # 128 tiles x 8 = 1024 workgroups
    assert "workgroups" in S.check_plan(1024, 4096, 4096, 128, 128, 8)  # 256 tiles x 8
    assert S.check_plan(512, 4096, 4096, 128, 128, 1) is not None
    assert S.check_plan(512, 4000, 4096, 128, 128, 2) is not None       # N % bn
    assert S.check_plan(512, 4096, 4100, 128, 128, 2) is not None       # K % 64
    assert S.tiles(512, 4096, 256, 128) == 64 and S.tiles(129, 256, 128, 128) == 4
    assert S.slab_floats(512, 4096, 256, 128, 4) == 2 * 256 * 256 * 128
    assert S.n_counters(512, 4096, 256, 128) == 64 * 8


def test_switch(monkeypatch):
    monkeypatch.setenv("LSA_GEMM_SKP", "0")
    assert not S.enabled() and S.plan(512, 4096, 4096) is None
    monkeypatch.setenv("LSA_GEMM_SKP", "1")
    assert S.enabled()
    monkeypatch.delenv("LSA_GEMM_SKP")
    assert S.enabled()


def test_shipped_table_parses_and_knob_is_registered():
    from llm_sharding_amd.utils.runtime_config import KNOBS
    assert "LSA_GEMM_SKP" in KNOBS and "LSA_GEMM_SKP_TUNING" in KNOBS
    with open(S.TUNING_FILE) as f:
        t = S.parse_table(f.read())
    for (N, K), rows in t.items():
        for M, (bm, bn, C, tm) in rows:
            assert S.check_plan(M, N, K, bm, bn, C) is None
            assert S.tiles(M, N, bm, bn) * C <= 256   # one workgroup per CU, one round


def test_cpu_engine_is_the_base_class_and_fixture_rows_stay_outside():
    import torch

    from llm_sharding_amd.config import get_preset
    from llm_sharding_amd.runtime.engine import StageEngine
    from llm_sharding_amd.runtime.engine_int4 import make_stage_engine
    from llm_sharding_amd.runtime.engine_skp import SKP_MAX_ROWS, SKP_MIN_ROWS, SkpStageEngine
    cfg = get_preset("tiny")
    assert type(make_stage_engine(cfg, 0, 1, "cpu", torch.float32, load=False)) is StageEngine
    assert issubclass(SkpStageEngine, StageEngine)
    for rows in (4, 160, 64, 800):  # the full-depth tripwire's decode and prefill row counts
        assert not (SKP_MIN_ROWS <= rows <= SKP_MAX_ROWS)
    e = SkpStageEngine(cfg, 0, 1, "cpu", torch.float32, load=False)
    assert e.skp_plans(512) is None and e.skp_plans(4) is None  # no GPU: StageEngine's forward
