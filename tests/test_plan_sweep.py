"""Every planner at every row count, on the CPU.

A forward picks its kernels from its row count, so each row count can reach another branch of
routes.route, hip.gemm_sk_plan, hip.gemm_sk_partial_plan, hip.gemm_wr_plan, gemm_skp.plan,
packing.proj_config / partial_config / fp8_proj_config and the int4 config functions. The sweep
calls them for M = 1..2048 on the projection shapes of every preset and on every (N, K) of the
three tuning tables, and holds every answer to the preconditions of the launcher that would
receive it - restated here from the ``_req`` lines of ops/hip.py, ops/int4.py, ops/gemm_skp.py and
from the host checks of lsa_gemm_sk (csrc/kernels/gemm_sk.hip) - with the workspaces an engine of
that shape allocates. Nothing is launched.
"""
import json

import pytest

from llm_sharding_amd.config import PRESETS, get_preset
from llm_sharding_amd.ops import gemm_skp, hip, int4, packing, routes
from llm_sharding_amd.runtime.engine import StageEngine

M_MAX = 2048
EPIS = (hip.EPI_QKV, hip.EPI_RESID, hip.EPI_SWIGLU, hip.EPI_RESID)  # of qkv, o, gate_up, down
SK_WS_SLAB = 2 * 256 * hip.SK_BM * 256  # hip.SkWorkspace(device): grid 256, bn 256
SK_WS_COUNTERS = 4 * 256


@pytest.fixture(autouse=True)
def _default_routes(monkeypatch):
    for name in ("LSA_GEMV_MAX_ROWS", "LSA_GEMM_WR", "LSA_GEMM_SKP"):
        monkeypatch.delenv(name, raising=False)


def _table_keys() -> set:
    keys = set()
    for path in (hip.SK_TUNING_FILE, packing.TUNING_FILE):
        with open(path) as fh:
            keys |= {(e["N"], e["K"]) for e in json.load(fh)["entries"]}
    with open(gemm_skp.TUNING_FILE) as fh:
        keys |= set(gemm_skp.parse_table(fh.read()))
    return keys


def _preset_shapes() -> dict:
    """preset -> [(N, K, epilogue, need_even)] of its four projections."""
    out = {}
    for name in sorted(PRESETS):
        cfg = get_preset(name)
        epis = (hip.EPI_QKV, hip.EPI_RESID, hip.EPI_STORE, hip.EPI_RESID) if cfg.is_gpt2 else EPIS
        out[name] = [(N, K, e, e == hip.EPI_SWIGLU) for (N, K), e in zip(StageEngine.proj_shapes(cfg), epis)]
    return out


def _cases() -> list:
    """(N, K, epilogues, need_even values, from a preset): a preset shape with the epilogue the
    engine gives it, a shape known only from a tuning table with every epilogue."""
    seen, out = {}, []
    for shapes in _preset_shapes().values():
        for N, K, epi, even in shapes:
            seen.setdefault((N, K), set()).add((epi, even))
    for (N, K), es in sorted(seen.items()):
        out.append((N, K, sorted({e for e, _ in es}), sorted({v for _, v in es}), True))
    for N, K in sorted(_table_keys() - set(seen)):
        out.append((N, K, [hip.EPI_STORE, hip.EPI_RESID, hip.EPI_SWIGLU, hip.EPI_QKV], [False, True], False))
    return out


# ------------------------------------------------------------------------------ launcher preconditions
def _sk_launch(M, N, K, epi, bm, bn, grid, dp, split, fused_ss=False):
    """Why hip.gemm_sk + lsa_gemm_sk would refuse this plan with the engine's SkWorkspace, or None."""
    if bn not in (128, 192, 256) or bm not in (128, 256):
        return f"tile {bm}x{bn}"
    if N % (16 if bn == 192 else bn) or (bn == 192 and epi == hip.EPI_SWIGLU and N % 32):
        return f"N={N} does not tile by bn={bn}"
    if fused_ss and bn == 192:
        return "ss_out with bn 192"
    if not 1 <= grid <= 1024:
        return f"grid {grid}"
    if SK_WS_SLAB < 2 * grid * bm * bn or SK_WS_COUNTERS < 2 * grid:
        return "workspace too small (wrapper)"
    nkt, tiles = K // 64, -(-M // bm) * -(-N // bn)
    G = min(grid, tiles * nkt)
    dp_rounds = tiles // G if dp else 0
    sk_tiles = tiles - dp_rounds * G
    if epi == hip.EPI_PARTIAL:
        if split < 1 or split > nkt or tiles * split > grid:
            return f"partial: {tiles} tiles x split {split} for grid {grid}, {nkt} K-tiles"
        return None
    if split > 0 and 0 < sk_tiles <= G:
        pass
    elif sk_tiles > 0 and sk_tiles * nkt < G:
        if dp_rounds > 0:
            sk_tiles += G
        else:
            G = sk_tiles * nkt
    if sk_tiles > 0 and (SK_WS_SLAB < 2 * G * bm * bn or SK_WS_COUNTERS < sk_tiles):
        return f"{sk_tiles} split tiles for {SK_WS_COUNTERS} tickets"
    return None


def _check_sk_plan(M, N, K, epi):
    bn, grid, dp, split, bm = hip.gemm_sk_plan(M, N, K)
    assert grid == hip.N_CU and dp in (0, 1) and split >= 0
    fused = epi == hip.EPI_RESID  # the engine's residual GEMMs write ss_out: bn 192 becomes 256 / 128
    if fused and bn == 192:
        bn = 256 if N % 256 == 0 else 128
    why = _sk_launch(M, N, K, epi, bm, bn, grid, dp, split, fused_ss=fused)
    assert why is None, why


def _check_partial_plan(M, N, K):
    pp = hip.gemm_sk_partial_plan(M, N, K)
    if pp is None:
        return
    bn, split = pp
    assert 1 <= split <= hip.PARTIAL_MAX_SPLIT and split <= K // 64
    # part_k: [PARTIAL_MAX_SPLIT, min(max_prefill_rows, PARTIAL_MAX_ROWS), N] floats, max_prefill_rows >= M
    assert hip.PARTIAL_MAX_SPLIT * min(M_MAX, hip.PARTIAL_MAX_ROWS) * N >= split * M * N
    why = _sk_launch(M, N, K, hip.EPI_PARTIAL, hip.SK_BM, bn, hip.N_CU, 0, split)  # as resid_proj calls it
    assert why is None, why


def _check_wr_plan(M, N, K, epi):
    bn = hip.gemm_wr_plan(M, N, K, epi, hip.EpiArgs())
    if bn is None:
        return
    assert bn in (128, 192, 256) and N % bn == 0 and K % 64 == 0
    assert epi in (hip.EPI_STORE, hip.EPI_QKV, hip.EPI_SWIGLU) and not (epi == hip.EPI_SWIGLU and bn == 192)
    assert routes.route(M, N, K, epi).kernel == "gemm_wr"


def _check_skp_plan(M, N, K):
    p = gemm_skp.plan(M, N, K)
    if p is None:
        return
    assert len(p) == 4 and p[3] in (0, 1)
    why = gemm_skp.check_plan(M, N, K, p[0], p[1], p[2])
    assert why is None, why


def _check_route(M, N, K, epi):
    for e in (None, epi):
        r = routes.route(M, N, K, e)
        assert r.kernel in ("gemv", "gemm_sk", "gemm_wr") and r.lo <= M <= r.hi
        assert r.kernel != "gemv" or M <= routes.GEMV_MAX_ROWS
        assert r.kernel != "gemm_wr" or r.params["bn"] in (128, 192, 256)


def _coop_ws_ok(N, M, cfg, slab, counters):
    tnw, nw, kf, sk = cfg[:4]
    return slab >= packing.coop_slab_floats(N, M, tnw, nw, kf, sk) and counters >= N // 16 // (tnw * nw)


def _check_proj_config(M, N, K, even, ws):
    algo, cfg = packing.proj_config(N // 16, M, need_even=even, k=K)
    if algo == "coop":
        assert packing.coop_norm(cfg) in packing.coop_candidates(N // 16, K, M, even), cfg
        assert _coop_ws_ok(N, M, cfg, *ws), f"coop workspace {ws} too small for {cfg}"
    else:
        tn, nw, u = cfg
        assert algo == "gemv" and M <= 64
        assert (tn, packing.row_blocks(M), nw, u) in packing.GEMV_CONFIGS and (K // 32) % u == 0 and (N // 16) % tn == 0
        assert not even or tn % 2 == 0


def _check_partial_config(M, N, K, ws):
    pc = packing.partial_config(N // 16, M, k=K)
    if pc is None:
        return
    assert M > 16 and pc in packing.coop_candidates(N // 16, K, M) and 1 <= pc[3] <= 8
    assert ws[1] >= N // 16 // (pc[0] * pc[1])


def _check_fp8_config(M, N, K, even, ws):
    algo, cfg = packing.fp8_proj_config(N // 16, M, need_even=even, k=K)
    if algo == "fp8":
        tn, nw, u2 = cfg
        assert M <= 64 and (tn, packing.row_blocks(M), nw, u2) in packing.FP8_CONFIGS
        assert tuple(cfg) in packing.fp8_gemv_candidates(N // 16, K, M, even)
    else:
        assert algo == "coop_fp8" and tuple(cfg) in packing.coop_fp8_candidates(N // 16, K, M), cfg
        assert _coop_ws_ok(N, M, cfg, *ws), f"coop workspace {ws} too small for {cfg}"


def _check_int4_config(M, N, K, even):
    cands = int4.int4_gemv_candidates(N // 16, K, M, even)
    tn, nw, ug = int4.int4_config(N // 16, M, need_even=even, k=K)
    assert (tn, nw, ug) in cands and (tn, packing.row_blocks(M), nw, ug) in int4.INT4_CONFIGS
    assert (N // 16) % tn == 0 and (not even or tn % 2 == 0)


def _engine_coop_ws(shapes) -> tuple:
    """(slab floats, counters) of StageEngine._alloc_runtime's CoopWorkspace for these projections."""
    even = tuple((N, K) for N, K, _, ev in shapes if ev)
    floats, groups = packing.coop_workspace_need([(N, K) for N, K, _, _ in shapes], packing.GEMV_MAX_ROWS, even_n=even)
    return max(floats, 1 << 24), max(groups, 4096)


# ------------------------------------------------------------------------------ the sweep
def _run(errors, what, N, K, M, fn, *args, may_refuse=False):
    """One planner call: an AssertionError or anything but a documented ValueError is a finding."""
    try:
        fn(*args)
    except ValueError as e:
        if not may_refuse:
            errors.append((what, N, K, M, f"ValueError: {e}"))
    except AssertionError as e:
        errors.append((what, N, K, M, f"launcher precondition: {e}"))
    except Exception as e:  # noqa: BLE001 - the point of the sweep
        errors.append((what, N, K, M, f"{type(e).__name__}: {e}"))


def _report(errors) -> str:
    shapes = sorted({e[:4] for e in errors})
    return f"{len(errors)} planner failures at (function, N, K, M) = {shapes[:40]}; first: {errors[:3]}"


def test_gemm_planners_every_row_count():
    """routes.route, gemm_sk_plan, gemm_sk_partial_plan, gemm_wr_plan and gemm_skp.plan for every M
    in 1..2048 (the partial plan: 1..PARTIAL_MAX_ROWS; above it the planner answers None)."""
    hip.gemm_sk_plan.cache_clear()
    errors = []
    for N, K, epis, _evens, _preset in _cases():
        sk_ok = N % 128 == 0 and K % 64 == 0  # what hip.gemm sends to gemm_sk / gemm_wr
        for M in range(1, M_MAX + 1):
            for epi in epis:
                _run(errors, "routes.route", N, K, M, _check_route, M, N, K, epi)
                if sk_ok:
                    _run(errors, "gemm_sk_plan", N, K, M, _check_sk_plan, M, N, K, epi)
                    _run(errors, "gemm_wr_plan", N, K, M, _check_wr_plan, M, N, K, epi)
            if sk_ok:
                if M <= hip.PARTIAL_MAX_ROWS:
                    _run(errors, "gemm_sk_partial_plan", N, K, M, _check_partial_plan, M, N, K)
                else:
                    assert hip.gemm_sk_partial_plan(M, N, K) is None
                _run(errors, "gemm_skp.plan", N, K, M, _check_skp_plan, M, N, K)
    assert not errors, _report(errors)


def test_layer_family_every_row_count():
    for name, shapes in _preset_shapes().items():
        nk = [(N, K) for N, K, _, _ in shapes]
        gmax = routes.gemv_max_rows(nk)
        assert 0 <= gmax <= routes.GEMV_MAX_ROWS, name
        fams = [routes.layer_family(M, nk) for M in range(1, M_MAX + 1)]
        assert set(fams) <= {"gemv", "gemm"} and all(f == "gemm" for f in fams[routes.GEMV_MAX_ROWS:]), name
        # one switch: a layer never returns to the GEMVs above its limit
        assert fams[:routes.GEMV_MAX_ROWS] == ["gemv"] * gmax + ["gemm"] * (routes.GEMV_MAX_ROWS - gmax), name


def test_decode_configs_every_row_count():
    """proj_config, partial_config, fp8_proj_config and the int4 configs for every decode row count
    (1..128; int4: 1..INT4_MAX_ROWS). A preset's own shapes must always get a config; a shape known
    only from a table may be refused with the documented ValueError for a flag it never runs with."""
    errors = []
    by_shape = {}
    for shapes in _preset_shapes().values():
        ws = _engine_coop_ws(shapes)
        for N, K, _, _ in shapes:
            old = by_shape.get((N, K), ws)
            by_shape[(N, K)] = (min(old[0], ws[0]), min(old[1], ws[1]))  # the smallest workspace any engine gives it
    for N, K, _epis, evens, preset in _cases():
        ws = by_shape.get((N, K), (1 << 24, 4096))
        for M in range(1, packing.GEMV_MAX_ROWS + 1):
            for even in evens:
                refuse = not preset
                if N % 16 == 0 and K % 32 == 0:
                    _run(errors, "proj_config", N, K, M, _check_proj_config, M, N, K, even, ws, may_refuse=refuse)
                if N % 16 == 0 and K % 64 == 0:
                    _run(errors, "fp8_proj_config", N, K, M, _check_fp8_config, M, N, K, even, ws, may_refuse=refuse)
                if N % 16 == 0 and K % int4.INT4_GROUP == 0 and M <= int4.INT4_MAX_ROWS:
                    _run(errors, "int4_config", N, K, M, _check_int4_config, M, N, K, even, may_refuse=refuse)
            if N % 16 == 0 and K % 32 == 0:
                _run(errors, "partial_config", N, K, M, _check_partial_config, M, N, K, ws)
        assert int4.int4_gemv_candidates(N // 16, K, int4.INT4_MAX_ROWS + 1) == []
    assert not errors, _report(errors)


# ------------------------------------------------------------------------------ the tie rule
def test_live_ties_take_the_lower_row_count():
    """The two shapes whose tuned row counts are equally far from a row count in between: the
    Llama-2-7B down projection at 704 rows (640 | 768) and the Llama-2-70B one at 448 (384 | 512)."""
    for (N, K), M, lo, hi in (((4096, 11008), 704, 640, 768), ((8192, 28672), 448, 384, 512)):
        tab = dict(hip._sk_partial()[(N, K)])
        assert lo in tab and hi in tab and (tab[lo] is None) != (tab[hi] is None), (N, K, tab)
        want = tab[lo]
        assert hip.gemm_sk_partial_plan(M, N, K) == (None if want is None else tuple(want))


@pytest.mark.parametrize("lo_plan,hi_plan", [(None, [128, 2]), ([128, 2], None), ([256, 4], [128, 2]), ([128, 2], [256, 4]),
                                             (None, None)])
@pytest.mark.parametrize("order", [0, 1])
def test_partial_plan_tie_ignores_what_the_entries_hold(monkeypatch, lo_plan, hi_plan, order):
    """Two entries at the same distance: the lower row count's, whatever either holds and in
    whichever order the table lists them."""
    ents = [(640, lo_plan), (768, hi_plan)]
    monkeypatch.setattr(hip, "_SK_PARTIAL", {(4096, 4096): ents[::-1] if order else ents})
    want = None if lo_plan is None else tuple(lo_plan)
    assert hip.gemm_sk_partial_plan(704, 4096, 4096) == want
    assert hip.gemm_sk_partial_plan(703, 4096, 4096) == want                       # nearer to 640
    assert hip.gemm_sk_partial_plan(705, 4096, 4096) == (None if hi_plan is None else tuple(hi_plan))
    assert hip.gemm_sk_partial_plan(512, 4096, 4096) is None                       # another 256-row tile count


@pytest.mark.parametrize("order", [0, 1])
def test_sk_plan_tie_ignores_what_the_entries_hold(monkeypatch, order):
    """gemm_sk_plan states the same rule (its table has no tie today: next test)."""
    for lo_cfg, hi_cfg in (((256, 256, 1, 4), (128, 256, 1, 0)), ((128, 256, 1, 0), (256, 256, 1, 4))):
        ents = [(400, lo_cfg), (432, hi_cfg)]
        monkeypatch.setattr(hip, "_SK_TUNED", {(4096, 4096): ents[::-1] if order else ents})
        hip.gemm_sk_plan.cache_clear()
        try:
            assert hip.gemm_sk_plan(416, 4096, 4096) == (lo_cfg[0], hip.N_CU, lo_cfg[2], lo_cfg[3], hip.SK_BM)
            assert hip.gemm_sk_plan(417, 4096, 4096) == (hi_cfg[0], hip.N_CU, hi_cfg[2], hi_cfg[3], hip.SK_BM)
        finally:
            hip.gemm_sk_plan.cache_clear()


def test_sk_table_has_no_tie():
    """gemm_sk_plan's classes are 128-row tiles and every tuned row count is a multiple of 128, so
    each class holds at most one measured row count and no row count has two nearest entries."""
    assert hip._sk_tuned()
    for (N, K), ents in hip._sk_tuned().items():
        ms = [m for m, _ in ents]
        assert all(m % 128 == 0 for m in ms), (N, K, ms)
        assert len(set(ms)) == len(ms), (N, K, ms)
