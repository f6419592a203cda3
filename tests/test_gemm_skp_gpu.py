"""lsa_gemm_skp (csrc/gemm_skp/gemm_skp.hip): gemm_sk's split-K GEMM with the fix-up shared by all
contributors of a tile. Shapes are the smallest at which the band hand-off can go wrong: one to
four row tiles with a ragged last one, one to three column tiles, 2 / 3 / 8 / 11 K-tiles (ranges
that divide unevenly), every tile shape, 2 / 3 / 4 / 8 contributors.

* bitwise equality with lsa_gemm_sk at the same (bm, bn, split): same partials, same summation
  order, so every output bit and every ss_out value;
* exact-integer operands against the integer result rounded once to bf16, bitwise;
* random data against fp32 torch at the threshold tests/test_gemm_sk_gpu.py uses (8e-3 on the
  global + worst-tile + worst-row metric of utils/numerics.py);
* 20 back-to-back launches: equal bits, every ticket counter zero after each;
* write footprint: guard rows and columns around out and ss_out untouched;
* the engine route: LSA_GEMM_SKP=0 against =1 on a 2-layer Llama-2-7B-shaped engine at 512 rows.
"""
import ctypes

import pytest
import torch

from llm_sharding_amd.ops import packing
from llm_sharding_amd.utils.numerics import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"

MS = (129, 256, 512)
NS = (128, 256, 384)
KS = (128, 192, 512, 704)
TILES = ((128, 128), (256, 128), (256, 256))
CONTRIBUTORS = (2, 3, 4, 8)
TOL = 8e-3  # tests/test_gemm_sk_gpu.py, store / residual epilogues


def mods():
    from llm_sharding_amd.ops import gemm_skp, hip
    hip.lib()
    return hip, gemm_skp


@pytest.fixture(scope="module")
def ws():
    return mods()[0].SkWorkspace(DEV, grid=1024, bn=256)


@pytest.fixture(scope="module")
def data():
    """Operands and fp32 references, made once: a[M_max, K_max], w per (N, K), residual r."""
    g = torch.Generator(device=DEV).manual_seed(11)
    a = torch.randn(max(MS), max(KS), device=DEV, generator=g).to(torch.bfloat16)
    r = torch.randn(max(MS), max(NS), device=DEV, generator=g).to(torch.bfloat16)
    w, ref = {}, {}
    for N in NS:
        for K in KS:
            w[N, K] = (torch.randn(N, K, device=DEV, generator=g) * 0.05).to(torch.bfloat16)
            ref[N, K] = a[:, :K].float() @ w[N, K].float().T
    return a, r, w, ref


def _cases(bm, bn):
    for N in NS:
        if N % bn:
            continue
        for K in KS:
            for C in CONTRIBUTORS:
                yield N, K, C


def _sk(h, ws, a, wp, M, N, K, epi, ep, bm, bn, C):
    tiles = -(-M // bm) * (N // bn)
    h.gemm_sk(a, wp, M, N, K, epi, ep, bn=bn, grid=tiles * C, dp=0, split=C, bm=bm, ws=ws)


@pytest.mark.parametrize("bm,bn", TILES)
@pytest.mark.parametrize("M", MS)
def test_bitwise_equal_to_gemm_sk_and_close_to_fp32(M, bm, bn, ws, data):
    h, skp = mods()
    a, r, w, ref = data
    ran = 0
    for N, K, C in _cases(bm, bn):
        A = a[:M, :K].contiguous()
        wp = packing.pack_b(w[N, K])
        tag = (M, N, K, bm, bn, C)
        if K // 64 < C:  # fewer K-tiles than contributors: refused by the binding and by the kernel's host entry
            out = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
            assert skp.check_plan(M, N, K, bm, bn, C) is not None
            with pytest.raises(ValueError):
                skp.gemm_skp(A, wp, M, N, K, h.EPI_STORE, h.make_epi(out=out, ldo=N), bm=bm, bn=bn, contributors=C, ws=ws)
            ep = h.make_epi(out=out, ldo=N)
            rc = skp._lib().lsa_gemm_skp(h._p(A), K, h._p(wp), M, N, K, h.EPI_STORE, ctypes.byref(ep), bm, bn, 0, C, 0, 8,
                                         h._p(ws.slab), h._p(ws.counters), ws.slab.numel(), ws.counters.numel(), h._stream())
            assert rc == 1, tag  # LSA_BAD_SHAPE
            assert int(out.abs().sum()) == 0
            continue
        for tm in (0, 1):
            # EPI_STORE
            o_sk = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
            o_p = torch.zeros_like(o_sk)
            _sk(h, ws, A, wp, M, N, K, h.EPI_STORE, h.make_epi(out=o_sk, ldo=N), bm, bn, C)
            skp.gemm_skp(A, wp, M, N, K, h.EPI_STORE, h.make_epi(out=o_p, ldo=N), bm=bm, bn=bn, contributors=C,
                         tile_major=tm, ws=ws)
            assert torch.equal(o_p, o_sk), ("store", tm) + tag
            if tm == 0:  # (tile_major 1 has the same bits)
                e = rel_err(o_p, ref[N, K][:M])
                assert e < TOL, ("store", e) + tag
            # EPI_RESID without and with ss_out (in place, as the engine runs it)
            for with_ss in (False, True):
                x_sk, x_p = r[:M, :N].clone(memory_format=torch.contiguous_format), r[:M, :N].clone(memory_format=torch.contiguous_format)
                s_sk = torch.full((M, N // 64), -1.0, device=DEV) if with_ss else None
                s_p = torch.full((M, N // 64), -2.0, device=DEV) if with_ss else None
                _sk(h, ws, A, wp, M, N, K, h.EPI_RESID, h.make_epi(out=x_sk, resid=x_sk, ldo=N, ldr=N, ss_out=s_sk), bm, bn, C)
                skp.gemm_skp(A, wp, M, N, K, h.EPI_RESID, h.make_epi(out=x_p, resid=x_p, ldo=N, ldr=N, ss_out=s_p),
                             bm=bm, bn=bn, contributors=C, tile_major=tm, ws=ws)
                assert torch.equal(x_p, x_sk), ("resid", with_ss, tm) + tag
                if with_ss:
                    assert torch.equal(s_p, s_sk), ("ss_out", tm) + tag
                if tm == 0:
                    e = rel_err(x_p, r[:M, :N].float() + ref[N, K][:M])
                    assert e < TOL, ("resid", with_ss, e) + tag
        ran += 1
    assert ran >= 4
    assert int(ws.counters.abs().sum()) == 0


@pytest.mark.parametrize("bm,bn", TILES)
def test_exact_integer_operands(bm, bn, ws):
    """A = +-1, W in {-1, 0, 1}: every fp32 partial sum is an exact integer in any order, so the
    only correct output is the integer result (plus an integer residual) rounded once to bf16."""
    h, skp = mods()
    g = torch.Generator(device=DEV).manual_seed(5)
    for M in MS:
        for N, K, C in _cases(bm, bn):
            if K // 64 < C:
                continue
            a = (torch.randint(0, 2, (M, K), device=DEV, generator=g) * 2 - 1).to(torch.bfloat16)
            w = (torch.randint(0, 3, (N, K), device=DEV, generator=g) - 1).to(torch.bfloat16)
            res = torch.randint(-64, 65, (M, N), device=DEV, generator=g).to(torch.bfloat16)
            want = a.double() @ w.double().T
            wp = packing.pack_b(w)
            out = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
            skp.gemm_skp(a, wp, M, N, K, h.EPI_STORE, h.make_epi(out=out, ldo=N), bm=bm, bn=bn, contributors=C, ws=ws)
            assert torch.equal(out, want.to(torch.bfloat16)), (M, N, K, C)
            x = res.clone()
            skp.gemm_skp(a, wp, M, N, K, h.EPI_RESID, h.make_epi(out=x, resid=x, ldo=N, ldr=N), bm=bm, bn=bn,
                         contributors=C, tile_major=1, ws=ws)
            assert torch.equal(x, (want + res.double()).to(torch.bfloat16)), (M, N, K, C)


@pytest.mark.parametrize("bm,bn,C", [(128, 128, 2), (256, 128, 4), (256, 256, 8), (128, 128, 3)])
def test_back_to_back_launches_and_counters(bm, bn, C, ws, data):
    h, skp = mods()
    a, r, w, ref = data
    M, N, K = 512, 256, 704
    A, wp = a[:M, :K].contiguous(), packing.pack_b(w[N, K])
    outs, sss, cnts = [], [], []
    for _ in range(20):  # no host synchronisation between the launches
        x = r[:M, :N].clone(memory_format=torch.contiguous_format)
        s = torch.zeros(M, N // 64, device=DEV)
        skp.gemm_skp(A, wp, M, N, K, h.EPI_RESID, h.make_epi(out=x, resid=x, ldo=N, ldr=N, ss_out=s), bm=bm, bn=bn,
                     contributors=C, ws=ws)
        outs.append(x)
        sss.append(s)
        cnts.append(ws.counters.clone())
    for x, s, c in zip(outs, sss, cnts):
        assert torch.equal(x, outs[0]) and torch.equal(s, sss[0])
        assert int(c.abs().sum()) == 0
    assert rel_err(outs[0], r[:M, :N].float() + ref[N, K][:M]) < TOL


@pytest.mark.parametrize("bm,bn,C", [(128, 128, 3), (256, 128, 4), (256, 256, 8)])
def test_write_footprint(bm, bn, C, ws, data):
    """Guard rows and columns around out, guard rows around ss_out (ss_out rows are N / 64 floats,
    contiguous: no column guard exists) keep their fill."""
    h, skp = mods()
    a, r, w, ref = data
    M, N, K, G = 129, 256, 512, 8
    A, wp = a[:M, :K].contiguous(), packing.pack_b(w[N, K])
    fill = 7.0
    big = torch.full((M + 2 * G, N + 2 * G), fill, dtype=torch.bfloat16, device=DEV)
    big[G:G + M, G:G + N] = r[:M, :N]
    ssb = torch.full((M + 2 * G, N // 64), fill, device=DEV)
    inner = big[G:, G:]
    skp.gemm_skp(A, wp, M, N, K, h.EPI_RESID,
                 h.make_epi(out=inner, resid=inner, ldo=big.stride(0), ldr=big.stride(0), ss_out=ssb[G:G + M]),
                 bm=bm, bn=bn, contributors=C, ws=ws)
    got = big[G:G + M, G:G + N]
    assert rel_err(got, r[:M, :N].float() + ref[N, K][:M]) < TOL
    mask = torch.ones_like(big, dtype=torch.bool)
    mask[G:G + M, G:G + N] = False
    assert bool((big[mask] == fill).all())
    assert bool((ssb[:G] == fill).all()) and bool((ssb[G + M:] == fill).all())
    want_ss = got.float().pow(2).view(M, N // 64, 64).sum(-1)
    assert rel_err(ssb[G:G + M], want_ss) < 1e-5


def _sk_equal_ranges(h, rows, N, K):
    """(bm, bn, C) when gemm_sk's own plan of the shape splits every tile into C equal K ranges
    (split mode in one round, or stream-K whose iterations divide evenly), else None: a gemm_skp
    plan equal to it sums the same partials in the same order."""
    bn, grid, dp, split, bm = h.gemm_sk_plan(rows, N, K)
    nkt, tiles = K // 64, -(-rows // bm) * -(-N // bn)
    if bn == 192 or tiles > grid or (dp and tiles == grid):
        return None
    if split > 0:
        return (bm, bn, min(split, nkt, grid // tiles))
    if grid % tiles == 0 and nkt % (grid // tiles) == 0:
        return (bm, bn, grid // tiles)
    return None


def test_engine_route_on_and_off(monkeypatch):
    """One 512-row decode step of a 2-layer Llama-2-7B-shaped engine with the route off and on.
    Where the table keeps gemm_sk's own tile and split for both projections the hidden states are
    bitwise equal; otherwise they agree at the tolerance tests/test_engine_gpu.py holds the engine
    to against the golden model (3e-2)."""
    h, skp = mods()
    from llm_sharding_amd.config import get_preset
    from llm_sharding_amd.runtime.engine import RandomSource
    from llm_sharding_amd.runtime.engine_int4 import make_stage_engine
    from llm_sharding_amd.runtime.engine_skp import SkpStageEngine
    cfg = get_preset("llama2-7b")
    rows = 512
    e = make_stage_engine(cfg, 0, 2, DEV, torch.bfloat16, source=RandomSource(cfg, 3), max_slots=rows, max_seq=16,
                          max_prefill_rows=rows)
    assert type(e) is SkpStageEngine
    H, I = cfg.hidden_size, cfg.intermediate_size
    g = torch.Generator(device=DEV).manual_seed(9)
    x = torch.randn(rows, H, device=DEV, generator=g).to(torch.bfloat16)
    outs = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("LSA_GEMM_SKP", flag)
        e.reset()
        slot, pos = e.prefill_rows(list(range(rows)), [1] * rows)
        plans = e.skp_plans(rows)
        assert (plans is None) if flag == "0" else True
        outs[flag] = e._forward_hip(x.clone(), e._i32(slot), e._i32(pos), None, rows, nsplit=e.decode_nsplit(rows)).clone()
        outs["plans" + flag] = plans
    plans = outs["plans1"]
    assert bool(torch.isfinite(outs["1"].float()).all())
    same_bits = all(p is None or _sk_equal_ranges(h, rows, N, K) == p[:3]
                    for (N, K), p in zip(((H, cfg.q_size), (H, I)), plans or (None, None)))
    if same_bits:
        assert torch.equal(outs["1"], outs["0"])
    else:
        assert rel_err(outs["1"], outs["0"]) < 3e-2
