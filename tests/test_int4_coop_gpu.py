"""The cooperative int4 (W4A16) GEMV for 17..128 rows (csrc/quant/gemv_coop_int4.hip) on the GPU:
the exact suite of tests/int4_cases.py over every built config and every K split it admits, the
one-hot code case, the same bits as the plain int4 kernel, replay in a captured graph, the
dispatcher and the refusals, and int4 engines at 96 and 128 decode rows."""
from collections import Counter

import pytest
import torch

import contract_cases as C
import exact_cases as X
import int4_cases as I4
import test_int4_gpu as T
from llm_sharding_amd.ops import int4, packing
from llm_sharding_amd.utils.numerics import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROWS = (17, 33, 65, 128)      # one valid row in the last row block (17, 65), a full one (128)
KS = (128, 384, 1024)         # one group; an odd group count against 2 splits; eight groups against 2 / 4 / 8
QKV_TILES = 12                # tests/int4_cases.py QKV_GEOM: N = 192, for workgroups of 4 tiles
QKV_GEOM_16 = (4, 2, 32)      # n_heads, n_kv, head_dim: N = 256 = 16 tiles, for workgroups of 8 tiles
_QKV16 = {}


def n_for(tnw, nw):
    """Two column groups of the config's workgroup width."""
    return 16 * tnw * nw * 2


def splits(tnw, nw, d, n_tiles, K, M, even=False):
    return [c[3] for c in int4.int4_coop_candidates(n_tiles, K, M, even) if c[:3] == (tnw, nw, d)]


def qkv_case(tiles_per_wg, M, K, rope, monkeypatch, device=DEV):
    """int4_cases' QKV case: its own 12 tiles where the workgroup width divides them, else the
    same builder at QKV_GEOM_16 (built once per shape, read-only)."""
    if QKV_TILES % tiles_per_wg == 0:
        return I4.case("qkv", M, K, rope, device=device)
    key = (M, K, rope, device)
    if key not in _QKV16:
        monkeypatch.setattr(I4, "QKV_GEOM", QKV_GEOM_16)
        _QKV16[key] = I4.build_qkv(M, K, 1000 * M + K + int(rope), device, rope=rope)
        monkeypatch.undo()
    return _QKV16[key]


def l_coop(h, cfg=None, ws=None):
    def f(x, w, M, N, K, epi, ep, ar, norm, eps=T.EPS):
        int4.gemv_coop_int4(x, w.wq, w.sc, M, N, K, epi, ep, norm=norm, eps=eps, ws=ws, a_rows=ar, cfg=cfg)
    return f


@pytest.mark.parametrize("cfg", int4.INT4_COOP_CONFIGS)
def test_exact_every_config(cfg, monkeypatch):
    h = T.hip()
    mb, tnw, nw, d = cfg
    N = n_for(tnw, nw)
    ran = Counter()
    for M in (m for m in ROWS if packing.row_blocks(m) == mb):
        for K in KS:
            sks = splits(tnw, nw, d, N // 16, K, M)
            assert sks == [s for s in int4.INT4_COOP_SPLITS if s <= K // 128]
            for sk in sks:
                launch, what = l_coop(h, (tnw, nw, d, sk)), f"coop int4 {cfg} sk {sk}"
                lin = I4.case("linear", M, N, K, device=DEV)
                ran["linear"] += T._linear(h, launch, lin, ("store", "store_bias", "resid", "resid_bias"), what)
                if K >= I4.K_ROUND_MIN:
                    ran["round_once"] += T._linear(h, launch, I4.case("round_once", M, N, K, device=DEV),
                                                   ("store", "resid", "resid_bias"), what)
                ran["swiglu"] += T._swiglu(h, launch, I4.case("swiglu", M, N // 2, K, device=DEV), what)
                ran["qkv_rope"] += T._qkv(h, launch, qkv_case(tnw * nw, M, K, True, monkeypatch), what)
                ran["qkv_bias"] += T._qkv(h, launch, qkv_case(tnw * nw, M, K, False, monkeypatch), what)
                ran["gelu"] += T._gelu(h, launch, I4.case("gelu", M, N, K, device=DEV), what)
                ran["a_rows"] += T._a_rows(h, launch, lin, what)
                ran["norm"] += T._norm(h, launch, I4.case("norm", M, N, K, device=DEV), what)
    kinds = ["linear", "round_once", "swiglu", "gelu", "a_rows", "norm", "qkv_rope", "qkv_bias"]
    assert all(ran[k] > 0 for k in kinds), (cfg, dict(ran))


def test_every_code_value_in_every_position():
    """tests/test_int4_gpu.py's one-hot case, 17 rows at a time: the one tile of its weights
    repeated four times side by side (a workgroup owns at least four tiles)."""
    h = T.hip()
    c = I4.case("one_hot", device=DEV)
    wq, sc, N = c.W.wq.repeat(4), c.W.sc.repeat(4, 1, 1), 4 * c.N
    for r0 in (*range(0, c.M - 17, 17), c.M - 17):             # 0, 17, ..., 102 and 111: all 128 one-hot rows
        obuf, out = C.guarded(17, N, device=DEV)
        int4.gemv_coop_int4(c.a[r0:r0 + 17].contiguous(), wq, sc, 17, N, c.K, h.EPI_STORE,
                            h.make_epi(out=out, ldo=out.stride(0)), cfg=(1, 4, 4, 1))
        torch.cuda.synchronize()
        C.assert_footprint(obuf, out, what=f"coop one-hot rows {r0}..{r0 + 17}")
        X.assert_bits_equal(out, c.exp[r0:r0 + 17].repeat(1, 4), f"coop {c.tag} rows {r0}..{r0 + 17}")


@pytest.mark.parametrize("M", [17, 33, 64])
def test_same_bits_as_the_plain_kernel(M, monkeypatch):
    """The two kernels share one contract: on operands whose group partial sums are exact in fp32
    their outputs are the same bits (store, residual with and without bias, QKV with RoPE and KV
    append on a workgroup of 8 tiles with 2 K splits)."""
    h = T.hip()
    c = I4.case("linear", M, 128, 384, device=DEV)
    for form in ("store", "resid", "resid_bias"):
        outs = []
        for fn in (int4.gemv_int4, int4.gemv_coop_int4):
            out = torch.zeros(M, c.N, dtype=torch.bfloat16, device=DEV)
            if form == "store":
                fn(c.a, c.W.wq, c.W.sc, M, c.N, c.K, h.EPI_STORE, h.make_epi(out=out, ldo=c.N))
            else:
                fn(c.a, c.W.wq, c.W.sc, M, c.N, c.K, h.EPI_RESID,
                   h.make_epi(out=out, resid=c.resid, ldo=c.N, ldr=c.N, bias=c.bias if form == "resid_bias" else None))
            outs.append(out)
        X.assert_bits_equal(outs[1], outs[0], f"coop vs plain int4 {form} {M} rows")
    q = qkv_case(8, M, 384, True, monkeypatch)
    res = []
    for fn, kw in ((int4.gemv_int4, {}), (int4.gemv_coop_int4, {"cfg": (1, 8, 4, 2)})):
        qo = torch.zeros(M, q.nh * q.hd, dtype=torch.bfloat16, device=DEV)
        kc, vc = (torch.zeros(q.slots, q.nkv, q.t_max, q.hd, dtype=torch.bfloat16, device=DEV) for _ in range(2))
        fn(q.a, q.W.wq, q.W.sc, M, q.N, q.K, h.EPI_QKV,
           h.make_epi(out=qo, k_cache=kc, v_cache=vc, slot=q.slot, pos=q.pos, cos=q.cos, sin=q.sin, ldo=qo.stride(0),
                      n_heads=q.nh, n_kv=q.nkv, head_dim=q.hd, t_max=q.t_max), **kw)
        res.append((qo, kc, vc))
    for a, b, name in zip(res[1], res[0], "qkv"):
        X.assert_bits_equal(a, b, f"coop vs plain int4 qkv {name} {M} rows")


def test_replay_in_a_captured_graph():
    """A split launch captured once and replayed three times gives the eager bits every time,
    and the arrival counters are back at zero."""
    h = T.hip()
    c = I4.case("linear", 65, 256, 1024, device=DEV)
    ws = h.CoopWorkspace(DEV, slab_floats=1 << 20, groups=64)
    out = torch.zeros(65, c.N, dtype=torch.bfloat16, device=DEV)
    ep = h.make_epi(out=out, resid=c.resid, ldo=c.N, ldr=c.N, bias=c.bias)

    def run():
        int4.gemv_coop_int4(c.a, c.W.wq, c.W.sc, 65, c.N, c.K, h.EPI_RESID, ep, ws=ws, cfg=(1, 8, 3, 4))
    run()
    torch.cuda.synchronize()
    X.assert_bits_equal(out, c.exp["resid_bias"], "coop int4 eager")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    for i in range(3):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        X.assert_bits_equal(out, c.exp["resid_bias"], f"coop int4 replay {i}")
        assert int(ws.counters.abs().sum()) == 0


def test_dispatch_and_argument_checks():
    h = T.hip()
    assert int4.int4_coop_config(3, 384, 65) is None           # 3 tiles: no workgroup width divides them
    for M in (65, 128):                                        # above the plain kernel's rows: the cooperative one
        c = I4.case("linear", M, 128, 384, device=DEV)
        obuf, out = C.guarded(M, c.N, device=DEV)
        assert int4.proj_int4(c.a, c.W.wq, c.W.sc, M, c.N, c.K, h.EPI_STORE, h.make_epi(out=out, ldo=out.stride(0))) is True
        torch.cuda.synchronize()
        C.assert_footprint(obuf, out, what=f"proj_int4 {M} rows")
        X.assert_bits_equal(out, c.exp["store"], f"proj_int4 {M} rows")
    c = I4.case("linear", 65, 48, 384, device=DEV)
    obuf, out = C.guarded(65, 48, device=DEV)
    ep = h.make_epi(out=out, ldo=out.stride(0))
    assert int4.proj_int4(c.a, c.W.wq, c.W.sc, 65, 48, 384, h.EPI_STORE, ep) is False
    torch.cuda.synchronize()
    assert bool(C.is_sentinel(obuf).all())                     # declined: nothing launched
    c = I4.case("linear", 65, 128, 384, device=DEV)
    out = torch.empty(129, 128, dtype=torch.bfloat16, device=DEV)
    ep, x = h.make_epi(out=out, ldo=128), torch.zeros(129, 384, dtype=torch.bfloat16, device=DEV)
    args = (65, 128, 384, h.EPI_STORE, ep)
    for bad in (lambda: int4.gemv_coop_int4(x, c.W.wq, c.W.sc, 16, 128, 384, h.EPI_STORE, ep),           # rows
                lambda: int4.gemv_coop_int4(x, c.W.wq, c.W.sc, 129, 128, 384, h.EPI_STORE, ep),
                lambda: int4.gemv_coop_int4(x, c.W.wq[:-16], c.W.sc, *args),                             # weight bytes
                lambda: int4.gemv_coop_int4(x, c.W.wq, c.W.sc.view(-1)[:-1], *args),                     # scales
                lambda: int4.gemv_coop_int4(x, c.W.wq, c.W.sc, *args, cfg=(1, 8, 3, 2),
                                            ws=h.CoopWorkspace(DEV, slab_floats=1024, groups=64)),       # workspace
                lambda: int4.gemv_coop_int4(x, c.W.wq, c.W.sc, *args, cfg=(1, 8, 3, 4)),                 # 3 groups, 4 splits
                lambda: int4.gemv_coop_int4(x, c.W.wq, c.W.sc, *args, cfg=(3, 8, 3, 1)),                 # not built
                lambda: int4.gemv_coop_int4(x, c.W.wq, c.W.sc, 65, 128, 384, h.EPI_ARGMAX,
                                            h.make_epi(keys=torch.zeros(65, dtype=torch.int64, device=DEV)))):
        with pytest.raises(ValueError):
            bad()


@pytest.mark.parametrize("kind", ["llama", "gpt2"])
def test_engine_decodes_96_and_128_rows_without_dequantising(kind, monkeypatch):
    """The int4 engine against the bf16 engine on the same effective weights at 96 and 128 decode
    rows; at 128 rows with a dequantise kernel that raises: every projection ran on int4."""
    cfg, e16, (e4,) = T._engines(kind, max_slots=128)
    T._same_effective_weights(cfg, e16, e4)
    g = torch.Generator().manual_seed(3)
    for rows in (96, 128):
        if rows == 128:
            def no_dequant(*a, **k):
                raise AssertionError("the decode forward dequantised a projection")
            monkeypatch.setattr(int4, "dequant_int4_packed", no_dequant)
        toks = torch.randint(3, cfg.vocab_size - 1, (rows,), generator=g)
        hs = []
        for e in (e16, e4):
            slots = list(range(rows))
            for s_ in slots:
                e.seq_len[s_] = 0
            sl, po = e.prefill_rows(slots, [1] * rows)
            hs.append(e.forward(e.embed(toks.to(DEV)), sl, po).clone())
        err = rel_err(hs[1], hs[0])
        print(f"{kind} int4 decode {rows} rows: rel err {float(err):.3e}")
        assert err < T.ENGINE_TOL, rows
