"""The exact-arithmetic harness (tests/exact_cases.py) catches what it claims to, shown without a
GPU: for a small shape of every case the "kernel" output is computed with plain torch and passes
the checker bitwise; then one mutation at a time - one product dropped or duplicated, one K step
of one tile taken from the neighbouring column tile, y rounded before the residual add,
truncation or round-half-up for round-to-nearest-even, a negated sin in the upper frequencies, a
wrong RoPE partner, the largest tied index for the smallest - must fail it. Every builder also
runs at every shape the GPU file uses, so a shape that breaks a builder's condition (the bound
of 256, every k used, the tie and double-rounding shares, the gate window) is found here."""
import pytest
import torch

import contract_cases as C
import exact_cases as X


def _fails(fn, *args, match=None, **kw):
    with pytest.raises(AssertionError, match=match):
        fn(*args, **kw)


@pytest.fixture(scope="module")
def lin():
    return X.build_linear(40, 64, 512, seed=1)


@pytest.fixture(scope="module")
def lin_fp8():
    return X.build_linear(40, 64, 512, seed=2, fp8=True)


@pytest.fixture(scope="module")
def ro():
    return X.build_linear(48, 64, 1024, seed=3, mode="round_once")


def _nonzero_product(case, m=17, n=35):
    k = int((case.w[n] != 0).nonzero()[5])
    return m, n, k, float(case.a[m, k]) * float(case.W.ref[n, k])


# ------------------------------------------------------------------------------ exact_int
@pytest.mark.parametrize("fp8", [False, True])
def test_exact_int_unmutated_passes(lin, lin_fp8, fp8):
    c = lin_fp8 if fp8 else lin
    y = c.a.double() @ c.W.ref.T
    bias = c.bias.double()
    X.assert_bits_equal(X.bf16_rne(y), c.exp["store"], "store", unit=c.unit)
    X.assert_bits_equal(X.bf16_rne(y + bias), c.exp["store_bias"], "store + bias")
    X.assert_bits_equal(X.bf16_rne(c.resid.double() + y), c.exp["resid"], "resid")
    X.assert_bits_equal(X.bf16_rne(c.resid.double() + y + bias), c.exp["resid_bias"], "resid + bias")
    for k, v in c.exp.items():  # the expected output IS the exact matrix: nothing was rounded
        assert float((v.double() / c.unit).abs().max()) <= X.BF16_INT_MAX
    assert torch.equal(c.exp["resid_bias"].double(), c.resid.double() + y + bias)
    if not fp8:  # the per-64-column sums of squares of integer outputs are exact in fp32
        ss = X.expected_ss(c.exp["resid"])
        assert torch.equal(ss, c.exp["resid"].float().pow(2).view(c.M, c.N // 64, 64).sum(-1))


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("form", ["store", "resid_bias"])
def test_one_product_dropped_or_duplicated(lin, lin_fp8, fp8, form):
    c = lin_fp8 if fp8 else lin
    m, n, k, prod = _nonzero_product(c)
    base = c.y + (c.resid.double() + c.bias.double() if form == "resid_bias" else 0)
    for sign in (-1, 1):  # dropped, duplicated
        y = base.clone()
        y[m, n] += sign * prod
        reads = "-1" if sign * prod < 0 else r"\+1"
        _fails(X.assert_bits_equal, y.float().to(torch.bfloat16), c.exp[form], "mutated", unit=c.unit,
               match=r"1 of \d+ element.*\(17, 35\).*difference " + reads + " products")


def test_k_step_from_the_neighbouring_column_tile(lin):
    c = lin
    m0, n0, k0 = 16, 32, 64
    a = c.a.double()[m0:m0 + 16, k0:k0 + 32]
    own, other = c.W.ref[n0:n0 + 16, k0:k0 + 32], c.W.ref[n0 + 16:n0 + 32, k0:k0 + 32]
    y = c.y.clone()
    y[m0:m0 + 16, n0:n0 + 16] += a @ (other - own).T
    _fails(X.assert_bits_equal, y.float().to(torch.bfloat16), c.exp["store"], "mutated", unit=c.unit)
    # and a whole 32-wide K step left out reads off as a difference of at most 32 products
    y = c.y.clone()
    y[m0:m0 + 16, n0:n0 + 16] -= a @ own.T
    _fails(X.assert_bits_equal, y.float().to(torch.bfloat16), c.exp["store"], "mutated", unit=c.unit, match="products")


# ------------------------------------------------------------------------------ round_once
def test_round_once_unmutated_passes(ro):
    c = ro
    assert c.stats["tie_share"] >= X.MIN_SHARE and c.stats["double_rounding_share"] >= X.MIN_SHARE
    X.assert_bits_equal(c.y.float().to(torch.bfloat16), c.exp["store"], "store")
    X.assert_bits_equal((c.resid.float() + c.y.float()).to(torch.bfloat16), c.exp["resid"], "resid")
    X.assert_bits_equal((c.resid.float() + c.y.float() + c.bias).to(torch.bfloat16), c.exp["resid_bias"], "resid + bias")


def test_y_rounded_before_the_residual_add(ro):
    c = ro
    twice = (c.resid.float() + c.y.float().to(torch.bfloat16).float()).to(torch.bfloat16)
    _fails(X.assert_bits_equal, twice, c.exp["resid"], "double rounding")


def test_truncation_and_round_half_up(ro):
    c = ro
    _fails(X.assert_bits_equal, X.bf16_trunc(c.y), c.exp["store"], "truncation")
    _fails(X.assert_bits_equal, X.bf16_half_up(c.y), c.exp["store"], "round half up")
    # half-up differs from RNE at ties only, and only at those that RNE rounds to the even side
    diff = C.bits(X.bf16_half_up(c.y)) != C.bits(c.exp["store"])
    assert bool((diff <= X.is_tie(c.y)).all()) and 0 < int(diff.sum()) < int(X.is_tie(c.y).sum())
    # the faulty conversions are what they say on values that are not ties
    x = torch.tensor([257.0, 258.0, 259.0, -257.0, -259.0, 1.0], dtype=torch.float64)
    assert X.bf16_rne(x).tolist() == [256.0, 258.0, 260.0, -256.0, -260.0, 1.0]
    assert X.bf16_trunc(x).tolist() == [256.0, 258.0, 258.0, -256.0, -258.0, 1.0]
    assert X.bf16_half_up(x).tolist() == [258.0, 258.0, 260.0, -258.0, -260.0, 1.0]


def test_round_once_builder_refuses_a_shape_without_ties():
    _fails(X.build_linear, 16, 64, 64, seed=4, mode="round_once", match="ties")


def test_exact_int_builder_refuses_a_result_above_256(monkeypatch):
    assert abs(float((X.ternary(64, 4096, X.gen(0), "cpu") != 0).float().mean()) - 0.25) < 0.02
    monkeypatch.setattr(X, "density_for", lambda K: 1.0)  # dense weights at K = 4096 reach about 300
    _fails(X.build_linear, 64, 256, 4096, seed=4, match="lower the density")


# ------------------------------------------------------------------------------ SwiGLU
@pytest.mark.parametrize("fp8", [False, True])
def test_swiglu_saturated_gate(fp8):
    c = X.build_swiglu(24, 64, 512, seed=5, fp8=fp8)
    gu = (c.a.float() @ c.W.ref.float().T).view(c.M, c.I // 16, 2, 16)
    g, u = gu[:, :, 0].reshape(c.M, c.I), gu[:, :, 1].reshape(c.M, c.I)
    assert torch.equal(1.0 + torch.exp(-g), torch.ones_like(g))             # fp32: silu(g) is exactly g
    X.assert_bits_equal(((g / (1.0 + torch.exp(-g))) * u).to(torch.bfloat16), c.exp, "swiglu")
    m, n = 3, 21
    k = int((c.W.ref.view(c.I // 16, 2, 16, c.K)[n // 16, 1, n % 16] != 0).nonzero()[2])
    u2 = u.clone()
    u2[m, n] -= float(c.a[m, k]) * float(c.W.ref.view(c.I // 16, 2, 16, c.K)[n // 16, 1, n % 16, k])
    _fails(X.assert_bits_equal, (g * u2).to(torch.bfloat16), c.exp, "one up product dropped")
    _fails(X.assert_bits_equal, ((g - 1) * u).to(torch.bfloat16), c.exp, "one gate product dropped in every element")


# ------------------------------------------------------------------------------ QKV
@pytest.mark.parametrize("hd", [64, 128])
def test_qkv_rope_model_and_mutations(hd):
    nh, nkv, _ = X.QKV_GEOMS[hd]
    c = X.build_qkv(9, nh, nkv, hd, 256, seed=6 + hd, rope=True)
    assert sorted(c.pos.tolist())[0] == 0 and sorted(c.pos.tolist())[-1] == c.t_max - 1 and len(set(c.pos.tolist())) == c.M
    zp = c.a.double() @ c.W.ref.T                                          # the GEMM result in the packed column order

    def run(**kw):
        q, k, v = X.qkv_epilogue_model(c, zp, **kw)
        kflat, kc = C.guarded_cache(c.slots, nkv, c.t_max, hd)
        vflat, vc = C.guarded_cache(c.slots, nkv, c.t_max, hd)
        kc[c.slot.long(), :, c.pos.long()] = k
        vc[c.slot.long(), :, c.pos.long()] = v
        X.check_qkv(c, q, kflat, kc, vflat, vc, "model")

    run()
    _fails(run, sin_flip_from=hd // 4)
    _fails(run, partner_xor=4)
    # the upper-frequency mutation leaves every fi < hd / 4 as it was
    q0, _, _ = X.qkv_epilogue_model(c, zp)
    q1, _, _ = X.qkv_epilogue_model(c, zp, sin_flip_from=hd // 4)
    d = (C.bits(q0) != C.bits(q1)).view(c.M, nh, 2, hd // 2)
    assert not bool(d[..., :hd // 4].any()) and bool(d[..., hd // 4:].any())


def test_qkv_cache_cell_outside_the_rows_is_caught():
    nh, nkv, hd = X.QKV_GEOMS[64]
    c = X.build_qkv(5, nh, nkv, hd, 256, seed=8, rope=False)
    zp = c.a.double() @ c.W.ref.T + c.bias.double()
    q, k, v = X.qkv_epilogue_model(c, zp)
    kflat, kc = C.guarded_cache(c.slots, nkv, c.t_max, hd)
    vflat, vc = C.guarded_cache(c.slots, nkv, c.t_max, hd)
    kc[c.slot.long(), :, c.pos.long()] = k
    vc[c.slot.long(), :, c.pos.long()] = v
    X.check_qkv(c, q, kflat, kc, vflat, vc, "model")
    free = next(p for p in range(c.t_max) if p not in c.pos.tolist())
    vc[0, 0, free, 3] = 1.0
    _fails(X.check_qkv, c, q, kflat, kc, vflat, vc, "model", match="outside")


# ------------------------------------------------------------------------------ arg-max
@pytest.mark.parametrize("fp8,negative", [(False, False), (False, True), (True, False)])
def test_argmax_ties(fp8, negative):
    c = X.build_argmax(40, 4096, 256, seed=9, fp8=fp8, negative=negative)
    assert torch.equal(c.logits.argmax(-1).int(), c.expected)              # torch.argmax: the first maximal index
    X.assert_tokens(c.expected.clone(), c, "model")
    _fails(X.assert_tokens, c.largest, c, "largest tied index", match="tied columns")
    assert negative == bool((c.logits < 0).all())
    # the geometry the planted sets promise
    assert c.cols[0][0] == 0 and c.cols[0][-1] == c.V - 1
    assert any(cs[0] // 16 == cs[1] // 16 for cs in c.cols) and any(cs[1] // 16 - cs[0] // 16 == 1 for cs in c.cols)
    assert any(cs[0] % 16 == 15 and cs[1] == cs[0] + 1 for cs in c.cols)
    assert all(cs[-1] - cs[0] >= c.V // 4 for cs in c.cols)
    # a chunked launch: each half of the vocabulary with its column offset
    half = c.V // 2
    lo, hi = c.logits[:, :half], c.logits[:, half:]
    tok = torch.where(lo.max(-1).values >= hi.max(-1).values, lo.argmax(-1), hi.argmax(-1) + half).int()
    X.assert_tokens(tok, c, "chunked model")


def test_padded_head():
    c = X.build_padded_head(7, 1000, 1024, 256, seed=10)
    logits = c.a.double() @ c.W.ref.T
    assert bool((logits[:, 1000:] == logits[:, :1]).all())
    assert torch.equal((logits.float() + c.bias).argmax(-1).int(), c.expected)
    _fails(X.assert_tokens, torch.full((7,), 1023, dtype=torch.int32), c, "the largest tied index")


def test_one_ulp_checker():
    e = torch.tensor([1.0, -1.0, 256.0, 0.0], dtype=torch.bfloat16)
    up = (C.bits(e.clone()) + torch.tensor([1, 1, -1, 0], dtype=torch.int16)).view(torch.bfloat16)
    assert X.assert_within_one_ulp(e, e) == 0.0
    assert X.assert_within_one_ulp(up, e) == 0.75
    two = (C.bits(e.clone()) + torch.tensor([2, 0, 0, 0], dtype=torch.int16)).view(torch.bfloat16)
    _fails(X.assert_within_one_ulp, two, e)
    _fails(X.assert_within_one_ulp, -e[:1], e[:1])


# ------------------------------------------------------------------------------ every GPU shape
@pytest.mark.parametrize("key", X.GPU_KEYS, ids=lambda k: "-".join(str(x) for x in k))
def test_builder_conditions_hold_at_every_gpu_shape(key):
    c = X.case(key)  # the builder asserts its own conditions
    assert c.tag
    X._CACHE.clear()
