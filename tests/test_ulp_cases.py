"""The half-ulp checker and the case builders of tests/ulp_cases.py, on the CPU.

Two things are shown without a GPU. The checker ACCEPTS a float32 emulation of the correct
formulas (the norms summed strictly in sequence, the worst order): the float64 references and the
slacks derived in ulp_cases.py leave room for a correct kernel. And it REJECTS each fault that the
aggregate tolerance tests cannot see: the cancelling GELU formula, truncation, silu rounded before
the multiply, RMSNorm without eps / with H + 8 / with the weight after the rounding / with a
neighbour's sum, and a one-pass LayerNorm variance."""
import pytest
import torch

import exact_cases as X
import ulp_cases as U


def _rejects(fn, *a, **kw) -> str:
    with pytest.raises(AssertionError) as e:
        fn(*a, **kw)
    return str(e.value)


# ------------------------------------------------------------------------------ the checker itself
def test_ulp_bf16():
    v = torch.tensor([1.0, 1.5, 1.9999, 2.0, -3.0, 2.0 ** -20, 255.0, 0.75], dtype=torch.float64)
    exp = torch.tensor([2.0 ** -7, 2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -6, 2.0 ** -27, 1.0, 2.0 ** -8], dtype=torch.float64)
    assert torch.equal(U.ulp_bf16(v), exp)


def test_checker_bounds():
    one = torch.tensor([1.0], dtype=torch.bfloat16)
    up = torch.tensor([1.0 + 2.0 ** -7], dtype=torch.bfloat16)
    # a hair below the tie: 1.0 is the correct rounding; its upper neighbour is more than 1/2 ulp away
    e = torch.tensor([1.0 + 2.0 ** -8 - 2.0 ** -20], dtype=torch.float64)
    assert U.assert_half_ulp(one, e, U.SLACK_ACT, "below a tie") < 0
    _rejects(U.assert_half_ulp, up, e + 0.0, 0.0, "wrong neighbour")
    # within the slack of a tie either neighbour passes, beyond it only the nearer one
    e = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -16], dtype=torch.float64)
    U.assert_half_ulp(one, e, U.SLACK_ACT, "tie + slack / 2")
    e = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -13], dtype=torch.float64)
    _rejects(U.assert_half_ulp, one, e, U.SLACK_ACT, "tie + 2 slack")
    # the slack counts in ulps of ``scale`` where one is given
    U.assert_half_ulp(one, e, U.SLACK_ACT, "scaled", scale=torch.tensor([8.0], dtype=torch.float64))
    # below 2^-120 an absolute 2^-119; a NaN never passes; a replaced input must give +-0
    tiny = torch.tensor([2.0 ** -125], dtype=torch.float64)
    U.assert_half_ulp(torch.tensor([0.0], dtype=torch.bfloat16), tiny, 0.0, "flushed")
    U.assert_half_ulp(torch.tensor([-0.0], dtype=torch.bfloat16), tiny * 0, 0.0, "zero", zero=torch.tensor([True]))
    _rejects(U.assert_half_ulp, torch.tensor([2.0 ** -118], dtype=torch.bfloat16), tiny, 0.0, "not tiny")
    _rejects(U.assert_half_ulp, torch.tensor([float("nan")], dtype=torch.bfloat16), tiny, 1.0, "nan")
    _rejects(U.assert_half_ulp, torch.tensor([2.0 ** -126], dtype=torch.bfloat16), tiny * 0, 0.0, "non-zero",
             zero=torch.tensor([True]))
    # the top of the range: an exact value that rounds to inf must come out as inf of its sign
    inf, top = torch.tensor([float("inf")], dtype=torch.bfloat16), torch.tensor([3.3895e38], dtype=torch.bfloat16)
    big = torch.tensor([4.3e38], dtype=torch.float64)
    U.assert_half_ulp(inf, big, 0.0, "overflow")
    U.assert_half_ulp(-inf, -big, 0.0, "overflow")
    _rejects(U.assert_half_ulp, top, big, 1.0, "stayed finite")
    _rejects(U.assert_half_ulp, -inf, big, 1.0, "wrong sign")
    _rejects(U.assert_half_ulp, inf, torch.tensor([3.3e38], dtype=torch.float64), U.SLACK_ACT, "inf out of reach")
    U.assert_half_ulp(top, torch.tensor([3.39e38], dtype=torch.float64), 0.0, "largest finite")
    msg = _rejects(U.assert_half_ulp, up, torch.tensor([1.0], dtype=torch.float64), 0.0, "message",
                   inp=torch.tensor([7.0], dtype=torch.float64))
    assert "1 of 1" in msg and "input 7.0" in msg and "kernel 1.0078125" in msg and "exact 1.0" in msg


# ------------------------------------------------------------------------------ sweeps
def test_sweeps_hold_every_finite_pattern():
    for c in (U.gelu_grid(), U.swiglu_grid()):
        p = c.patterns.reshape(-1)
        fin = p[U.is_finite_pattern(p)].int() & 0xFFFF
        assert fin.unique().numel() == U.N_FINITE == 65280, c.tag
    # the operands: every normal value and both zeros, nothing a unit may flush or propagate
    g = U.gelu_grid()
    assert X.C.bits(g.a).int().unique().numel() == U.N_NORMAL_OR_ZERO
    s = U.swiglu_grid()
    assert X.C.bits(s.a[:, :U.SWIGLU_COLS].contiguous()).int().unique().numel() == U.N_NORMAL_OR_ZERO
    assert X.C.bits(s.gate.contiguous()).int().unique().numel() == U.N_NORMAL_OR_ZERO
    for a in (g.a, s.a):
        f = a.float()
        assert bool(torch.isfinite(f).all()) and not bool(((f != 0) & (f.abs() < 2.0 ** -126)).any())
    assert bool((s.a[:, U.SWIGLU_COLS:] == 1).all())
    assert int(g.zero.sum()) == 65536 - U.N_NORMAL_OR_ZERO + 2


def test_weights_reproduce_the_operand():
    """y = A W^T is the A element itself (identity), the gate its pattern and the up u_n."""
    g = U.gelu_grid()
    assert torch.equal(g.a.double() @ U.identity_rows().double().T, g.a.double())
    s = U.swiglu_grid()
    gu = (s.a.double() @ U.swiglu_rows().double().T).view(U.R_SWIGLU, U.K_ACT // 16, 2, 16)
    assert torch.equal(gu[:, :, 0].reshape(U.R_SWIGLU, U.K_ACT), s.gate.double())
    assert torch.equal(gu[:, :, 1].reshape(U.R_SWIGLU, U.K_ACT), s.up.double()[None, :].expand(U.R_SWIGLU, -1))
    w = U.swiglu_rows()
    assert bool((X.fp8_bytes(w).view(U.packing.FP8).float() == w).all())  # e4m3 holds 1, 3, -0.5, 0.15625
    r = U.repeat_rows(g.a, U.M_GEMM)
    assert r.shape[0] == U.M_GEMM and torch.equal(r[:16], g.a) and torch.equal(r[16], g.a[1]) and torch.equal(r[143], g.a[7])


def test_bias_sweep_values():
    for seed in U.BIAS_SEEDS:
        c = U.gelu_bias(seed)
        b = c.bias
        assert b.dtype == torch.float32 and b.numel() == U.K_ACT and bool((c.a == 0).all())
        tail = (b >= -10) & (b <= -2)
        small = b.abs() < 2
        assert int(tail.sum()) >= 2048 and int(small.sum()) >= 1500 and int((b > 0).sum()) > 800
        assert int(((b.view(torch.int32) & 0xFFFF) != 0).sum()) > 4000  # not bf16 values: fp32 mantissas
    assert not torch.equal(U.gelu_bias(U.BIAS_SEEDS[0]).bias, U.gelu_bias(U.BIAS_SEEDS[1]).bias)


# ------------------------------------------------------------------------------ activations
def _gelu_inputs():
    g = U.gelu_grid()
    yield g, g.a.float(), g.zero
    for seed in U.BIAS_SEEDS:
        c = U.gelu_bias(seed)
        yield c, c.bias[None, :].expand(U.R_GELU, -1), None


def test_gelu_emulation_accepted():
    for c, v, zero in _gelu_inputs():
        worst = U.assert_half_ulp(U.gelu_f32(v).to(torch.bfloat16), c.exact, U.SLACK_ACT, c.tag, inp=c.inp, zero=zero)
        print(f"{c.tag}: float32 emulation, worst excess over 1/2 ulp {worst:.3g} ulp")
        assert worst < U.SLACK_ACT / 4


def test_cancelling_gelu_rejected():
    g = U.gelu_grid()
    msg = _rejects(U.assert_half_ulp, U.gelu_f32_cancelling(g.a.float()).to(torch.bfloat16), g.exact, U.SLACK_ACT, g.tag,
                   inp=g.inp, zero=g.zero)
    print(msg)
    bad = (U.gelu_f32_cancelling(g.a.float()).to(torch.bfloat16).double() - g.exact).abs() > 1.5 * U.ulp_bf16(g.exact)
    x = g.a.float()[bad & (g.exact.abs() >= U.TINY)]
    assert x.numel() > 100 and float(x.max()) < -4 and float(x.min()) > -10
    c = U.gelu_bias(U.BIAS_SEEDS[0])
    _rejects(U.assert_half_ulp, U.gelu_f32_cancelling(c.bias[None, :].expand(U.R_GELU, -1)).to(torch.bfloat16), c.exact,
             U.SLACK_ACT, c.tag, inp=c.inp)


def test_truncation_rejected():
    g = U.gelu_grid()
    _rejects(U.assert_half_ulp, X.bf16_trunc(U.gelu_f32(g.a.float())), g.exact, U.SLACK_ACT, g.tag, inp=g.inp, zero=g.zero)
    s = U.swiglu_grid()
    _rejects(U.assert_half_ulp, X.bf16_trunc(U.silu_f32(s.gate) * s.up), s.exact, U.SLACK_ACT, s.tag, inp=s.inp, zero=s.zero)


def test_swiglu_emulation_accepted_and_early_rounding_rejected():
    s = U.swiglu_grid()
    worst = U.assert_half_ulp((U.silu_f32(s.gate) * s.up).to(torch.bfloat16), s.exact, U.SLACK_ACT, s.tag, inp=s.inp, zero=s.zero)
    print(f"{s.tag}: float32 emulation, worst excess over 1/2 ulp {worst:.3g} ulp")
    assert worst < U.SLACK_ACT / 4
    early = (U.silu_f32(s.gate).to(torch.bfloat16).float() * s.up).to(torch.bfloat16)
    _rejects(U.assert_half_ulp, early, s.exact, U.SLACK_ACT, s.tag, inp=s.inp, zero=s.zero)


# ------------------------------------------------------------------------------ RMSNorm
@pytest.mark.parametrize("H", U.RMS_GENERIC + U.RMS_REG)
def test_rmsnorm_emulation_accepted_and_faults_rejected(H):
    c = U.rms_case(H)
    for eps in U.RMS_EPS:
        for w in (c.w, None):
            exact = U.rms_exact(c.x, w, eps)
            assert bool((exact[c.zero_row] == 0).all())
            tag = f"rmsnorm H {H} eps {eps} w {w is not None}"
            worst = U.assert_half_ulp(U.rms_f32(c.x, w, eps), exact, U.SLACK_NORM, tag)
            assert worst < U.SLACK_NORM / 4, (tag, worst)
            for fault in ("no_eps", "h_plus_8", "next_row") + (("weight_after",) if w is not None else ()):
                out = U.rms_f32(c.x, w, eps, fault=fault)
                if fault == "no_eps":
                    out = torch.nan_to_num(out.float(), nan=0.0).to(torch.bfloat16)  # (the all-zero row: 0 x inf)
                _rejects(U.assert_half_ulp, out, exact, U.SLACK_NORM, f"{tag} {fault}")


@pytest.mark.parametrize("H,S", U.PARTIAL_CASES)
def test_partials_case(H, S):
    c = U.partial_case(H, S)
    hs = c.resid.double() + c.P.double().sum(0)
    assert bool(X.is_bf16(hs).all()) and torch.equal(c.h.double(), hs) and bool((c.h[c.zero_row] == 0).all())
    for w in (c.w, None):
        exact = U.rms_exact(c.h, w, 1e-5)
        U.assert_half_ulp(U.rms_f32(c.h, w, 1e-5), exact, U.SLACK_NORM, f"partials H {H} S {S}")
        _rejects(U.assert_half_ulp, U.rms_f32(c.h, w, 1e-5, fault="next_row"), exact, U.SLACK_NORM, "next_row")


# ------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("with_pos", [False, True])
@pytest.mark.parametrize("H", U.LN_WIDTHS)
def test_layernorm_emulation_accepted(H, with_pos):
    c = U.layernorm_case(H, with_pos)
    exact, scale = U.layernorm_exact(c.xr, c.g, c.b, U.LN_EPS)
    out = U.layernorm_f32(c.xr, c.g, c.b, U.LN_EPS)
    worst = U.assert_half_ulp(out, exact, U.SLACK_NORM, f"layernorm H {H}", scale=scale)
    assert worst < U.SLACK_NORM / 4
    X.assert_bits_equal(out[c.const], c.b, "constant row")
    assert torch.equal(exact[c.const], c.b.double())


def test_layernorm_one_pass_variance_rejected():
    """E[x^2] - mu^2 in float32 on the row with mean 8 and std 0.25, at the widest case (H = 1600:
    the sequential sum of squares reaches 1e5 and carries the most rounding). The slack is counted
    in ulps of |t| (1 + |mu| / sigma) + |b|, 32 times the element's own ulp on this row, so the
    fault shows where it exceeds that allowance: the worst excess of this emulation is 0.034 ulp of
    the scale at H = 1600 (rejected, the slack is 0.0156), 0.011 at H = 1024 and 0.0086 at H = 768
    (both inside the slack; elements up to 41 of their own ulps away)."""
    H = max(U.LN_WIDTHS)
    c = U.layernorm_case(H, False)
    exact, scale = U.layernorm_exact(c.xr, c.g, c.b, U.LN_EPS)
    r = slice(c.big, c.big + 1)
    out = U.layernorm_f32(c.xr[r], c.g, c.b, U.LN_EPS, one_pass=True)
    print(_rejects(U.assert_half_ulp, out, exact[r], U.SLACK_NORM, f"layernorm H {H} one-pass variance", scale=scale[r]))
