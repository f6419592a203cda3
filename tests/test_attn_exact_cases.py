"""CPU side of the per-element attention contract (tests/attn_exact_cases.py): the builders'
stated conditions, float32 emulations of both kernel classes (fp32 P with q pre-scaled; bf16 P
with the product scaled afterwards) with 1, 4 and 16 splits that must pass every case, and fault
models that must fail theirs."""
import functools

import pytest
import torch

import attn_exact_cases as E
import contract_cases as C

SHAPES = [(8, 2, 64), (8, 8, 128)]
CLASSES = [E.FP32_P, E.BF16_P]
ids = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)  # noqa: E731


def _a_lens(hd, nsplit):
    return tuple(C.membership_lengths(hd, C.split_edge_lengths(hd, nsplit) if nsplit > 1 else ()))


@functools.lru_cache(maxsize=2)
def _a_case(shape, lens):
    case, q = E.build_select_case(*shape, list(lens))
    return case, q, E.select_expected(case, case.slot, case.lens_t)


def _b_lens(hd):
    return tuple(E.B_LENS + [C.t_max_for(hd)])


@functools.lru_cache(maxsize=2)
def _b_case(shape, variant):
    case, q = E.build_b_case(variant, *shape, list(_b_lens(shape[2])))
    return case, q, E.interval_reference(q, case)


def _check_b(out, shape, variant, cls):
    case, q, (ref, A, S, T) = _b_case(shape, variant)
    return E.check_interval(out, ref, A, E.slack_c(S, T, shape[2], cls), shape[0], shape[2], f"{shape} {variant} {cls}")


# ------------------------------------------------------------------------------ builders
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_select_case_conditions(shape):
    nh, nkv, hd = shape
    case, q, (exp, cnt) = _a_case(shape, _a_lens(hd, 4))
    t_max = case.t_max
    margin = E.select_margin(hd)
    assert margin >= (32 if hd == 128 else 46) and t_max * 2.0 ** -margin * 32 < 2.0 ** -10
    D = E.head_dims(nh, hd)
    assert bool(D[:, 0].all()) and bool((D.sum(1) == hd // 8 + (torch.arange(nh) % 8 != 0)).all())
    assert len({tuple(r.tolist()) for r in D[:min(nh, 8)]}) == min(nh, 8)   # the heads of a group differ
    sig = E.sigma(hd)
    assert 0 < int((sig < 0).sum()) < hd
    # both arithmetic orders give the selected keys exactly 256 scale_log2 and every other key exactly 0
    sl2 = E.scale_log2_f32(hd)
    row = max(range(case.rows), key=lambda r: case.lens[r])
    k = case.K[int(case.slot[row]), 0, :case.lens[row]].float()                # [T, hd]
    qh = q[0].float().view(nh, hd)
    pre = ((qh * sl2)[:, None, :] * k[None]).sum(-1)
    post = (qh[:, None, :] * k[None]).sum(-1) * sl2
    sel = D[:, torch.arange(case.lens[row]) % hd]                              # [nh, T]
    want = torch.where(sel, 256.0 * sl2, torch.zeros(()))
    assert torch.equal(pre, want) and torch.equal(post, want)
    assert float(256.0 * sl2) == margin
    # expected vectors: the direct float64 sum over the selected keys of the cache itself
    assert bool((cnt >= 1).all()) and int(cnt.max()) <= t_max // 8 + t_max // hd + 2
    g = nh // nkv
    for r in (0, row, case.rows // 2):
        T, s = case.lens[r], int(case.slot[r])
        selr = D[:, torch.arange(T) % hd]
        v = case.V[s, :, :T].double().repeat_interleave(g, 0)                  # [nh, T, hd]
        assert torch.equal((v * selr[:, :, None]).sum(1).long(), exp[r]) and torch.equal(selr.sum(1), cnt[r])
    # poison beyond every length, as in the membership cases
    for r, T in enumerate(case.lens):
        s = int(case.slot[r])
        assert bool(torch.isfinite(case.K[s, :, :T].float()).all()) and bool(C.is_sentinel(case.K[s, :, T:]).all())
        assert bool(C.is_sentinel(case.V[s, :, T:]).all())


def test_rounding_helpers():
    x = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -40, -3.0 - 2.0 ** -7,
                      0.0, 2.0 - 2.0 ** -9, 1e-3], dtype=torch.float64)
    want = torch.tensor([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -3.0, 0.0, 2.0, float(torch.tensor(1e-3).bfloat16())],
                        dtype=torch.float64)
    assert torch.equal(E.rne_bf16(x), want)
    # (a cast through fp32 rounds 1 + 2^-8 + 2^-40 to the tie first and then to even: 1.0)
    assert float(x[3].float().bfloat16()) == 1.0
    out = torch.tensor([1.0, 1.0, 1.0078125, -2.0, 0.0], dtype=torch.bfloat16)
    ref = torch.tensor([1.0 + 2.0 ** -8, 1.0 - 2.0 ** -9, 1.0, -2.0 - 2.0 ** -7, 0.0], dtype=torch.float64)
    need = E.needed_slack(out, ref, torch.ones(5, dtype=torch.float64))
    assert need.tolist() == [0.0, 0.0, 2.0 ** -8, 0.0, 0.0]
    # the interval rule: exactly the roundings of [ref - s, ref + s], NaN and a missed tie-side fail
    ref = torch.tensor([[1.0 + 2.0 ** -8, 4.0]], dtype=torch.float64)
    A, c = torch.ones(1, 2, dtype=torch.float64), torch.full((1, 1), 2.0 ** -20, dtype=torch.float64)
    for good in ([1.0, 4.0], [1.0078125, 4.0]):
        E.check_interval(torch.tensor([good], dtype=torch.bfloat16), ref, A, c, 1, 2)
    for bad in ([0.9921875, 4.0], [1.0, 4.03125], [float("nan"), 4.0]):
        with pytest.raises(AssertionError):
            E.check_interval(torch.tensor([bad], dtype=torch.bfloat16), ref, A, c, 1, 2)


def test_slack_values():
    """The derived constants at the sizes the docstring quotes; the bf16-P class adds 2^-8 except at T = 1."""
    S = torch.tensor([[12.0], [40.0], [12.0]], dtype=torch.float64)
    T = torch.tensor([1100, 1100, 1])
    c = E.slack_c(S, T, 128, E.FP32_P)[:, 0].tolist()
    assert 6.5e-5 < c[0] < 7.0e-5 and 1.2e-4 < c[1] < 1.3e-4 and c[2] < 3.7e-5
    cm = E.slack_c(S, T, 128, E.BF16_P)[:, 0].tolist()
    assert 2.0 ** -8 < cm[0] < 2.0 ** -8 + 1e-3 and cm[2] < 2.0e-4


# ------------------------------------------------------------------------------ emulations pass
@pytest.mark.parametrize("nsplit", [1, 4, 16])
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_emulation_passes_case_a(shape, cls, nsplit):
    case, q, (exp, cnt) = _a_case(shape, _a_lens(shape[2], nsplit))
    resid = E.check_select(E.emulate(q, case, cls, nsplit), exp, cnt, case.lens_t, f"{shape} {cls} nsplit {nsplit}")
    assert resid < 0.5
    print(f"case A emulation {shape} {cls} nsplit {nsplit}: {case.rows} rows, worst decode residual {resid:.3f}")


@pytest.mark.parametrize("variant", E.B_VARIANTS)
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_emulation_passes_case_b(shape, cls, variant):
    case, q, _ = _b_case(shape, variant)
    for nsplit in (1, 4, 16):
        worst = _check_b(E.emulate(q, case, cls, nsplit), shape, variant, cls)
        print(f"case B emulation {shape} {cls} {variant} nsplit {nsplit}: worst needed slack {worst:.3e} A")


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_emulation_passes_the_ties(shape, cls):
    case, q, exp = E.build_tie_case(*shape)
    for nsplit in (1, 4):
        E.check_ties(E.emulate(q, case, cls, nsplit), exp, f"{shape} {cls}")


def test_length_one_is_bitwise():
    """At len 1 the interval is the single value V[0], for both classes."""
    shape = SHAPES[0]
    case, q, (ref, A, S, T) = _b_case(shape, "gauss")
    assert case.lens[0] == 1
    for cls in CLASSES:
        c = E.slack_c(S, T, shape[2], cls)
        v0 = case.V[int(case.slot[0]), :, 0].repeat_interleave(shape[0] // shape[1], 0).reshape(1, -1)
        E.check_interval(v0, ref[:1], A[:1], c[:1], shape[0], shape[2])
        off = (v0.view(torch.int16) + 1).view(torch.bfloat16)                  # one ulp away
        with pytest.raises(AssertionError):
            E.check_interval(off, ref[:1], A[:1], c[:1], shape[0], shape[2])


# ------------------------------------------------------------------------------ faults fail
def _fails_b(shape, variant, cls, fault, nsplit):
    case, q, _ = _b_case(shape, variant)
    with pytest.raises(AssertionError, match="outside the interval"):
        _check_b(E.emulate(q, case, cls, nsplit, fault), shape, variant, cls)


@pytest.mark.parametrize("fault,nsplit", [("bf16_p", 1), ("bf16_qscale", 1), ("bf16_partials", 4), ("trunc", 1),
                                          ("ln_merge", 4)])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_fp32_bound_rejects_the_rounding_faults(shape, fault, nsplit):
    for variant in ("gauss", "peaked+4"):
        _fails_b(shape, variant, E.FP32_P, fault, nsplit)


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_bf16_p_bound_rejects_the_merge_fault(shape):
    _fails_b(shape, "peaked", E.BF16_P, "ln_merge", 4)


@pytest.mark.parametrize("fault", ["trunc", "half_up"])
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_ties_reject_the_conversions(shape, cls, fault):
    case, q, exp = E.build_tie_case(*shape)
    with pytest.raises(AssertionError, match="not rounded to even"):
        E.check_ties(E.emulate(q, case, cls, 1, fault), exp)


@pytest.mark.parametrize("fault", ["drop_dim", "swap_heads"])
@pytest.mark.parametrize("cls", CLASSES)
def test_case_a_rejects_the_dot_product_faults(cls, fault):
    shape = (8, 2, 64)                                                         # a GQA group of 4
    case, q, (exp, cnt) = _a_case(shape, _a_lens(64, 4))
    with pytest.raises(AssertionError, match="selected keys give"):
        E.check_select(E.emulate(q, case, cls, 4, fault), exp, cnt, case.lens_t)


def test_every_fault_is_covered():
    covered = {"bf16_p", "bf16_qscale", "bf16_partials", "trunc", "ln_merge", "half_up", "drop_dim", "swap_heads"}
    assert covered == set(E.FAULTS) and set(E.LOOSE_FAULTS) == {"trunc", "half_up", "ln_merge", "drop_dim", "swap_heads"}
