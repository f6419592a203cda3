"""Builders, float64 references, checkers and float32 emulations for the per-element contract of
the attention kernels (tests/test_attn_exact_cases.py on the CPU, tests/test_attn_exact_gpu.py on
the GPU). contract_cases.py fixes WHICH keys a row attends (q = 0) and an aggregate
``rel_err < 1e-2``; neither sees the q . k dot product beyond dim 0, the head indexing inside a
GQA group, or a rounding that is a hundred times coarser than the kernel's own. Three cases:

**Case A, selected keys (exact).** ``sigma(d) = +-1`` is a fixed sign pattern over the dims.
``K[key] = 16 sigma(key % hd) e_(key % hd)`` and query head r (global index) is
``q_r[d] = 16 sigma(d)`` for ``d in D_r = {d : d % 8 == r % 8} + {0}``, 0 elsewhere. A key with
``key % hd in D_r`` scores exactly ``256 scale log2(e)`` (one non-zero product, power-of-two
factors: exact whether q is scaled first or the product afterwards), every other key exactly 0:
32 (hd 128) or 46 (hd 64) binades lower, so all unselected keys together weigh less than
``t_max 2^-32 32 < 2^-10`` of one V unit. V is contract_cases' power-of-two pattern, NaN beyond
every length. ``round(out n_r)`` with ``n_r`` = head r's selected keys below len must be the
integer vector of exactly those keys. One q dim dropped, a wrong partner lane, a wrong sign (the
key's weight drops by 2^-65), two heads of a group swapped or a padding column read as a head
moves a dim by at least 1.

**Case B, rounding interval (per element).** q (distinct per head) and K Gaussian bf16, a peaked
variant with 3 q, V N(0, 1) (cancelling) or N(0, 1) + 4, and contract_cases' score ramps. With
``ref = sum p_i v_i`` and ``A = sum p_i |v_i|`` in float64 from the same bf16 inputs, every
element must satisfy ``bf16(ref - s) <= out <= bf16(ref + s)``, both ends rounded to nearest
even: ``out`` is the correct rounding of some value within ``s = c A`` of the exact one. NaN
fails. At len 1 the interval is the single value V[0].

**Ties.** The interval admits both neighbours of a tie by construction, and Case A's quotients
never tie (an odd 9-bit significand would have to divide a sum <= 126), so neither sees an
output conversion that rounds ties away from zero. ``build_tie_case``: q = 0 and 2 or 4 keys whose
V values alternate between x and y = ulp(x) / 2 or 3 ulp(x) / 2: every weight is exactly 1, the
sum and the quotient are exact in fp32, the quotient is a tie, and the output must be the even
neighbour bit for bit.

The slack ``c`` is derived from the operations of a correct kernel, never from a measurement.
u = 2^-24 (fp32 unit roundoff), S = max over a row's keys of ``sum_j |q_j k_j| scale log2(e)``
(the magnitude that the score's rounding errors scale with), T = the row's keys. A relative
perturbation e_i of the weights changes ``sum p_i v_i / sum p_i`` by at most ``max |e_i| (A +
|ref|) <= 2 max |e_i| A``; rounding errors of the two accumulations count once for l and once
for o, the same factor 2.

fp32-P kernels (attn_split_body in csrc/kernels/attn_body.h: attn_split_kernel,
attn_small_kernel, attn_oproj_kernel; attn_kv8_body in csrc/cache/kv8.hip, whose per-key scales
are powers of two and cost nothing):

* exponent of a weight, in units of u, times ln 2 for the weight itself:
  - the score: scale_log2 = fl(fl(hd^-1/2) fl(log2 e)) 3, ``q_j scale_log2`` 1, the product 1,
    8 sequential adds in a lane and log2(LPK) <= 4 DPP levels 12: 17 S;
  - the subtractions ``s - m``, ``m_old - m_new`` along the key's chain of rescalings (they
    telescope to at most 2 S) and ``lse - max lse`` (2 S + log2 T <= 2 S + 11): 6 S + 11;
  - ``lse = m + log2f(l)``: the add at |lse| <= S + 11, log2f within 2 ulp of a value <= 11:
    S + 11 + 44;
  together ln 2 (24 S + 66);
* one ulp = 2 u of v_exp_f32 for the weight itself, for every rescaling of its accumulator (at
  most one per iteration, n_it <= n_seq), three key-group merges, the wave merge and the split
  merge: 2 (n_seq + 6);
* accumulation, per accumulator: n_seq sequential adds (a lane takes every KPI-th key, KPI >= 16:
  n_seq = ceil(T / 16)), the product p v 1, n_it <= n_seq rescaling multiplies, three
  ``l a + l' b`` merges 9, the wave merge over <= 8 waves 9, the divide 1, the split merge (16
  adds, product, divide) 18: 2 n_seq + 38.

``c32(S, T) = 2 u (ln 2 ((depth + 12) S + 66) + 4 n_seq + 50)`` with depth = 12: 6.8e-5 =
2^-13.9 at S = 12 (Gaussian q, k at hd 128) and T = 1100, 1.2e-4 at S = 40 (the ramps, the
peaked variant); an upper bound, since the errors do not all align.

bf16-P kernels (flash_prefill_kernel, gqa_decode_kernel in csrc/kernels/attn_prefill.hip):
``c = 2^-8 + c32`` - each weight enters the PV product rounded once to bf16 (unit roundoff
2^-8) while l keeps the unrounded sum, so the factor is 1, not 2 - and in c32 the score is one
fp32 multiply after an MFMA sum whose order is not documented: depth = hd (a sequential sum),
n_seq = T (the PV MFMAs likewise).

Everything is plain torch, drawn on the CPU from seeded generators and moved, and runs on any
device.
"""
from __future__ import annotations

import math
from typing import Optional

import torch

import contract_cases as C
import exact_cases as X
from ulp_cases import ulp_bf16

LOG2E_F32 = 1.4426950408889634
U32 = 2.0 ** -24
U_BF16 = 2.0 ** -8
SEL_A = SEL_B = 16.0
FP32_P, BF16_P = "fp32", "mfma"       # the two kernel classes
B_LENS = [1, 2, 3, 17, 64, 65, 129, 256, 257, 513]  # + t_max
B_VARIANTS = ("gauss", "gauss+4", "peaked", "peaked+4", "ramp-up", "ramp-down")


def scale_log2_f32(hd: int) -> torch.Tensor:
    """The kernels' fp32 scale: float(hd ** -0.5) * 1.4426950408889634f, rounded to fp32."""
    return torch.tensor(hd ** -0.5, dtype=torch.float32) * torch.tensor(LOG2E_F32, dtype=torch.float32)


# ------------------------------------------------------------------------------ slack
def c32(S: torch.Tensor, T: torch.Tensor, hd: int, cls: str = FP32_P) -> torch.Tensor:
    """The derived slack in units of A (module docstring); ``S`` [n, nh], ``T`` [n] -> [n, nh]."""
    T = T.double().to(S.device)[:, None]
    depth, n_seq = (12.0, torch.ceil(T / 16)) if cls == FP32_P else (float(hd), T)
    return 2 * U32 * (math.log(2.0) * ((depth + 12) * S.double() + 66) + 4 * n_seq + 50)


def slack_c(S: torch.Tensor, T: torch.Tensor, hd: int, cls: str) -> torch.Tensor:
    """c32, plus 2^-8 for the bf16-P class - except at T = 1, where the lone weight is
    exp2(0) = 1, a bf16 value: nothing is rounded and the rule stays out == V[0] bit for bit."""
    c = c32(S, T, hd, cls)
    if cls == FP32_P:
        return c
    return c + torch.where(T.to(S.device)[:, None] > 1, U_BF16, 0.0)


# ------------------------------------------------------------------------------ bf16 rounding of float64
def rne_bf16(x: torch.Tensor) -> torch.Tensor:
    """float64 -> the nearest bf16 value (ties to even), as float64, in ONE rounding (a cast
    through fp32 rounds twice). Normal range only."""
    m, e = torch.frexp(x.double())                       # x = m 2^e, |m| in [0.5, 1)
    return torch.ldexp(torch.round(torch.ldexp(m, torch.full_like(e, 8))), e - 8)  # torch.round: half to even


def _rounding_cell(out: torch.Tensor):
    """(lo, hi) float64: the reals that round to the bf16 value ``out`` (closed; ties ignored)."""
    o = out.double()
    a = o.abs()
    m, _ = torch.frexp(a)
    up = 0.5 * ulp_bf16(a)
    down = torch.where(m == 0.5, 0.5 * up, up)           # a power of two: the binade below is finer
    up, down = torch.where(a == 0, torch.zeros_like(a), up), torch.where(a == 0, torch.zeros_like(a), down)
    lo = torch.where(o >= 0, o - down, o - up)
    hi = torch.where(o >= 0, o + up, o + down)
    return lo, hi


def needed_slack(out: torch.Tensor, ref: torch.Tensor, A: torch.Tensor) -> torch.Tensor:
    """Per element the smallest s / A for which ``out`` is a rounding of a value within s of ref."""
    lo, hi = _rounding_cell(out)
    need = torch.clamp(torch.maximum(lo - ref, ref - hi), min=0.0)
    need = torch.where(need > 0, need / A, need)         # (A = 0 and need > 0: inf)
    return torch.nan_to_num(need, nan=float("inf"))


def check_interval(out: torch.Tensor, ref: torch.Tensor, A: torch.Tensor, c: torch.Tensor, nh: int, hd: int,
                   what: str = "", T: Optional[torch.Tensor] = None) -> float:
    """Every element: bf16(ref - c A) <= out <= bf16(ref + c A) (``c`` [n, nh]). Returns the worst
    needed slack in units of A."""
    assert out.dtype == torch.bfloat16, out.dtype
    n = ref.shape[0]
    # (on the CPU, as ulp_cases.assert_half_ulp: frexp / ldexp / round are exact there)
    o = out[:, :nh * hd].detach().cpu().double().reshape(n, nh, hd)
    ref, A = ref.detach().cpu().reshape(n, nh, hd), A.detach().cpu().reshape(n, nh, hd)
    s = c.detach().cpu().double()[:, :, None] * A
    ok = (o >= rne_bf16(ref - s)) & (o <= rne_bf16(ref + s))          # (NaN fails)
    need = needed_slack(o, ref, A)
    worst = float(need.max()) if need.numel() else 0.0
    if not bool(ok.all()):
        bad = ~ok
        flat = torch.where(bad, need, torch.full_like(need, -1.0)).reshape(-1)
        r, h, d = (int(i) for i in torch.unravel_index(flat.argmax(), bad.shape))
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {bad.numel()} element(s) outside the interval; row {r} head {h} dim {d}: "
            f"kernel {float(o[r, h, d])!r} exact {float(ref[r, h, d])!r} A {float(A[r, h, d])!r} needs "
            f"{float(need[r, h, d]):.3e} A, allowed {float(c[r, h]):.3e} A (T {int(T[r]) if T is not None else '?'})")
    return worst


# ------------------------------------------------------------------------------ case A
def sigma(hd: int, device="cpu") -> torch.Tensor:
    d = torch.arange(hd, device=device)
    return torch.where((d * 5 + d // 7) % 3 == 0, -1.0, 1.0)


def head_dims(nh: int, hd: int, device="cpu") -> torch.Tensor:
    """bool [nh, hd]: D_r."""
    d, r = torch.arange(hd, device=device)[None, :], torch.arange(nh, device=device)[:, None]
    return (d % 8 == r % 8) | (d == 0)


def select_q(rows: int, nh: int, hd: int, device="cpu") -> torch.Tensor:
    """bf16 [rows, nh * hd]: q_r[d] = 16 sigma(d) on D_r, the same for every row."""
    q = torch.where(head_dims(nh, hd, device), SEL_A * sigma(hd, device)[None, :], 0.0).to(torch.bfloat16)
    return q.reshape(1, nh * hd).expand(rows, -1).contiguous()


def select_margin(hd: int) -> float:
    """A selected key's score in the exp2 domain = binades between selected and unselected keys."""
    return SEL_A * SEL_B * float(scale_log2_f32(hd))


def build_select_case(nh: int, nkv: int, hd: int, lens: list, device="cpu"):
    """(case, q): contract_cases' membership cache (V pattern, NaN beyond every length) with
    K[key] = 16 sigma(key % hd) e_(key % hd) on the valid cells."""
    case = C.build_membership_case(nh, nkv, hd, lens, device)
    t_max = case.t_max
    assert t_max * 2.0 ** -select_margin(hd) * 32 < 2.0 ** -10, (hd, select_margin(hd))
    key, d = torch.arange(t_max, device=device), torch.arange(hd, device=device)
    kpat = torch.where(d[None, :] == (key % hd)[:, None], SEL_B * sigma(hd, device)[None, :], 0.0).to(torch.bfloat16)
    valid = key[None, :] < case.lens_t[:, None]
    nan = C.sentinel_fill(torch.empty((), dtype=torch.bfloat16, device=device))
    case.K[case.slot.long()] = torch.where(valid[:, None, :, None], kpat[None, None], nan)
    return case, select_q(case.rows, nh, hd, device)


def select_expected(case: C.AttnCase, slots: torch.Tensor, lens: torch.Tensor):
    """(exp int64 [n, nh, hd], cnt int64 [n, nh]): per head the integer per-dim sums and the number
    of its selected keys (key % hd in D_r) below lens[i] in slot slots[i]."""
    dev, nh, hd, t_max, g = case.V.device, case.nh, case.hd, case.t_max, case.nh // case.nkv
    key, d = torch.arange(t_max, device=dev), torch.arange(hd, device=dev)
    cls = torch.arange(8, device=dev)[:, None]
    sel = ((key % hd)[None, :] % 8 == cls) | ((key % hd)[None, :] == 0)      # [8, t_max]: D_r depends on r % 8
    onehot = torch.zeros(8, t_max + 1, hd, dtype=torch.int64, device=dev)
    onehot[:, key + 1, key % hd] = C.v_weight(key, hd)[None, :] * sel
    lens, slots = lens.long().to(dev), slots.long().to(dev)
    head = torch.arange(nh, device=dev)
    base = onehot.cumsum(1)[:, lens][head % 8].permute(1, 0, 2)              # [n, nh, hd]
    cnt = torch.cat([torch.zeros(8, 1, dtype=torch.int64, device=dev), sel.long().cumsum(1)], 1)[:, lens][head % 8].t()
    sh = case.shift[slots][:, head // g]                                     # [n, nh]
    idx = (d[None, None, :] - sh[:, :, None]) % hd
    assert bool((cnt >= 1).all())                                            # key 0 is selected for every head
    return base.gather(2, idx), cnt


def check_select(out: torch.Tensor, exp: torch.Tensor, cnt: torch.Tensor, lens: torch.Tensor, what: str = "") -> float:
    """``round(out n_r)`` is exactly ``exp`` for every (row, head); returns the worst decode residual."""
    n, nh, hd = exp.shape
    o = out[:, :nh * hd]
    assert bool(torch.isfinite(o.float()).all()), f"{what}: non-finite output (poisoned cache cells leaked in)"
    v = o.double().reshape(n, nh, hd) * cnt.to(o.device).double()[:, :, None]
    ints = v.round()
    bad = (ints.long() != exp.to(o.device)).any(-1)
    if bool(bad.any()):
        r, h = bad.nonzero()[0].tolist()
        dim = int((ints[r, h].long() != exp[r, h].to(o.device)).nonzero()[0])
        raise AssertionError(
            f"{what}: row {r} (len {int(lens[r])}) head {h}: dim {dim} decodes to {int(ints[r, h, dim])}, the head's "
            f"{int(cnt[r, h])} selected keys give {int(exp[r, h, dim])}; {int(bad.sum())} (row, head) pairs differ")
    return float((v - ints).abs().max())


# ------------------------------------------------------------------------------ ties
TIE_LENS = [2, 4, 2, 4, 2, 4]


def build_tie_case(nh: int, nkv: int, hd: int, device="cpu"):
    """(case, q, expected bf16 [rows, nh * hd]): q = 0 and 2 or 4 keys. Even keys hold
    x_d = (8 + (d + 5 kvh + row) % 8) / 8 * 2^(d % 3) (4-bit significands), odd keys
    y_d = c_d * 2^(d % 3 - 8), c_d = 1 or 3: the mean (x + y) / 2 is exact in fp32 in every
    summation order and lies half way between two bf16 values - below it the even one for c = 1
    (the half-up conversion returns the other), above it for c = 3 (truncation returns the
    other). The vectors of a key share a binade, so the e4m3 cache holds them exactly too."""
    case, slot_t, lens_t, key, valid = C._case_common(nh, nkv, hd, TIE_LENS, device)
    rows, t_max = case.rows, case.t_max
    d = torch.arange(hd, device=device)
    j = (d[None, None, :] + 5 * torch.arange(nkv, device=device)[None, :, None]
         + torch.arange(rows, device=device)[:, None, None]) % 8               # [rows, nkv, hd]
    sc = 2.0 ** (d % 3).double()
    x = (8 + j).double() / 8 * sc
    y = torch.where((d // 3) % 2 == 0, 1.0, 3.0).double() * sc * 2.0 ** -8
    odd = (key % 2 == 1)[None, None, :, None]
    vv = torch.where(odd, y.expand(rows, nkv, hd)[:, :, None, :], x[:, :, None, :]).to(torch.bfloat16)
    assert bool((vv[:, :, :2].double().sum(2) == x + y).all())               # exact in bf16
    nan = C.sentinel_fill(torch.empty((), dtype=torch.bfloat16, device=device))
    kpat = (((key[:, None] * 5 + d[None, :] * 3) % 17 - 8).float() / 8).to(torch.bfloat16)
    case.V[slot_t] = torch.where(valid[:, None, :, None], vv, nan)
    case.K[slot_t] = torch.where(valid[:, None, :, None], kpat[None, None], nan)
    mean = (x + y) / 2
    exp = X.bf16_rne(mean)
    assert bool(X.is_tie(mean).all()) and bool((X.bf16_half_up(mean) != exp).any()) and bool((X.bf16_trunc(mean) != exp).any())
    exp = exp.repeat_interleave(nh // nkv, 1).reshape(rows, nh * hd)
    return case, torch.zeros(rows, nh * hd, dtype=torch.bfloat16, device=device), exp


def check_ties(out: torch.Tensor, exp: torch.Tensor, what: str = "") -> None:
    o = out[:, :exp.shape[1]]
    bad = C.bits(o.contiguous()) != C.bits(exp.to(o.device).contiguous())
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} tie(s) not rounded to even, first at {bad.nonzero()[0].tolist()}: "
                                 f"kernel {float(o[bad][0])!r} expected {float(exp.to(o.device)[bad][0])!r}")


# ------------------------------------------------------------------------------ case B
def gauss_q(rows: int, nh: int, hd: int, peaked: bool, seed: int, device="cpu") -> torch.Tensor:
    """bf16 [rows, nh * hd], distinct per row and head; ``peaked``: times 3."""
    q = torch.randn(rows, nh * hd, generator=X.gen(seed + 17)) * (3.0 if peaked else 1.0)
    return q.to(torch.bfloat16).to(device)


def build_gauss_case(nh: int, nkv: int, hd: int, lens: list, device="cpu", v_offset: float = 0.0, seed: int = 0):
    """K N(0, 1), V N(0, 1) + v_offset on the valid cells, NaN beyond every length."""
    case, slot_t, lens_t, key, valid = C._case_common(nh, nkv, hd, lens, device)
    g = X.gen(seed)
    nan = C.sentinel_fill(torch.empty((), dtype=torch.bfloat16, device=device))
    shape = (case.rows, nkv, case.t_max, hd)
    kk = torch.randn(shape, generator=g).to(torch.bfloat16).to(device)
    vv = (torch.randn(shape, generator=g) + v_offset).to(torch.bfloat16).to(device)
    case.K[slot_t] = torch.where(valid[:, None, :, None], kk, nan)
    case.V[slot_t] = torch.where(valid[:, None, :, None], vv, nan)
    return case


def build_b_case(variant: str, nh: int, nkv: int, hd: int, lens: list, device="cpu"):
    """(case, q [case.rows, nh * hd]) of one of B_VARIANTS."""
    seed = B_VARIANTS.index(variant) * 1000 + nh * 7 + hd
    if variant.startswith("ramp"):
        return C.build_score_case(nh, nkv, hd, lens, device, rising=variant == "ramp-up", seed=seed)
    case = build_gauss_case(nh, nkv, hd, lens, device, 4.0 if variant.endswith("+4") else 0.0, seed)
    return case, gauss_q(case.rows, nh, hd, variant.startswith("peaked"), seed, device)


def b_query(variant: str, rows: int, nh: int, hd: int, device="cpu") -> torch.Tensor:
    """Queries for ``rows`` rows that are not the case's own (prefill runs): the ramps' c e_0, or
    Gaussian rows."""
    if variant.startswith("ramp"):
        q = torch.zeros(rows, nh, hd, dtype=torch.bfloat16, device=device)
        q[:, :, 0] = 80.0 / (8.0 * hd ** -0.5 * LOG2E_F32)
        return q.view(rows, nh * hd)
    return gauss_q(rows, nh, hd, variant.startswith("peaked"), B_VARIANTS.index(variant) + 5 * rows, device)


def interval_reference(q: torch.Tensor, case: C.AttnCase, lens=None, rows=None):
    """(ref, A float64 [n, nh * hd], S float64 [n, nh], T int64 [n]): fp64 softmax attention of
    query row i over keys [0, len) of case row rows[i]'s slot, ``A = sum p |v|`` and
    ``S = max_key sum_j |q_j k_j| scale log2(e)``."""
    nh, nkv, hd = case.nh, case.nkv, case.hd
    g = nh // nkv
    rows = list(range(case.rows)) if rows is None else list(rows)
    n = len(rows)
    ref = torch.zeros(n, nh, hd, dtype=torch.float64, device=q.device)
    A, S = torch.zeros_like(ref), torch.zeros(n, nh, dtype=torch.float64, device=q.device)
    Ts = [int(case.lens[r] if lens is None else lens[i]) for i, r in enumerate(rows)]
    for i, r in enumerate(rows):
        T, s = Ts[i], int(case.slot[r])
        k = case.K[s, :, :T].double().repeat_interleave(g, 0)                # [nh, T, hd]
        v = case.V[s, :, :T].double().repeat_interleave(g, 0)
        qi = q[i, :nh * hd].double().view(nh, hd)
        p = torch.softmax(torch.einsum("hd,htd->ht", qi, k) * hd ** -0.5, -1)
        ref[i] = torch.einsum("ht,htd->hd", p, v)
        A[i] = torch.einsum("ht,htd->hd", p, v.abs())
        S[i] = torch.einsum("hd,htd->ht", qi.abs(), k.abs()).amax(1) * (hd ** -0.5 * LOG2E_F32)
    return ref.reshape(n, nh * hd), A.reshape(n, nh * hd), S, torch.tensor(Ts, dtype=torch.int64)


# ------------------------------------------------------------------------------ float32 emulations
# What a correct (or a deliberately faulty) kernel of either class computes, in float32 on the CPU:
# q pre-scaled and P in fp32 (FP32_P) or the product scaled afterwards and P rounded to bf16 for the
# PV product only (BF16_P); an online softmax in 64-key blocks inside every split chunk, the splits
# merged through lse = m + log2(l); one conversion of the result.
FAULTS = ("bf16_p", "bf16_qscale", "bf16_partials", "trunc", "half_up", "ln_merge", "drop_dim", "swap_heads")
LOOSE_FAULTS = FAULTS[3:]     # what the bf16-P bound has to reject as well


def _bf16_round(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16).float()


def emulate(q: torch.Tensor, case: C.AttnCase, cls: str = FP32_P, nsplit: int = 1, fault: Optional[str] = None,
            lens=None, rows=None, block: int = 64) -> torch.Tensor:
    """bf16 [n, nh * hd]. ``fault``: one of FAULTS (bf16_partials and ln_merge show only where a
    row has more than one non-empty split; swap_heads needs a GQA group of at least 2)."""
    assert fault is None or fault in FAULTS, fault
    nh, nkv, hd = case.nh, case.nkv, case.hd
    g = nh // nkv
    rows = list(range(case.rows)) if rows is None else list(rows)
    sl2 = scale_log2_f32(hd)
    out = torch.zeros(len(rows), nh, hd, dtype=torch.float32)
    for i, r in enumerate(rows):
        T, s = int(case.lens[r] if lens is None else lens[i]), int(case.slot[r])
        k = case.K[s, :, :T].cpu().float().repeat_interleave(g, 0)           # [nh, T, hd]
        v = case.V[s, :, :T].cpu().float().repeat_interleave(g, 0)
        qi = q[i, :nh * hd].cpu().float().view(nh, hd).clone()
        if fault == "swap_heads":
            assert g >= 2
            qi[[0, 1]] = qi[[1, 0]]
        if fault == "drop_dim":
            qi[torch.arange(nh), torch.arange(nh) % 8 + 8] = 0.0             # a dim of D_r
        if cls == FP32_P:
            qs = qi * sl2
            if fault == "bf16_qscale":
                qs = _bf16_round(qs)
            sc = (qs[:, None, :] * k).sum(-1)                                # [nh, T]
        else:
            sc = (qi[:, None, :] * k).sum(-1) * sl2
        chunk = C.split_chunk(T, nsplit, hd)
        parts, lses = [], []
        for k0 in range(0, T, chunk):
            k1 = min(T, k0 + chunk)
            m = torch.full((nh,), -1e30)
            l, o = torch.zeros(nh), torch.zeros(nh, hd)
            for b0 in range(k0, k1, block):
                sb = sc[:, b0:min(k1, b0 + block)]
                mn = torch.maximum(m, sb.amax(1))
                alpha = torch.exp2(m - mn)
                p = torch.exp2(sb - mn[:, None])
                l = l * alpha + p.sum(1)
                pv = _bf16_round(p) if (cls == BF16_P or fault == "bf16_p") else p
                o = o * alpha[:, None] + torch.einsum("ht,htd->hd", pv, v[:, b0:min(k1, b0 + block)])
                m = mn
            part = o / l[:, None]
            parts.append(_bf16_round(part) if fault == "bf16_partials" else part)
            lses.append(m + (torch.log(l) if fault == "ln_merge" else torch.log2(l)))
        if len(parts) == 1:                                                  # a lone active split writes the output
            out[i] = parts[0]
        else:
            lse = torch.stack(lses)                                          # [splits, nh]
            w = torch.exp2(lse - lse.amax(0))
            out[i] = (w[:, :, None] * torch.stack(parts)).sum(0) / w.sum(0)[:, None]
    out = out.reshape(len(rows), nh * hd)
    if fault == "trunc":
        return X.bf16_trunc(out)
    if fault == "half_up":
        return X.bf16_half_up(out)
    return out.to(torch.bfloat16)
