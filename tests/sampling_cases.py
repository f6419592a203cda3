"""Shared cases of the sampling tests (tests/test_sampling.py on the CPU, test_sampling_gpu.py
on the device): fixed numpy seeds, bf16-rounded 2.5 * N(0, 1) logits, per-row parameters that
cycle through every path of the contract, and ``top_p`` chosen per row FROM THE DATA.

Why top_p is not random: the device sums masses in 32-bit fixed point and fp32 ``expf`` while
the reference sums in fp64; the two kept sets can only be compared exactly when ``p`` is not
within that error of a cumulative mass. With uniformly random ``p`` margins as small as 1.7e-6
were measured at V = 32000. Here a boundary value-group whose own mass is >= 4e-3 is chosen and
``p`` is set to the cumulative mass through it minus half its mass, so ``|cum - p| >= 2e-3`` on
both sides - about 60x the fp32 error bound of a 256-way partial-sum reduction at V = 128256,
``(V / 256 + 8) * 2^-24 ~= 3e-5``. A row with no such group (flat distributions at high
temperature without top-k) gets ``top_p = 1``.

Each case and its reference result are computed once per process and shared; callers must not
modify them.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np
import torch

from llm_sharding_amd.ops import sampling as S

TEMPS = (0.7, 1.0, 1.3)
MIN_GROUP_MASS = 4e-3
P_MARGIN = 2e-3          # every row's |cum - p| at the top-p boundary is at least this
GAP_MIN = 1e-3           # rows whose two best perturbed scores are closer may differ on the device
GAP_ROWS_MAX = 0.02      # ... and at most this fraction of the rows may be such rows

# (rows, V, ld) of the kernel-vs-reference cases
KERNEL_CASES = ((1, 1000, 1024), (5, 32000, 32000), (129, 50257, 50304), (3, 128256, 128256), (1024, 1000, 1024))


def top_ks(V: int) -> tuple:
    return (0, 7, 50, 5000, V + 5, 1)


@dataclass(frozen=True, eq=False)
class Case:
    rows: int
    V: int
    ld: int
    logits: torch.Tensor    # bf16 [rows, ld]; columns >= V poisoned with the row maximum + 10
    T: np.ndarray           # fp32 [rows]; 0 = greedy
    top_k: np.ndarray       # int32
    top_p: np.ndarray       # fp32
    seed: np.ndarray        # uint64
    ctr: np.ndarray         # int32


def bf16_round(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.asarray(a, dtype=np.float32)).to(torch.bfloat16)


def data_top_p(l64: np.ndarray, T: float, k: int, which: str, rng) -> float:
    """``top_p`` for one row from its own masses (module docstring). ``which``: "first" keeps
    only the best value-group, "last" cuts at the lowest eligible group, "any" at a random one."""
    V = l64.size
    z = l64 / float(np.float32(T))
    if 0 < k < V:
        z = z[z >= np.partition(z, V - k)[V - k]]
    vals, inv = np.unique(z, return_inverse=True)
    gm = np.bincount(inv, weights=np.exp(z - z.max()), minlength=vals.size)[::-1]
    gm = gm / gm.sum()
    cum = np.cumsum(gm)
    ok = np.nonzero(gm >= MIN_GROUP_MASS)[0]
    if which == "first":
        ok = ok[ok == 0]
    if ok.size == 0:
        return 1.0
    j = int(ok[0] if which == "first" else (ok[-1] if which == "last" else rng.choice(ok)))
    p = float(np.float32(cum[j] - 0.5 * gm[j]))
    return p if 0.0 < p < 1.0 else 1.0


@functools.lru_cache(maxsize=None)
def make_case(rows: int, V: int, ld: int) -> Case:
    rng = np.random.default_rng(20240 + 7 * V + rows)
    lg = bf16_round(2.5 * rng.standard_normal((rows, V)))
    l64 = lg.to(torch.float64).numpy()
    full = torch.empty((rows, ld), dtype=torch.bfloat16)
    full[:, :V] = lg
    if ld > V:
        full[:, V:] = (lg.float().max(dim=1, keepdim=True).values + 10.0).to(torch.bfloat16)
    ks = top_ks(V)
    T = np.zeros(rows, dtype=np.float32)
    top_k = np.zeros(rows, dtype=np.int32)
    top_p = np.ones(rows, dtype=np.float32)
    for r in range(rows):
        greedy = r % 7 == 3
        T[r] = 0.0 if greedy else TEMPS[r % 3]
        top_k[r] = ks[(r // 3) % len(ks)] if rows > 2 else ks[2]
        if greedy or r % 5 == 0:
            continue  # top_p = 1
        which = "first" if r % 5 == 1 else "any"
        top_p[r] = data_top_p(l64[r], T[r], int(top_k[r]), which, rng)
    if rows <= 2:  # a single row must still take the whole path: temperature + top-k + top-p
        T[0] = 0.7
        top_p[0] = data_top_p(l64[0], T[0], int(top_k[0]), "any", rng)
    seed = rng.integers(0, 1 << 64, size=rows, dtype=np.uint64)
    ctr = rng.integers(1, 4096, size=rows).astype(np.int32)
    return Case(rows, V, ld, full, T, top_k, top_p, seed, ctr)


@functools.lru_cache(maxsize=None)
def reference(rows: int, V: int, ld: int):
    """``sample_reference`` of the case: (tokens, kept, gap, p_margin)."""
    c = make_case(rows, V, ld)
    return S.sample_reference(c.logits, V, c.T, c.top_k, c.top_p, [int(s) for s in c.seed], c.ctr)


def expected_dbg(rows: int, V: int, ld: int):
    """(threshold key, kept count) per row, as the kernel's ``dbg`` reports them: the smallest
    16-bit key in the kept set (the maximum's key on a greedy row; 0 on a sampled row with both
    filters off, where no threshold is searched) and its size."""
    c = make_case(rows, V, ld)
    _, kept, _, _ = reference(rows, V, ld)
    keys = S.key16(S.bf16_bits(c.logits[:, :V]))
    thr = np.where(kept, keys, 1 << 20).min(axis=1)
    unfiltered = (c.T > 0) & ((c.top_k <= 0) | (c.top_k >= V)) & (c.top_p >= 1)
    return np.where(unfiltered, 0, thr), kept.sum(axis=1)


# ------------------------------------------------------------------------------ goodness of fit
GOF_V, GOF_T, GOF_K, GOF_DRAWS = 1000, 0.8, 40, 8192


@functools.lru_cache(maxsize=None)
def gof_case():
    """One V = 1000 row with T = 0.8, k = 40 and a data-chosen p. Returns (logits bf16 [1, V],
    p, kept bool [V], probs fp64 [V]: the contract's distribution over the kept set)."""
    rng = np.random.default_rng(777)
    lg = bf16_round(2.5 * rng.standard_normal((1, GOF_V)))
    l64 = lg.to(torch.float64).numpy()[0]
    p = data_top_p(l64, GOF_T, GOF_K, "last", rng)
    _, kept, _, pm = S.sample_reference(lg, GOF_V, GOF_T, GOF_K, p, 1, 1)
    assert pm[0] >= P_MARGIN
    z = l64 / float(np.float32(GOF_T))
    w = np.where(kept[0], np.exp(z - z.max()), 0.0)
    return lg, p, kept[0], w / w.sum()


def gof_seeds(n: int = GOF_DRAWS):
    """Distinct (seed, position) pairs of the goodness-of-fit draws."""
    rng = np.random.default_rng(4242)
    return rng.integers(0, 1 << 64, size=n, dtype=np.uint64), (1 + np.arange(n) % 2048).astype(np.int32)


def chi2_stat(tokens: np.ndarray, kept: np.ndarray, probs: np.ndarray):
    """(Pearson chi^2, degrees of freedom, draws outside the kept set, smallest expected count)."""
    tokens = np.asarray(tokens).reshape(-1)
    counts = np.bincount(tokens, minlength=probs.size).astype(np.float64)
    outside = int(counts[~kept].sum())
    exp = probs[kept] * tokens.size
    return float(((counts[kept] - exp) ** 2 / exp).sum()), int(kept.sum()) - 1, outside, float(exp.min())
