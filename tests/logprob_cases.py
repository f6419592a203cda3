"""Shared builders of the log-probability tests (tests/test_logprobs.py on the CPU,
tests/test_logprobs_gpu.py on the device): bf16 rows of every kind the contract names, targets
that include the arg-max, a tied value and the last valid column, and the comparison itself
(ids and ranks exactly, values to ``TOL``).

``TOL`` is derived, not measured (csrc/sampling/logprobs.hip): flooring V <= 2^17 fixed-point
terms to 2^-32 moves ln S by <= 3.0e-5, exp / log add ~3e-7 and the fp32 subtraction at
|lp| <= 200 adds 1.2e-5."""
import numpy as np
import torch

from llm_sharding_amd.ops.logprobs import TOP_MAX, logprobs_reference

TOL = 1e-4
KINDS = ("gaussian", "constant", "near_constant", "spread", "neg_inf")


def gaussian_rows(rows: int, V: int, seed: int = 0, scale: float = 2.0) -> torch.Tensor:
    """N(0, scale^2) rounded to bf16: with V in the thousands the values tie naturally."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((rows, V), generator=g) * scale).to(torch.bfloat16)


def constant_row(V: int, value: float = 1.5) -> torch.Tensor:
    return torch.full((V,), value, dtype=torch.bfloat16)


def near_constant_row(V: int) -> torch.Tensor:
    """Two adjacent bf16 values alternate (the larger on odd columns): the top-20 are the odd
    columns 1, 3, 5, ... - decided purely by index."""
    r = torch.full((V,), 2.0, dtype=torch.bfloat16)
    r[1::2] = 2.015625
    return r


def spread_row(V: int, hot: int, seed: int = 1) -> torch.Tensor:
    """One logit at +80, the rest near -80."""
    g = torch.Generator().manual_seed(seed)
    r = (-80.0 + 0.5 * torch.randn(V, generator=g)).to(torch.bfloat16)
    r[hot % V] = 80.0
    return r


def neg_inf_row(V: int, seed: int = 2) -> torch.Tensor:
    """A Gaussian row with about a third of its entries at -inf (column 0 kept finite)."""
    g = torch.Generator().manual_seed(seed)
    r = (torch.randn(V, generator=g) * 2.0).to(torch.bfloat16)
    m = torch.rand(V, generator=g) < 0.33
    m[0] = False
    r[m] = float("-inf")
    return r


def row_of(kind: str, V: int) -> torch.Tensor:
    return {"gaussian": lambda: gaussian_rows(1, V, 7)[0], "constant": lambda: constant_row(V),
            "near_constant": lambda: near_constant_row(V), "spread": lambda: spread_row(V, V // 3),
            "neg_inf": lambda: neg_inf_row(V)}[kind]()


def targets_of(row: torch.Tensor) -> list:
    """[the arg-max, a later column of a value that occurs at least twice (the last column of the
    most frequent value; the arg-max again if nothing ties), the last valid column]."""
    v = row.float()
    V = v.numel()
    vals, inv, cnt = torch.unique(v, return_inverse=True, return_counts=True)
    tied = int(torch.argmax(v))
    if int(cnt.max()) > 1:
        tied = int(torch.nonzero(inv == int(torch.argmax(cnt)))[-1])
    return [int(torch.argmax(v)), tied, V - 1]


def every_kind(V: int):
    """(logits bf16 [3 * len(KINDS), V], targets, kinds): each kind of row three times, once per
    target of :func:`targets_of`."""
    rows, tg, kinds = [], [], []
    for k in KINDS:
        r = row_of(k, V)
        for t in targets_of(r):
            rows.append(r)
            tg.append(t)
            kinds.append(k)
    return torch.stack(rows), tg, kinds


def mixed_batch(rows: int, V: int, seed: int = 3):
    """Gaussian rows with a few special rows mixed in, per-row targets (arg-max / tied / last /
    random) and ``n_top`` cycling through 0, 1, 5, 20."""
    lg = gaussian_rows(rows, V, seed)
    for i, k in enumerate(KINDS[1:]):
        if 2 + 5 * i < rows:
            lg[2 + 5 * i] = row_of(k, V)
    g = torch.Generator().manual_seed(seed + 100)
    rnd = torch.randint(0, V, (rows,), generator=g).tolist()
    tg = [(targets_of(lg[r]) + [rnd[r]])[r % 4] for r in range(rows)]
    n_top = [(0, 1, 5, 20)[(r // 2) % 4] for r in range(rows)]
    return lg, tg, n_top


def padded(lg: torch.Tensor, ld: int, offset: int = 0, fill: float = float("nan")):
    """``lg`` [rows, V] as a view of a ``fill``-ed buffer with row stride ``ld``, starting
    ``offset`` elements into it (offset 1: row bases are not 16-byte aligned)."""
    rows, V = lg.shape
    buf = torch.full((rows * ld + offset,), fill, dtype=torch.bfloat16)
    view = buf[offset:offset + rows * ld].view(rows, ld)
    view[:, :V] = lg
    return buf, view


def check(got, ref, rows=None, what: str = "") -> float:
    """``got`` (host tensors or arrays of ``Logprobs``) against the reference ``ref``: ids and
    ranks exact, values within TOL (an infinite reference value must be matched exactly).
    Returns the largest value error; prints it."""
    sl = slice(None) if rows is None else rows
    worst = 0.0
    for name in ("tok_rank", "top_id"):
        g, r = np.asarray(getattr(got, name))[sl].astype(np.int64), np.asarray(getattr(ref, name))[sl]
        assert (g == r).all(), f"{what}: {name} differs on rows {np.unique(np.nonzero(g != r)[0])[:8]}"
    for name in ("lse", "tok_lp", "top_lp"):
        g = np.asarray(getattr(got, name))[sl].astype(np.float64)
        r = np.asarray(getattr(ref, name))[sl]
        fin = np.isfinite(r)
        same = (g == r) | (np.isnan(g) & np.isnan(r))
        assert same[~fin].all(), f"{what}: {name} differs where the reference is not finite"
        if fin.any():
            err = float(np.abs(g[fin] - r[fin]).max())
            worst = max(worst, err)
            assert err <= TOL, f"{what}: {name} off by {err:.3e} > {TOL}"
    print(f"{what}: max value error {worst:.3e}")
    return worst


__all__ = ["TOL", "KINDS", "TOP_MAX", "logprobs_reference", "gaussian_rows", "constant_row", "near_constant_row",
           "spread_row", "neg_inf_row", "row_of", "targets_of", "every_kind", "mixed_batch", "padded", "check"]
