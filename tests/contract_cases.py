"""Case builders and checkers for the kernel contract tests (tests/test_contract_cases.py on the
CPU, tests/test_attn_membership_gpu.py and tests/test_footprint_gpu.py on the GPU).

Two contracts that a norm-based comparison on Gaussian inputs cannot see:

* **Exact key membership** of the attention kernels. With ``q = 0`` every score is 0 and every
  softmax weight exactly 1, so a row's output is ``sum_{key < len} V[key] / len``. V carries one
  power of two per key (``V[key, (key + shift) % hd] = 2 ** ((key // hd) % 6)``), so with
  ``t_max <= 12 * hd`` every per-dim sum is an integer <= 126 and ``round(out * len)`` must be
  exactly the integer vector of keys ``[0, len)``: one key too few or too many moves one dim by
  at least 1, while the bf16 rounding of the output moves it by less than
  ``126 * 2 ** -8 < 0.5``. Every cache cell at ``key >= len`` (and every unused slot) is NaN.
* **Write / read footprints.** Outputs are windows inside larger buffers pre-filled with a
  sentinel bit pattern; after the launch every element outside the window must still hold the
  sentinel and every element inside must not. Operands carry NaN in every row / column the
  kernel has no business reading.

Everything here is plain torch and runs on any device.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import torch

# ------------------------------------------------------------------------------ sentinels
# bf16: a quiet NaN with a payload (a NaN a kernel computes is 0x7FC0 / 0xFFC0); fp32: another
# payload; integers: -12345
_SENT = {
    torch.bfloat16: (torch.int16, 0x7FC1),
    torch.float32: (torch.int32, 0x7FC00BAD),
    torch.int32: (torch.int32, -12345),
    torch.int64: (torch.int64, -12345),
}
GUARD_ROWS = 256  # one full largest row tile (gemm_sk bm = 256)
GUARD_COLS = 64   # ld = N + 64 keeps ld % 8 == 0 (16-byte aligned rows)


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(_SENT[t.dtype][0])


def sentinel_fill(t: torch.Tensor) -> torch.Tensor:
    bits(t).fill_(_SENT[t.dtype][1])
    return t


def is_sentinel(t: torch.Tensor) -> torch.Tensor:
    return bits(t) == _SENT[t.dtype][1]


def guarded(rows: int, cols: int, dtype=torch.bfloat16, device="cpu", guard_rows: int = GUARD_ROWS,
            guard_cols: int = GUARD_COLS):
    """(buf, window): ``window`` is the [rows, cols] view at row ``guard_rows``, column 0 of the
    sentinel-filled ``buf`` [guard_rows + rows + guard_rows, cols + guard_cols]."""
    buf = sentinel_fill(torch.empty(rows + 2 * guard_rows, cols + guard_cols, dtype=dtype, device=device))
    return buf, buf[guard_rows:guard_rows + rows, :cols]


def guarded_flat(n: int, dtype=torch.float32, device="cpu", guard: int = 4096):
    """(buf, window) for a 1-D buffer of ``n`` elements with ``guard`` sentinels on each side."""
    buf = sentinel_fill(torch.empty(n + 2 * guard, dtype=dtype, device=device))
    return buf, buf[guard:guard + n]


def operand(rows: int, cols: int, device="cpu", scale: float = 1.0, gen=None, dtype=torch.bfloat16,
            guard_rows: int = GUARD_ROWS, guard_cols: int = GUARD_COLS):
    """(buf, window): a random [rows, cols] operand inside a NaN buffer (rows beyond ``rows`` and
    columns beyond ``cols`` are the NaN sentinel): whatever a kernel reads outside the window
    shows up as a non-finite result."""
    buf, win = guarded(rows, cols, dtype, device, guard_rows, guard_cols)
    win.copy_((torch.randn(rows, cols, device=device, generator=gen) * scale).to(dtype))
    return buf, win


def window_mask(buf: torch.Tensor, window: torch.Tensor) -> torch.Tensor:
    """Bool mask over ``buf`` (contiguous) of the elements that ``window`` (a view of it) covers."""
    assert buf.is_contiguous() and window.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr()
    m = torch.zeros(buf.numel(), dtype=torch.bool, device=buf.device)
    m.as_strided(tuple(window.shape), tuple(window.stride()), window.storage_offset() - buf.storage_offset()).fill_(True)
    return m.view(buf.shape)


def _where(bad: torch.Tensor, limit: int = 5) -> str:
    idx = bad.nonzero()[:limit].tolist()
    return f"{int(bad.sum())} element(s), first at {idx}"


def assert_footprint_mask(buf: torch.Tensor, mask: torch.Tensor, optional: Optional[torch.Tensor] = None,
                          inside: str = "written", what: str = "") -> None:
    """``mask`` (bool, ``buf``'s shape): True = must have been written (no longer the sentinel),
    False = must still be the bit-identical sentinel. ``optional``: elements that may be either.
    ``inside="any"``: only the outside is checked (workspaces a kernel may leave partly unused)."""
    sent = is_sentinel(buf)
    outside_bad = ~mask & ~sent
    unwritten = mask & sent
    if optional is not None:
        outside_bad &= ~optional
        unwritten &= ~optional
    assert not bool(outside_bad.any()), f"{what}: written outside the window: {_where(outside_bad)}"
    if inside == "written":
        assert not bool(unwritten.any()), f"{what}: left unwritten inside the window: {_where(unwritten)}"


def assert_footprint(buf: torch.Tensor, window: torch.Tensor, optional: Optional[torch.Tensor] = None,
                     inside: str = "written", what: str = "") -> None:
    """Every element of ``buf`` outside ``window`` is still the sentinel (bit compare), every
    element inside is not. ``optional``: bool, the window's shape, elements that may be either."""
    mask = window_mask(buf, window)
    opt = None
    if optional is not None:
        opt = torch.zeros_like(mask)
        opt.view(-1).as_strided(tuple(window.shape), tuple(window.stride()),
                                window.storage_offset() - buf.storage_offset()).copy_(optional)
    assert_footprint_mask(buf, mask, opt, inside, what)


# ------------------------------------------------------------------------------ KV cache
def guarded_cache(slots: int, n_kv: int, t_max: int, hd: int, device="cpu", dtype=torch.bfloat16):
    """(flat, cache): a [slots, n_kv, t_max, hd] cache view inside a sentinel-filled flat
    allocation with a guard band of 512 key rows on each side."""
    g, n = 512 * hd, slots * n_kv * t_max * hd
    flat = sentinel_fill(torch.empty(n + 2 * g, dtype=dtype, device=device))
    return flat, flat[g:g + n].view(slots, n_kv, t_max, hd)


def cache_cells_mask(flat: torch.Tensor, cache: torch.Tensor, slot, pos) -> torch.Tensor:
    """Mask over ``flat`` of the cells (slot[m], every head, pos[m], :)."""
    m = torch.zeros(flat.numel(), dtype=torch.bool, device=flat.device)
    mv = m.as_strided(tuple(cache.shape), tuple(cache.stride()), cache.storage_offset() - flat.storage_offset())
    mv[torch.as_tensor(slot).long().to(flat.device), :, torch.as_tensor(pos).long().to(flat.device), :] = True
    return m


def assert_cache_footprint(flat: torch.Tensor, cache: torch.Tensor, slot, pos, what: str = "") -> None:
    """Exactly the cells (slot[m], head, pos[m], :) of the cache were written; every other cell of
    the allocation (guard bands included) is the bit-identical sentinel."""
    assert_footprint_mask(flat, cache_cells_mask(flat, cache, slot, pos), what=what)


# ------------------------------------------------------------------------------ membership
BASE_LENGTHS = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513]


def t_max_for(hd: int) -> int:
    """Deliberately no multiple of 32 or 64, and <= 12 * hd (per-dim sums stay <= 126)."""
    return 1100 if hd == 128 else 750


def _dedupe(xs):
    seen, out = set(), []
    for x in xs:
        if x not in seen:
            seen.add(x)
            out.append(x)
    return out


def membership_lengths(hd: int, extra=()) -> list:
    t_max = t_max_for(hd)
    out = _dedupe(BASE_LENGTHS + ([1023, 1024, 1025, 1100] if hd == 128 else []) + [t_max] + list(extra))
    assert all(1 <= x <= t_max for x in out), out
    return out


def split_chunk(T: int, nsplit: int, hd: int, min_chunk: int = 64, waves: int = 4) -> int:
    """Keys per split of the split-KV decode kernel (csrc/kernels/attn_body.h:54-58):
    ``chunk = ceil(T / nsplit)``, at least ``min_chunk``, rounded up to KPI = keys per workgroup
    iteration = (64 lanes / (hd / 8) lanes per key) * waves."""
    kpi = (64 // (hd // 8)) * waves
    chunk = -(-T // nsplit)
    chunk = max(chunk, min_chunk)
    return -(-chunk // kpi) * kpi


def split_edge_lengths(hd: int, nsplit: int) -> list:
    """c - 1, c, c + 1 around every chunk edge c of the longest and of a mid-sized context."""
    t_max = t_max_for(hd)
    out = []
    for T in (t_max, 513):
        chunk = split_chunk(T, nsplit, hd)
        for s in range(1, nsplit):
            c = s * chunk
            if c < T:
                out += [x for x in (c - 1, c, c + 1) if 1 <= x <= t_max]
    return _dedupe(out)


def pad_lengths(lens: list, n: int) -> list:
    """``lens`` repeated cyclically up to at least ``n`` rows."""
    out = list(lens)
    i = 0
    while len(out) < n:
        out.append(lens[i % len(lens)])
        i += 1
    return out


def batches(rows: int, b: int) -> list:
    """Row ranges of ``b`` rows covering [0, rows) (the last one overlaps the one before)."""
    assert rows >= b
    out = [(r, r + b) for r in range(0, rows - b + 1, b)]
    if out[-1][1] != rows:
        out.append((rows - b, rows))
    return out


def v_weight(key: torch.Tensor, hd: int) -> torch.Tensor:
    return 2 ** ((key // hd) % 6)


@dataclass
class AttnCase:
    nh: int
    nkv: int
    hd: int
    t_max: int
    lens: list
    kflat: torch.Tensor
    vflat: torch.Tensor
    K: torch.Tensor          # [slots, nkv, t_max, hd] view of kflat
    V: torch.Tensor
    slot: torch.Tensor       # int32 [rows]
    pos: torch.Tensor        # int32 [rows] = len - 1
    kv_len: torch.Tensor     # int32 [rows]
    pos_decoy: torch.Tensor  # int32 [rows]: valid positions != len - 1 (the kv_len form must ignore pos)
    shift: Optional[torch.Tensor] = None     # int64 [slots, nkv]
    expected: Optional[torch.Tensor] = None  # int64 [rows, nkv, hd]

    @property
    def rows(self) -> int:
        return len(self.lens)

    @property
    def lens_t(self) -> torch.Tensor:
        return self.kv_len.long()


def _assign_slots(lens: list, t_max: int):
    """One slot per row plus two unused (all-NaN) slots; the last row with len == t_max gets the
    last slot, the others a rotated order."""
    rows = len(lens)
    slots = rows + 2
    unused = {0, slots // 2}
    avail = [s for s in range(slots) if s not in unused]
    full = [i for i, x in enumerate(lens) if x == t_max]
    slot = [None] * rows
    if full and (slots - 1) in avail:
        slot[full[-1]] = slots - 1
        avail.remove(slots - 1)
    rest = [i for i in range(rows) if slot[i] is None]
    rot = avail[3 % len(avail):] + avail[:3 % len(avail)] if avail else []
    for i, s in zip(rest, rot):
        slot[i] = s
    return slots, slot


def _case_common(nh, nkv, hd, lens, device):
    t_max = t_max_for(hd)
    assert t_max <= 12 * hd and all(1 <= x <= t_max for x in lens)
    slots, slot = _assign_slots(lens, t_max)
    kflat, K = guarded_cache(slots, nkv, t_max, hd, device)
    vflat, V = guarded_cache(slots, nkv, t_max, hd, device)
    lens_t = torch.tensor(lens, dtype=torch.int64, device=device)
    slot_t = torch.tensor(slot, dtype=torch.int64, device=device)
    key = torch.arange(t_max, device=device)
    valid = key[None, :] < lens_t[:, None]                                  # [rows, t_max]
    decoy = (lens_t * 7 + 3) % t_max
    decoy = torch.where(decoy == lens_t - 1, (decoy + 1) % t_max, decoy)
    case = AttnCase(nh, nkv, hd, t_max, list(lens), kflat, vflat, K, V, slot_t.to(torch.int32),
                    (lens_t - 1).to(torch.int32), lens_t.to(torch.int32), decoy.to(torch.int32))
    return case, slot_t, lens_t, key, valid


def build_membership_case(nh: int, nkv: int, hd: int, lens: list, device="cpu") -> AttnCase:
    """Cache for one row per entry of ``lens``: valid keys hold the power-of-two V pattern
    (rotated by a per-(slot, kv-head) shift, so a wrong slot or head decodes wrong too) and finite
    K; every cell at key >= len and every unused slot is the NaN sentinel."""
    case, slot_t, lens_t, key, valid = _case_common(nh, nkv, hd, lens, device)
    t_max, slots = case.t_max, case.K.shape[0]
    nan = sentinel_fill(torch.empty((), dtype=torch.bfloat16, device=device))  # the payload survives a select
    d = torch.arange(hd, device=device)
    shift = (7 * torch.arange(slots, device=device)[:, None] + 3 * torch.arange(nkv, device=device)[None, :]) % hd
    case.shift = shift
    sh = shift[slot_t]                                                       # [rows, nkv]
    # V[row, kvh, key, dim] = w[key] where dim == (key + shift) % hd
    hit = (d[None, None, None, :] - sh[:, :, None, None]) % hd == (key % hd)[None, None, :, None]
    w = v_weight(key, hd).to(torch.bfloat16)[None, None, :, None]
    vv = torch.where(hit, w, torch.zeros((), dtype=torch.bfloat16, device=device))
    case.V[slot_t] = torch.where(valid[:, None, :, None], vv, nan)
    kpat = (((key[:, None] * 5 + d[None, :] * 3) % 17 - 8).float() / 8).to(torch.bfloat16)  # finite, exact
    case.K[slot_t] = torch.where(valid[:, None, :, None], kpat[None, None], nan)
    case.expected = expected_rows(case, slot_t, lens_t)
    return case


def expected_rows(case: AttnCase, slots: torch.Tensor, lens: torch.Tensor) -> torch.Tensor:
    """int64 [n, nkv, hd]: the integer per-dim sums of keys [0, lens[i]) of slot slots[i]
    (table[len][dim] for shift 0, rotated by the (slot, kv head) shift)."""
    dev, hd, t_max = case.V.device, case.hd, case.t_max
    key, d = torch.arange(t_max, device=dev), torch.arange(hd, device=dev)
    onehot = torch.zeros(t_max + 1, hd, dtype=torch.int64, device=dev)
    onehot[key + 1, key % hd] = v_weight(key, hd)
    base = onehot.cumsum(0)[lens.long().to(dev)]                             # [n, hd]
    sh = case.shift[slots.long().to(dev)]                                    # [n, nkv]
    idx = (d[None, None, :] - sh[:, :, None]) % hd                           # [n, nkv, hd]
    return base[:, None, :].expand(-1, case.nkv, -1).gather(2, idx)


def pattern_v_row(case: AttnCase, row: int, key: int) -> torch.Tensor:
    """The pattern's V[key] for ``row``'s slot, all kv heads ([nkv, hd], fp64): what the cache
    would hold at ``key`` if it were valid (used to model a kernel that lets key ``len`` in)."""
    dev = case.V.device
    sh = case.shift[case.slot[row].long()]                                   # [nkv]
    out = torch.zeros(case.nkv, case.hd, dtype=torch.float64, device=dev)
    out[torch.arange(case.nkv, device=dev), (key + sh) % case.hd] = float(2 ** ((key // case.hd) % 6))
    return out


def membership_reference(case: AttnCase, drop: Optional[str] = None, add: bool = False,
                         renormalise: bool = True) -> torch.Tensor:
    """bf16 [rows, nh * hd]: the fp64 mean of the cache's V rows over a row's key set, rounded to
    bf16 once. ``drop``: "last" / "middle" leaves key len - 1 / len // 2 out, ``add`` lets key
    ``len`` in (a faulty kernel's key set); ``renormalise``: the faulty softmax also divides by the
    faulty key count (else by len)."""
    g = case.nh // case.nkv
    out = torch.zeros(case.rows, case.nh, case.hd, dtype=torch.float64, device=case.V.device)
    for r, T in enumerate(case.lens):
        s = int(case.slot[r])
        acc = case.V[s, :, :T].double().sum(1)                               # [nkv, hd]
        n = T
        if drop is not None:
            k = T - 1 if drop == "last" else T // 2
            acc = acc - case.V[s, :, k].double()
            n -= 1
        if add:
            acc = acc + pattern_v_row(case, r, T)
            n += 1
        out[r] = (acc / (n if renormalise else T)).repeat_interleave(g, 0)
    return out.reshape(case.rows, -1).to(torch.bfloat16)


def decode_membership(out: torch.Tensor, lens_t: torch.Tensor, nh: int, hd: int):
    """(ints [rows, nh, hd] int64, worst |out * len - ints|)."""
    o = out.double().view(out.shape[0], nh, hd) * lens_t.to(out.device).double()[:, None, None]
    ints = o.round()
    resid = float((o - ints).abs().max()) if o.numel() else 0.0
    return ints.long(), resid


def check_membership(out: torch.Tensor, case: AttnCase, r0: int = 0, r1: Optional[int] = None,
                     what: str = "", expected: Optional[torch.Tensor] = None,
                     lens_t: Optional[torch.Tensor] = None) -> float:
    """``out`` [r1 - r0, >= nh * hd] decodes to exactly the keys [0, len) of rows r0 .. r1;
    returns the worst decode residual."""
    r1 = case.rows if r1 is None else r1
    nh, hd, g = case.nh, case.hd, case.nh // case.nkv
    o = out[:, :nh * hd]
    assert bool(torch.isfinite(o.float()).all()), f"{what}: non-finite output (poisoned cache cells leaked in)"
    lens_t = case.lens_t[r0:r1] if lens_t is None else lens_t
    exp = (case.expected[r0:r1] if expected is None else expected).repeat_interleave(g, 1)  # [rows, nh, hd]
    ints, resid = decode_membership(o.contiguous(), lens_t, nh, hd)
    bad = (ints != exp.to(ints.device)).any(-1)                              # [rows, nh]
    if bool(bad.any()):
        r, hh = bad.nonzero()[0].tolist()
        dim = int((ints[r, hh] != exp[r, hh]).nonzero()[0])
        raise AssertionError(
            f"{what}: row {r0 + r} (len {int(lens_t[r])}) head {hh}: dim {dim} decodes to {int(ints[r, hh, dim])}, "
            f"keys [0, len) give {int(exp[r, hh, dim])}; {int(bad.sum())} (row, head) pairs differ")
    return resid


# ------------------------------------------------------------------------------ score range
def build_score_case(nh: int, nkv: int, hd: int, lens: list, device="cpu", rising: bool = True, seed: int = 0):
    """(case, q): scores that are not Gaussian. q = c * e_0 for every head and K[key, 0] ramps
    over the row's own context from -4 to 4 (rising) or 4 to -4, with c chosen so that
    score * log2(e) spans 80: the running maximum moves in every block (rising) or never
    (falling). V is Gaussian + 4; cells at key >= len are NaN as in the membership cases."""
    case, slot_t, lens_t, key, valid = _case_common(nh, nkv, hd, lens, device)
    gen = torch.Generator(device=device).manual_seed(seed)
    nan = sentinel_fill(torch.empty((), dtype=torch.bfloat16, device=device))  # the payload survives a select
    rows, t_max = case.rows, case.t_max
    a = 4.0
    c = 80.0 / (2 * a * hd ** -0.5 * math.log2(math.e))
    span = (lens_t - 1).clamp(min=1).double()
    ramp = a * (2 * key[None, :].double() / span[:, None] - 1)               # [rows, t_max]
    if not rising:
        ramp = -ramp
    kk = torch.randn(rows, nkv, t_max, hd, device=device, generator=gen) * 0.5
    kk[..., 0] = ramp[:, None, :].float()
    vv = torch.randn(rows, nkv, t_max, hd, device=device, generator=gen) + 4.0
    case.K[slot_t] = torch.where(valid[:, None, :, None], kk.to(torch.bfloat16), nan)
    case.V[slot_t] = torch.where(valid[:, None, :, None], vv.to(torch.bfloat16), nan)
    q = torch.zeros(rows, nh, hd, dtype=torch.bfloat16, device=device)
    q[:, :, 0] = c
    return case, q.view(rows, nh * hd)


def attention_reference(q: torch.Tensor, case: AttnCase, lens=None, rows=None) -> torch.Tensor:
    """fp64 softmax attention of row r over keys [0, len_r) of its slot: [rows, nh * hd]."""
    nh, nkv, hd = case.nh, case.nkv, case.hd
    g = nh // nkv
    rows = range(case.rows) if rows is None else rows
    out = torch.zeros(len(rows), nh, hd, dtype=torch.float64, device=q.device)
    for i, r in enumerate(rows):
        T = int(case.lens[r] if lens is None else lens[i])
        s = int(case.slot[r])
        k = case.K[s, :, :T].double().repeat_interleave(g, 0)                # [nh, T, hd]
        v = case.V[s, :, :T].double().repeat_interleave(g, 0)
        sc = torch.einsum("hd,htd->ht", q[i].double().view(nh, hd), k) * hd ** -0.5
        out[i] = torch.einsum("ht,htd->hd", torch.softmax(sc, -1), v)
    return out.reshape(len(rows), nh * hd)


def guarded_q(q: torch.Tensor):
    """(buf, window): ``q`` copied into a NaN-padded buffer (rows beyond it and columns beyond
    n_heads * head_dim are NaN; ldq = width + 64)."""
    buf, win = guarded(q.shape[0], q.shape[1], q.dtype, q.device)
    win.copy_(q)
    return buf, win
