"""Case builders for the fp8 KV cache tests (tests/test_kv8.py on the CPU, tests/test_kv8_gpu.py on
the GPU). Everything here is plain torch on the CPU: references are computed once per process
(lru_cache) and only copied to the device by the tests.

* ``vector_pool(hd)``: every one of the 65280 finite bf16 bit patterns, twice - sorted by
  magnitude and cut into vectors (each vector covers a narrow range, the maxima sweep the whole
  format from the denormals to 3.4e38), and dealt round-robin (each vector spans the whole
  format, so most of its values vanish against its maximum) - plus Gaussian vectors at scales
  2^-20 .. 2^20.
* ``append_case``: staging tensors filled from the pool, rows on permuted slots with several
  positions per slot, and the expected fp8 tensors inside guarded allocations.
* ``quantize_cache``: a contract_cases attention cache (NaN beyond every length) as fp8 tensors
  whose cells at or beyond each length, and unused slots, hold the NaN code and a NaN scale.
"""
from __future__ import annotations

import functools

import torch

import contract_cases as C
from llm_sharding_amd.ops import kv8

U8_SENT = 0xA5          # sentinel byte of guarded uint8 buffers (an ordinary finite code: only bit compares see it)
NAN_CODE = 0x7F         # e4m3fn NaN
GUARD_KEYS = 512        # guard band, in key rows, on each side of a guarded tensor


def finite_bf16_patterns() -> torch.Tensor:
    """All 65280 finite bf16 values (bf16 [65280]), sorted by magnitude, negative before positive."""
    b = torch.arange(1 << 16, dtype=torch.int32)
    b = b[(b & 0x7F80) != 0x7F80]
    key = (b & 0x7FFF) * 2 + (1 - (b >> 15))
    b = b[torch.argsort(key)]
    assert b.numel() == 65280
    return b.to(torch.int16).view(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def vector_pool(hd: int):
    """(pool bf16 [n, hd], n_pattern_vectors): the first ``n_pattern_vectors`` rows hold every
    finite bf16 pattern twice (sorted runs, then round-robin), the rest are Gaussian."""
    p = finite_bf16_patterns()
    n = p.numel() // hd
    a = p.view(n, hd)
    b = p.view(hd, n).t().contiguous()
    g = torch.Generator().manual_seed(hd)
    k = torch.arange(-20, 21, dtype=torch.float32).repeat_interleave(6)
    gauss = (torch.randn(k.numel(), hd, generator=g) * (2.0 ** k)[:, None]).to(torch.bfloat16)
    return torch.cat([a, b, gauss]), 2 * n


def guarded_u8(shape, device="cpu"):
    """(flat, view): a uint8 tensor of ``shape`` [..., t, hd] inside a U8_SENT-filled allocation."""
    g, n = GUARD_KEYS * shape[-1], int(torch.tensor(shape).prod())
    flat = torch.full((n + 2 * g,), U8_SENT, dtype=torch.uint8, device=device)
    return flat, flat[g:g + n].view(*shape)


def guarded_f32(shape, device="cpu"):
    """(flat, view): an fp32 tensor of ``shape`` inside a sentinel-filled allocation."""
    g, n = GUARD_KEYS, int(torch.tensor(shape).prod())
    flat = C.sentinel_fill(torch.empty(n + 2 * g, dtype=torch.float32, device=device))
    return flat, flat[g:g + n].view(*shape)


def append_rows(rows: int, t_max: int):
    """(n_slots, slot, pos): rows on permuted slots (at most 37 in use, two never named), several
    positions per slot once rows exceed them; all cells distinct."""
    used = min(rows, 37)
    n_slots = used + 2
    perm = [(5 * i + 3) % used + 1 for i in range(used)]          # slots 1 .. used, slot 0 and the last unused
    assert sorted(perm) == list(range(1, used + 1))
    slot = [perm[m % used] for m in range(rows)]
    pos = [((m // used) * 7 + 3 * slot[m]) % t_max for m in range(rows)]
    assert len(set(zip(slot, pos))) == rows and -(-rows // used) <= t_max
    return n_slots, slot, pos


@functools.lru_cache(maxsize=None)
def append_case(hd: int, n_kv: int, rows: int, t_max: int = 40) -> dict:
    """Staging tensors (zeros except the named cells), the rows, and the expected fp8 tensors as
    whole guarded allocations: sentinel everywhere except the named cells."""
    pool, n_pat = vector_pool(hd)
    n_slots, slot, pos = append_rows(rows, t_max)
    sl, ps = torch.tensor(slot), torch.tensor(pos)
    idx = torch.arange(rows * n_kv).view(rows, n_kv)
    kvec = pool[idx % pool.shape[0]]                                # [rows, n_kv, hd]
    vvec = pool[(idx + pool.shape[0] // 2 + 1) % pool.shape[0]]
    shape = (n_slots, n_kv, t_max, hd)
    kst, vst = torch.zeros(shape, dtype=torch.bfloat16), torch.zeros(shape, dtype=torch.bfloat16)
    kst[sl, :, ps], vst[sl, :, ps] = kvec, vvec
    exp = {}
    for name, vec in (("k", kvec), ("v", vvec)):
        codes, s = kv8.quantize_reference(vec)
        f8, c8 = guarded_u8(shape)
        fs, cs = guarded_f32(shape[:3])
        c8[sl, :, ps], cs[sl, :, ps] = codes, s
        exp[name + "8"], exp[name + "s"] = f8, fs
    return {"shape": shape, "slot": slot, "pos": pos, "kst": kst, "vst": vst, "exp": exp,
            "covers_all_patterns": rows * n_kv >= n_pat}


def quantize_cache(K: torch.Tensor, V: torch.Tensor):
    """(k8, v8, ks, vs) of a bf16 cache [slots, n_kv, t, hd] whose invalid cells are NaN: valid
    vectors by the reference, every vector with a NaN in it as NAN_CODE codes and a NaN scale."""
    out = []
    for t in (K.cpu(), V.cpu()):
        bad = torch.isnan(t.float()).any(-1)
        codes, s = kv8.quantize_reference(torch.where(bad[..., None], torch.zeros((), dtype=t.dtype), t))
        codes[bad] = NAN_CODE
        s[bad] = float("nan")
        out.append((codes, s))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def kv8_edge_lengths(hd: int, kpi: int, nsplits=(4, 16), min_chunk: int = 64) -> list:
    """c - 1, c, c + 1 around every chunk edge c of a kernel with ``kpi`` keys per iteration, for
    the longest and a mid-sized context."""
    t_max = C.t_max_for(hd)
    out = []
    for nsplit in nsplits:
        for T in (t_max, 513):
            chunk = kv8.split_chunk_kv8(T, nsplit, kpi, min_chunk)
            for s in range(1, nsplit):
                c = s * chunk
                if c < T:
                    out += [x for x in (c - 1, c, c + 1) if 1 <= x <= t_max]
    return sorted(set(out))
