"""Shared builders of the paged KV cache tests (tests/test_kv_paged.py on the CPU,
tests/test_kv_paged_gpu.py on the GPU): shuffled block tables, append / gather cases with their
expected bytes from the torch references of ops/kv_paged.py, and attention cases whose pages are a
static cache cut up under a shuffled table with NaN everywhere else. Everything here runs on the CPU."""
import functools

import torch

from llm_sharding_amd.ops import kv_paged as KP

PAGE = KP.PAGE
SENTINEL = 0x7FC1  # a bf16 NaN pattern no computation produces: marks bytes nobody may write


def shuffled_table(lens, max_seq: int, n_pages: int, seed: int = 0) -> torch.Tensor:
    """int32 [len(lens), max_seq / PAGE]: slot s holds pages for ``lens[s]`` tokens, dealt from a
    random permutation of [1, n_pages) one page per slot in turn, so the pages of one slot are
    non-monotone and interleaved with the other slots'. Unassigned entries are 0."""
    need = [KP.pages_for(n) for n in lens]
    assert sum(need) <= n_pages - 1 and max(lens, default=0) <= max_seq
    g = torch.Generator().manual_seed(seed)
    perm = (torch.randperm(n_pages - 1, generator=g) + 1).tolist()
    table = torch.zeros((len(lens), max_seq // PAGE), dtype=torch.int32)
    for i in range(max(need, default=0)):
        for s, n in enumerate(need):
            if i < n:
                table[s, i] = perm.pop()
    return table


def live_pages_assigned(table: torch.Tensor, slot, lens, n_pages: int) -> bool:
    """Every page a row reads (slot[r], tokens [0, lens[r])) is assigned, and no page serves two
    (slot, index) entries: the condition under which paged and static attention see the same keys."""
    tab = KP.sanitize_table(table, n_pages)
    used = tab[tab > 0].tolist()
    if len(set(used)) != len(used):
        return False
    return all(bool((tab[s, :KP.pages_for(n)] > 0).all()) for s, n in zip(slot, lens))


def pages_from_static(k: torch.Tensor, v: torch.Tensor, table: torch.Tensor, n_pages: int, fill: float = float("nan")):
    """Cut a static [slots, n_kv, T, hd] pair into pools under ``table``; every unassigned page and
    page 0 hold ``fill``."""
    S, n_kv, T, hd = k.shape
    kp = torch.full((n_pages, n_kv, PAGE, hd), fill, dtype=k.dtype)
    vp = torch.full((n_pages, n_kv, PAGE, hd), fill, dtype=v.dtype)
    for s in range(S):
        for i, pg in enumerate(table[s].tolist()):
            if 1 <= pg < n_pages:
                kp[pg] = k[s, :, i * PAGE:(i + 1) * PAGE]
                vp[pg] = v[s, :, i * PAGE:(i + 1) * PAGE]
    return kp, vp


def sentinel_pool(n_pages: int, n_kv: int, hd: int) -> torch.Tensor:
    return torch.full((n_pages, n_kv, PAGE, hd), SENTINEL, dtype=torch.int16).view(torch.bfloat16)


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.cpu().contiguous().view(torch.int16)


# ------------------------------------------------------------------------------ append / gather
@functools.lru_cache(maxsize=None)
def append_case(hd: int, n_kv: int, rows: int) -> dict:
    """``rows`` distinct cells over 5 slots of a 192-token cache (positions 63 and 64, both sides of
    a page edge, among them), a shuffled interleaved table with spare pages, sentinel pools and the
    pools the reference leaves. Slot 4 keeps a null entry for its last page."""
    S, T, n_pages = 5, 192, 19
    g = torch.Generator().manual_seed(1000 * hd + 10 * n_kv + rows)
    kst = torch.randn(S, n_kv, T, hd, generator=g).to(torch.bfloat16)
    vst = torch.randn(S, n_kv, T, hd, generator=g).to(torch.bfloat16)
    table = shuffled_table([T, T, T, T, T - PAGE], T, n_pages, seed=rows)
    cells = [(0, 63), (0, 64), (1, 0), (2, 127), (3, 128), (1, 191), (4, 5)]
    free = [(s, p) for s in range(S) for p in range(T - PAGE if s == 4 else T) if (s, p) not in cells]
    perm = torch.randperm(len(free), generator=g).tolist()
    cells = (cells + [free[i] for i in perm])[:rows]
    slot, pos = [c[0] for c in cells], [c[1] for c in cells]
    kp, vp = sentinel_pool(n_pages, n_kv, hd), sentinel_pool(n_pages, n_kv, hd)
    KP.append_reference(kst, vst, kp, vp, table, slot, pos)
    return {"shape": (S, n_kv, T, hd), "n_pages": n_pages, "kst": kst, "vst": vst, "table": table, "slot": slot,
            "pos": pos, "exp": (kp, vp)}


# ------------------------------------------------------------------------------ attention
CONTEXTS = (1, 63, 64, 65, 130, 1100)
ATTN_MAX_SEQ = 1152   # 18 pages
ATTN_N_KV = 2


@functools.lru_cache(maxsize=None)
def attn_case(hd: int, g: int) -> dict:
    """Slot s holds CONTEXTS[s] Gaussian K/V tokens (NaN beyond them) in a static cache and, cut up
    under a shuffled table, in pools whose every other page - page 0 included - is NaN."""
    gen = torch.Generator().manual_seed(100 * hd + g)
    S, n_kv, T = len(CONTEXTS), ATTN_N_KV, ATTN_MAX_SEQ
    k = torch.full((S, n_kv, T, hd), float("nan"), dtype=torch.bfloat16)
    v = torch.full((S, n_kv, T, hd), float("nan"), dtype=torch.bfloat16)
    for s, n in enumerate(CONTEXTS):
        k[s, :, :n] = torch.randn(n_kv, n, hd, generator=gen).to(torch.bfloat16)
        v[s, :, :n] = torch.randn(n_kv, n, hd, generator=gen).to(torch.bfloat16)
    n_pages = sum(KP.pages_for(n) for n in CONTEXTS) + 1 + 7      # 7 pages nobody owns
    table = shuffled_table(CONTEXTS, T, n_pages, seed=hd + g)
    kp, vp = pages_from_static(k, v, table, n_pages)
    q = torch.randn(129, g * n_kv * hd, generator=gen).to(torch.bfloat16)
    return {"k": k, "v": v, "kp": kp, "vp": vp, "table": table, "n_pages": n_pages, "q": q, "n_heads": g * n_kv,
            "n_kv": n_kv, "hd": hd}


def attn_rows(rows: int, first: int = 0) -> tuple:
    """(slot, lens) of a launch: row r reads slot (first + r) % 6; the first visit of a slot reads
    its whole context, later visits a shorter prefix, so lengths mix inside one launch."""
    slot = [(first + r) % len(CONTEXTS) for r in range(rows)]
    lens = [max(1, CONTEXTS[s] - 7 * (r // len(CONTEXTS))) for r, s in enumerate(slot)]
    return slot, lens


def attn_reference(q: torch.Tensor, kp: torch.Tensor, vp: torch.Tensor, table: torch.Tensor, slot, lens,
                   n_heads: int) -> torch.Tensor:
    """fp64 softmax attention of row r over keys [0, lens[r]) of slot[r], read from the static
    tensors the table describes: [rows, n_heads * hd]."""
    k, v = KP.to_static(kp, vp, table)
    n_kv, hd = k.shape[1], k.shape[3]
    g = n_heads // n_kv
    out = torch.zeros(len(slot), n_heads, hd, dtype=torch.float64)
    for r, (s, T) in enumerate(zip(slot, lens)):
        kk = k[s, :, :T].double().repeat_interleave(g, 0)
        vv = v[s, :, :T].double().repeat_interleave(g, 0)
        w = torch.einsum("hd,htd->ht", q[r, :n_heads * hd].double().view(n_heads, hd), kk) * hd ** -0.5
        out[r] = torch.einsum("ht,htd->hd", torch.softmax(w, -1), vv)
    return out.reshape(len(slot), n_heads * hd)
