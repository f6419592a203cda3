"""Builders shared by tests/test_speculative.py (CPU) and tests/test_speculative_gpu.py: hand-built
histories with their expected drafts, random draft / accept states, prompts and scripts."""
import numpy as np
import torch

# (name, history, k, (nmin, nmax), expected drafts, expected matched) - lookup mode, worked by hand
DRAFT_CASES = [
    ("L=1", [7], 3, (1, 3), [7, 7, 7], 0),
    ("L=2 no match", [7, 8], 3, (1, 3), [8, 8, 8], 0),
    ("L=2 match at e=0", [8, 8], 3, (1, 3), [8, 8, 8], 1),           # c = 1, period 1: hist[1] repeated
    ("match ending at e=0", [5, 9, 4, 5], 2, (1, 3), [9, 4], 1),
    ("match ending at e=L-2", [1, 2, 3, 3], 2, (1, 3), [3, 3], 1),    # c = 3 = L-1: the drafts extend themselves
    ("equal m: the later wins", [5, 1, 5, 2, 5], 2, (1, 3), [2, 5], 1),
    ("longer and older beats shorter and newer", [1, 2, 3, 9, 3, 8, 1, 2, 3], 3, (1, 3), [9, 3, 8], 3),
    ("m capped at nmax", [1, 2, 3, 4, 7, 1, 2, 3, 4], 2, (1, 2), [7, 1], 2),
    ("m capped: the later of two capped matches", [3, 4, 6, 2, 3, 4, 7, 9, 3, 4], 2, (1, 2), [7, 9], 2),
    ("nmin=2 rejects a 1-gram", [5, 1, 2, 5], 3, (2, 3), [5, 5, 5], 0),
    ("nmin=2 takes a 2-gram", [4, 5, 1, 4, 5], 3, (2, 3), [1, 4, 5], 2),
    ("period 1", [9, 4, 4], 7, (1, 3), [4] * 7, 1),
    ("period 2", [1, 2, 1, 2], 7, (1, 3), [1, 2, 1, 2, 1, 2, 1], 2),
    ("period 3", [1, 2, 3, 1, 2, 3], 7, (1, 3), [1, 2, 3, 1, 2, 3, 1], 3),
    ("no match", [1, 2, 3, 4, 5], 4, (1, 3), [5] * 4, 0),
]


def hist_matrix(rows, ld, fill=0):
    """int32 [len(rows), ld] holding each history at the front; the lengths."""
    h = np.full((len(rows), ld), fill, dtype=np.int32)
    for i, r in enumerate(rows):
        h[i, :len(r)] = r
    return h, np.array([len(r) for r in rows], dtype=np.int32)


def random_state(n_seq, L, k, vocab, max_seq, ld, seed):
    """A random draft / accept state: histories over ``vocab`` (odd sequences get a planted repeat of
    their tail so that long matches exist over a large vocabulary too), lengths ``L - (s % 3)``
    (at least 1), cells beyond the length filled with a sentinel, a script, limits within reach of
    one step, a few finished sequences and EOS ids drawn from the vocabulary's low end."""
    rng = np.random.default_rng(seed)
    hist = rng.integers(0, vocab, (n_seq, ld), dtype=np.int64).astype(np.int32)
    hlen = np.array([max(1, L - (s % 3)) for s in range(n_seq)], dtype=np.int32)
    for s in range(1, n_seq, 2):
        n = int(hlen[s])
        w = int(rng.integers(1, 10))
        if n > 2 * w + 2:
            p = int(rng.integers(0, n - 2 * w - 1))
            hist[s, n - w:n] = hist[s, p:p + w]
    for s in range(n_seq):
        hist[s, hlen[s]:] = -5 - s
    script = rng.integers(0, vocab, (n_seq, ld), dtype=np.int64).astype(np.int32)
    limit = (hlen + rng.integers(1, k + 3, n_seq)).astype(np.int32)
    done = (rng.random(n_seq) < 0.2).astype(np.int32)
    eos = np.full(8, -1, dtype=np.int32)
    eos[:3] = rng.integers(0, min(vocab, 6), 3)
    return {"hist": hist, "hlen": hlen, "script": script, "limit": limit, "done": done, "eos": eos,
            "max_seq": max_seq, "k": k}


def random_cand(tokens, n_seq, k, vocab, seed):
    """The model's tokens for a step fed ``tokens``: sequence s agrees with its first ``s % (k + 2)``
    drafts (all of them and a bonus token when that reaches k), the rest is random."""
    rng = np.random.default_rng(seed)
    cand = rng.integers(0, vocab, n_seq * (k + 1), dtype=np.int64).astype(np.int32)
    for s in range(n_seq):
        r0, a = s * (k + 1), min(k, s % (k + 2))
        cand[r0:r0 + a] = tokens[r0 + 1:r0 + 1 + a]
        if a < k and cand[r0 + a] == tokens[r0 + a + 1]:
            cand[r0 + a] = (cand[r0 + a] + 1) % vocab
    return cand


def prompt(cfg, seed, n_random=12, n_repeat=7):
    """``n_random`` random tokens followed by the first ``n_repeat`` of them again."""
    g = torch.Generator().manual_seed(seed)
    p = torch.randint(3, cfg.vocab_size, (n_random,), generator=g).tolist()
    return p + p[:n_repeat]


def corrupt(script, n_prompt, vocab, every=3):
    """``script`` with every ``every``-th generated position (0, every, ..) replaced by (t + 1) % V."""
    out = list(script)
    for i in range(n_prompt, len(out), every):
        out[i] = (out[i] + 1) % vocab
    return out
