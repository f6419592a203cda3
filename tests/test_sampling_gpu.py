"""Seeded temperature / top-k / top-p sampling on the device (csrc/sampling/sampling.hip):
the noise against the numpy Philox, the kernel against the fp64 reference on the shared cases
(tests/sampling_cases.py: thresholds and kept counts exactly, tokens wherever the reference's
two best scores are >= 1e-3 apart), determinism and placement independence, the drawn
distribution, the captured SamplingDecodeGraph, the logits of the fp8 and GPT-2 heads and the
graph-mode server's switch to sampling graphs."""
import numpy as np
import pytest
import torch

import sampling_cases as C
from llm_sharding_amd.config import LlamaConfig, tiny, tiny_gpt2
from llm_sharding_amd.ops import sampling as S
from llm_sharding_amd.runtime.engine import RandomSource, StageEngine
from llm_sharding_amd.runtime.sampling import Sampler, SamplingDecodeGraph, SamplingParams
from llm_sharding_amd.utils.numerics import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev_args(c, rows=None):
    sl = slice(None) if rows is None else rows
    return (torch.from_numpy(c.T[sl].copy()).to(DEV), torch.from_numpy(c.top_k[sl].copy()).to(DEV),
            torch.from_numpy(c.top_p[sl].copy()).to(DEV), torch.from_numpy(c.seed[sl].copy().view(np.int64)).to(DEV),
            torch.from_numpy(c.ctr[sl].copy()).to(DEV))


def _launch(logits, V, T, k, p, seed, ctr, dbg=True):
    """lsa_sample + argmax_finalize -> (tokens int64 numpy, dbg int32 numpy [rows, 2])."""
    from llm_sharding_amd.ops import hip
    rows = T.numel()
    keys = torch.zeros(rows, dtype=torch.int64, device=DEV)
    d = torch.full((rows, 2), -1, dtype=torch.int32, device=DEV) if dbg else None
    S.sample(logits, V, rows, T, k, p, seed, ctr, keys, dbg=d)
    tok = torch.empty(rows, dtype=torch.int32, device=DEV)
    hip.argmax_finalize(keys, rows, tok)
    return tok.cpu().numpy().astype(np.int64), (d.cpu().numpy() if dbg else None)


# ------------------------------------------------------------------------------ noise
def test_noise_bits_and_gumbel():
    seed, ctr, n = 0xC0FFEE1234567890, 1234, 50257
    bits, g = S.sample_noise(seed, ctr, 0, n, DEV)
    want = S.noise_bits(seed, ctr, np.arange(n))
    got = bits.cpu().numpy().view(np.uint32)
    assert (got == want).all()
    err = np.abs(g.cpu().numpy().astype(np.float64) - S.gumbel_from_bits(want)).max()
    print(f"max |g - g_ref64| over {n} indices: {err:.2e}")
    assert err <= 1e-5
    # a range that does not start at a Philox block boundary
    bits2, _ = S.sample_noise(seed, ctr, 4093, 37, DEV)
    assert (bits2.cpu().numpy().view(np.uint32) == want[4093:4093 + 37]).all()
    # forced words, the two extremes x >> 9 == 0 and == 2^23 - 1 among them
    forced = np.array([0, 0x1FF, 0x200, 0xFFFFFE00, 0xFFFFFFFF, 0x80000000, 0x7FFFFFFF, 12345 << 9], dtype=np.uint32)
    fb, fg = S.sample_noise(0, 0, 0, forced.size, DEV, bits_in=torch.from_numpy(forced.view(np.int32)).to(DEV))
    assert (fb.cpu().numpy().view(np.uint32) == forced).all()
    ferr = np.abs(fg.cpu().numpy().astype(np.float64) - S.gumbel_from_bits(forced)).max()
    print(f"max |g - g_ref64| on the forced words: {ferr:.2e}")
    assert ferr <= 1e-5 and np.isfinite(fg.cpu().numpy()).all()


# ------------------------------------------------------------------------------ kernel vs reference
@pytest.mark.parametrize("case", C.KERNEL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_kernel_matches_reference(case):
    rows, V, ld = case
    c = C.make_case(*case)
    ref_tok, kept, gap, _ = C.reference(*case)
    thr, cnt = C.expected_dbg(*case)
    if ld > V:  # poisoned padding: it would win every row if it were read
        assert bool((c.logits[:, V:].float().min(dim=1).values > c.logits[:, :V].float().max(dim=1).values).all())
    tok, dbg = _launch(c.logits.to(DEV), V, *_dev_args(c))
    assert (tok >= 0).all() and (tok < V).all()
    assert (dbg[:, 0] == thr).all(), f"threshold keys differ on rows {np.nonzero(dbg[:, 0] != thr)[0][:8]}"
    assert (dbg[:, 1] == cnt).all(), f"kept counts differ on rows {np.nonzero(dbg[:, 1] != cnt)[0][:8]}"
    assert kept[np.arange(rows), tok].all(), "a token outside the reference kept set"
    sampled = c.T > 0
    must = sampled & (gap >= C.GAP_MIN)
    print(f"{case}: {int(must.sum())} of {int(sampled.sum())} sampled rows compared, "
          f"{int((tok[sampled] == ref_tok[sampled]).sum())} equal")
    assert (tok[must] == ref_tok[must]).all(), f"tokens differ on rows {np.nonzero(must & (tok != ref_tok))[0][:8]}"
    # greedy rows: the lowest-index maximum, whatever the gap
    assert (tok[~sampled] == ref_tok[~sampled]).all()


def test_unaligned_rows_take_the_scalar_path():
    """ld not a multiple of 8: rows do not start 16-byte aligned."""
    c = C.make_case(5, 32000, 32000)
    ref_tok, kept, gap, _ = C.reference(5, 32000, 32000)
    V, ld = 32000, 32003
    lg = torch.zeros((5, ld), dtype=torch.bfloat16)
    lg[:, :V] = c.logits
    lg[:, V:] = 100.0
    tok, dbg = _launch(lg.to(DEV), V, *_dev_args(c))
    thr, cnt = C.expected_dbg(5, 32000, 32000)
    assert (dbg[:, 0] == thr).all() and (dbg[:, 1] == cnt).all()
    ok = (gap >= C.GAP_MIN) | (c.T == 0)
    assert (tok[ok] == ref_tok[ok]).all() and kept[np.arange(5), tok].all()


# ------------------------------------------------------------------------------ determinism, placement
def test_determinism_and_placement():
    case = (129, 50257, 50304)
    rows, V, ld = case
    c = C.make_case(*case)
    lg = c.logits.to(DEV)
    args = _dev_args(c)
    t0, _ = _launch(lg, V, *args)
    for _ in range(2):
        t, _ = _launch(lg, V, *args)
        assert (t == t0).all()
    perm = np.random.default_rng(5).permutation(rows)
    pt = torch.from_numpy(perm).to(DEV)
    tp, _ = _launch(lg[pt].contiguous(), V, *(a[pt].contiguous() for a in args))
    assert (tp == t0[perm]).all()
    # a row alone gives the token it gives inside the batch
    for r in [int(np.nonzero((c.T > 0) & (c.top_p < 1))[0][0]), int(np.nonzero(c.T == 0)[0][0]), rows - 1]:
        t1, _ = _launch(lg[r:r + 1], V, *(a[r:r + 1].contiguous() for a in args))
        assert t1[0] == t0[r], f"row {r}: {t1[0]} alone, {t0[r]} in the batch"


# ------------------------------------------------------------------------------ distribution
def test_device_draws_follow_the_kept_distribution():
    from scipy.stats import chi2
    lg, p, kept, probs = C.gof_case()
    seeds, ctrs = C.gof_seeds()
    rows = 1024
    full = torch.empty((rows, 1024), dtype=torch.bfloat16)
    full[:, :C.GOF_V] = lg
    full[:, C.GOF_V:] = 100.0
    full = full.to(DEV)
    T = torch.full((rows,), C.GOF_T, dtype=torch.float32, device=DEV)
    k = torch.full((rows,), C.GOF_K, dtype=torch.int32, device=DEV)
    pp = torch.full((rows,), p, dtype=torch.float32, device=DEV)
    toks = []
    for i in range(C.GOF_DRAWS // rows):
        sl = slice(i * rows, (i + 1) * rows)
        t, _ = _launch(full, C.GOF_V, T, k, pp, torch.from_numpy(seeds[sl].copy().view(np.int64)).to(DEV),
                       torch.from_numpy(ctrs[sl].copy()).to(DEV), dbg=False)
        toks.append(t)
    stat, dof, outside, min_exp = C.chi2_stat(np.concatenate(toks), kept, probs)
    print(f"kept {kept.sum()}, smallest expected count {min_exp:.1f}, chi2 {stat:.1f} at {dof} dof, "
          f"critical {chi2.ppf(1 - 1e-6, dof):.1f}")
    assert outside == 0
    assert stat < chi2.ppf(1 - 1e-6, dof)


# ------------------------------------------------------------------------------ graph
def _graph_run(eng, prompts, params, late, steps=6):
    """Prefill ``prompts`` into slots 0.., sample the first tokens, capture a "full"
    SamplingDecodeGraph and replay ``steps`` times (``late`` = (step, row, params) applied
    between replays). Returns (first tokens, history, per-step (hidden, logits, params))."""
    rows = len(prompts)
    eng.reset()
    sl, po = eng.prefill_rows(list(range(rows)), [len(p) for p in prompts])
    h = eng.forward(eng.embed(torch.tensor([t for p in prompts for t in p], device=DEV)), sl, po)
    eng.advance(list(range(rows)), [len(p) for p in prompts])
    last = [int(i) for i in np.cumsum([len(p) for p in prompts]) - 1]
    first = Sampler(eng).sample(h, last, params, [len(p) for p in prompts])
    g = SamplingDecodeGraph(eng, rows, "full", history_len=steps)
    cur = list(params)
    for i, p in enumerate(cur):
        g.set_params(i, p)
    g.tokens.copy_(first.to(torch.int32))
    g.capture()
    pos0 = g.pos.clone()
    rec = []
    for s in range(steps):
        if late is not None and late[0] == s:
            g.set_params(late[1], late[2])
            cur[late[1]] = late[2]
        g.replay()
        torch.cuda.synchronize()
        rec.append((g.out_hidden.clone(), g.logits.clone(), list(cur)))
    assert torch.equal(g.pos, pos0 + steps)
    return first.cpu(), g.history.clone().cpu(), rec, pos0.cpu().tolist()


def test_sampling_decode_graph():
    cfg = LlamaConfig(num_hidden_layers=2, vocab_size=32000, max_position_embeddings=512, name="Llama-2-7B-2L")
    eng = StageEngine(cfg, 0, 2, DEV, torch.bfloat16, has_embed=True, has_head=True, source=RandomSource(cfg, 0),
                      max_slots=4, max_seq=128, max_prefill_rows=64)
    g = torch.Generator().manual_seed(3)
    prompts = [torch.randint(3, cfg.vocab_size, (n,), generator=g).tolist() for n in (5, 9, 3, 7)]
    params = [SamplingParams(0.7, top_p=0.9, seed=11), SamplingParams(1.0, top_k=50, seed=12),
              SamplingParams(0.0), SamplingParams(1.3, top_k=5000, top_p=0.95, seed=14)]
    late = (3, 0, SamplingParams(1.0, top_k=1, seed=11))  # from replay 3 on, row 0 keeps only the maximum
    first, hist, rec, pos0 = _graph_run(eng, prompts, params, late)
    V, smp = cfg.vocab_size, Sampler(eng)
    assert pos0 == [len(p) for p in prompts]
    n_cmp = 0
    for s, (h, lg, cur) in enumerate(rec):
        ctr = [p + s + 1 for p in pos0]  # the position the step's token occupies
        args = ([p.temperature for p in cur], [p.top_k for p in cur], [p.top_p for p in cur], [p.seed for p in cur], ctr)
        ref_tok, kept, gap, _ = S.sample_reference(lg.cpu(), V, *args)
        tok = hist[s].numpy().astype(np.int64)
        assert kept[np.arange(4), tok].all(), f"replay {s}: a token outside the kept set"
        must = (gap >= C.GAP_MIN) & np.array([not p.greedy for p in cur])
        assert (tok[must] == ref_tok[must]).all(), f"replay {s}: graph {tok} reference {ref_tok}"
        eager = smp.sample(h, None, cur, ctr).cpu().numpy()          # the eager Sampler on the same states
        assert (eager[must] == tok[must]).all() and (eager[must] == ref_tok[must]).all()
        n_cmp += int(must.sum())
        row_max = lg[:, :V].float().max(dim=1).values.cpu()
        assert lg[2, tok[2]].float().cpu() == row_max[2]               # the greedy row attains its maximum
        if s >= late[0]:
            assert lg[0, tok[0]].float().cpu() == row_max[0]           # set_params took effect
    assert n_cmp >= 12
    # the same seeds reproduce the run bitwise
    first2, hist2, _, _ = _graph_run(eng, prompts, params, late)
    assert torch.equal(first, first2) and torch.equal(hist, hist2)


# ------------------------------------------------------------------------------ fp8 / GPT-2 heads
class _CpuGen(RandomSource):
    """Random weights drawn on the CPU in bf16, then moved / cast: the GPU engine and the fp32
    CPU engine see identical values."""

    def layer(self, i, device, dtype):
        return {k: v.to(device, dtype) for k, v in super().layer(i, "cpu", torch.bfloat16).items()}

    def embedding(self, device, dtype):
        return super().embedding("cpu", torch.bfloat16).to(device, dtype)

    def final_norm(self, device, dtype):
        return super().final_norm("cpu", torch.bfloat16).to(device, dtype)

    def lm_head(self, device, dtype):
        return super().lm_head("cpu", torch.bfloat16).to(device, dtype)

    def pos_embedding(self, device, dtype):
        t = super().pos_embedding("cpu", torch.bfloat16)
        return None if t is None else t.to(device, dtype)

    def final_norm_bias(self, device, dtype):
        t = super().final_norm_bias("cpu", torch.bfloat16)
        return None if t is None else t.to(device, dtype)


def _logits_pair(cfg, weight_dtype, rows_idx, n_rows=9):
    src = _CpuGen(cfg, 4)
    kw = dict(has_embed=True, has_head=True, source=src, max_slots=2, max_seq=64, max_prefill_rows=64)
    eg = StageEngine(cfg, 0, cfg.num_hidden_layers, DEV, torch.bfloat16, weight_dtype=weight_dtype, **kw)
    ec = StageEngine(cfg, 0, cfg.num_hidden_layers, "cpu", torch.float32, **kw)
    h = torch.randn((n_rows, cfg.hidden_size), generator=torch.Generator().manual_seed(2)).to(torch.bfloat16)
    got = Sampler(eg).logits(h.to(DEV), rows_idx)
    want = ec.logits_torch(h.float()[rows_idx])
    assert got.dtype == torch.bfloat16 and got.shape == (len(rows_idx), cfg.head_rows)
    V = cfg.vocab_size
    return eg, got[:, :V].float().cpu(), want[:, :V]


def test_fp8_head_logits():
    """e4m3 weights round with a relative error uniform in +-2^-4 (rms 3.6 %), independent per
    weight, so a logit - a sum of independently perturbed terms - is off by about 3.6 % of the
    terms' root-sum-square: the bound is about twice that."""
    cfg = tiny(layers=1, hidden=1024, heads=8, kv_heads=8, head_dim=128, inter=2048, vocab=4096)
    eg, got, want = _logits_pair(cfg, "fp8", [7, 0, 3, 3, 8])
    assert eg.lm_head_s is not None
    e = rel_err(got, want)
    print(f"fp8 head logits: rel err {float(e):.3e}")
    assert e < 0.08


def test_gpt2_head_logits_and_sampling():
    """LayerNorm + biased (padding-masked) head: bf16 activations and outputs against fp32."""
    cfg = tiny_gpt2(layers=1)
    rows_idx = [4, 1, 1, 6]
    eg, got, want = _logits_pair(cfg, "bf16", rows_idx)
    e = rel_err(got, want)
    print(f"GPT-2 head logits: rel err {float(e):.3e}")
    assert e < 2e-2
    # the padded vocabulary (500 of 512 columns) is never sampled
    h = torch.randn((9, cfg.hidden_size), generator=torch.Generator().manual_seed(2)).to(torch.bfloat16).to(DEV)
    tok = Sampler(eg).sample(h, list(range(9)) * 8, [SamplingParams(5.0, seed=s) for s in range(72)], [3] * 72)
    assert int(tok.max()) < cfg.vocab_size and len(set(tok.tolist())) > 20


# ------------------------------------------------------------------------------ server
def _gpu_server(cfg):
    from llm_sharding_amd.parallel.server import PipelineServer
    return PipelineServer(cfg, RandomSource(cfg, 11), 0, 1, 0, cfg.num_hidden_layers, device=DEV, batch=2,
                          microbatches=2, max_seq=128, prefill_budget=16)


def test_server_switches_to_sampling_graphs():
    """Graph-mode server: greedy until the first non-greedy request is admitted (here while other
    requests are decoding), then SamplingDecodeGraphs that take over positions and tokens; the
    run is reproducible from its seeds and another seed changes only the sampled requests."""
    from llm_sharding_amd.runtime.engine import DecodeGraph
    cfg = tiny(layers=2)
    g = torch.Generator().manual_seed(5)
    prompts = [torch.randint(3, cfg.vocab_size, (n,), generator=g).tolist() for n in (3, 9, 20, 1, 17, 6)]

    def run(seed0):
        srv = _gpu_server(cfg)
        assert not srv.sampling_on and all(type(x) is DecodeGraph for x in srv.graphs)
        params = [None, None, None, None, SamplingParams(0.9, top_k=40, top_p=0.95, seed=seed0),
                  SamplingParams(1.2, seed=seed0 + 1)]
        rids = [srv.submit(p, 8, eos_ids=(), sampling=sp) for p, sp in zip(prompts, params)]
        srv.serve(stop_when_idle=True)
        assert srv.sampling_on and all(isinstance(x, SamplingDecodeGraph) for x in srv.graphs)
        return [srv.requests[r].output_ids for r in rids]

    a, b, c = run(50), run(50), run(60)
    assert a == b
    assert all(len(o) == 8 and max(o) < cfg.vocab_size for o in a)
    assert a[4] != c[4] or a[5] != c[5]
    # an all-greedy server never builds the sampling path
    srv = _gpu_server(cfg)
    srv.generate(prompts[:3], 4, eos_ids=())
    assert not srv.sampling_on and srv.sampler is None and all(type(x) is DecodeGraph for x in srv.graphs)
    # the switch carries the device state of requests in flight over, rows start greedy
    srv.graphs[1].pos.copy_(torch.tensor([7, 19], dtype=torch.int32))
    srv.graphs[1].tokens.copy_(torch.tensor([33, 44], dtype=torch.int32))
    srv._enable_sampling()
    assert srv.graphs[1].pos.tolist() == [7, 19] and srv.graphs[1].tokens.tolist() == [33, 44]
    assert srv.graphs[0].pos.tolist() == [0, 0] and float(srv.graphs[1].temperature.abs().max()) == 0.0
