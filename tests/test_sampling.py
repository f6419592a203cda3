"""Seeded temperature / top-k / top-p sampling, CPU side: the Philox known answers, the fp64
reference against transformers' logits warpers and against its own distribution, the
preconditions of the GPU cases (tests/sampling_cases.py), SamplingParams, the CPU engine, the
continuous-batching server and the request / command-line plumbing."""
import numpy as np
import pytest
import torch

import sampling_cases as C
from llm_sharding_amd.config import tiny
from llm_sharding_amd.ops import sampling as S
from llm_sharding_amd.parallel.scheduler import plan_stages
from llm_sharding_amd.parallel.server import PipelineServer
from llm_sharding_amd.runtime.engine import RandomSource, StageEngine
from llm_sharding_amd.runtime.sampling import (EagerSamplingDecode, Sampler, SamplingParams)


# ------------------------------------------------------------------------------ Philox / noise
@pytest.mark.parametrize("ctr, key, want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(ctr, key, want):
    got = S.philox4x32_10(ctr, key)
    assert " ".join(f"{int(x):08x}" for x in got) == want


def test_noise_is_a_function_of_seed_position_and_index():
    seed, ctr = 0x0123456789ABCDEF, 77
    all_ = S.noise_bits(seed, ctr, np.arange(64))
    some = S.noise_bits(seed, ctr, np.array([63, 5, 6, 40]))
    assert (some == all_[[63, 5, 6, 40]]).all()
    blk = S.philox4x32_10((1, ctr, 0, 0), (0x89ABCDEF, 0x01234567))
    assert (all_[4:8] == blk).all()
    assert (S.noise_bits(seed, ctr + 1, np.arange(64)) != all_).any()
    g = S.gumbel_from_bits(np.array([0, 0xFFFFFFFF], dtype=np.uint32))
    assert np.allclose(g, [-np.log(-np.log(2.0 ** -24)), -np.log(-np.log1p(-2.0 ** -24))], rtol=1e-12)


# ------------------------------------------------------------------------------ kept sets vs HF
def test_kept_sets_equal_hf_warpers():
    from transformers import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    V, rows = 1000, 18
    rng = np.random.default_rng(99)
    l32 = (2.5 * rng.standard_normal((rows, V))).astype(np.float32)  # fp32, not bf16-rounded: tie-free
    l64 = l32.astype(np.float64)
    ks = C.top_ks(V)
    checked = 0
    for r in range(rows):
        assert np.unique(l32[r]).size == V
        T, k = C.TEMPS[r % 3], ks[(r // 3) % len(ks)]
        p = 1.0 if r % 5 == 0 else C.data_top_p(l64[r], T, k, "first" if r % 5 == 1 else "any", rng)
        _, kept, _, pm = S.sample_reference(l32[r:r + 1], V, T, k, p, 1, 1)
        assert pm[0] >= C.P_MARGIN
        sc = torch.from_numpy(l32[r:r + 1].copy())
        sc = TemperatureLogitsWarper(float(np.float32(T)))(None, sc)
        if k > 0:
            sc = TopKLogitsWarper(top_k=int(k))(None, sc)
        if p < 1.0:
            sc = TopPLogitsWarper(top_p=float(p))(None, sc)
        hf = torch.isfinite(sc)[0].numpy()
        assert (hf == kept[0]).all(), f"row {r}: T={T} k={k} p={p}: HF keeps {hf.sum()}, reference {kept[0].sum()}"
        checked += int(p < 1.0)
    assert checked >= rows // 2


# ------------------------------------------------------------------------------ goodness of fit
def test_reference_draws_follow_the_kept_distribution():
    from scipy.stats import chi2
    lg, p, kept, probs = C.gof_case()
    seeds, ctrs = C.gof_seeds()
    n = seeds.size
    tok, _, _, _ = S.sample_reference(lg.expand(n, -1), C.GOF_V, C.GOF_T, C.GOF_K, p, [int(s) for s in seeds], ctrs)
    stat, dof, outside, min_exp = C.chi2_stat(tok, kept, probs)
    print(f"kept {kept.sum()}, smallest expected count {min_exp:.1f}, chi2 {stat:.1f} at {dof} dof, "
          f"critical {chi2.ppf(1 - 1e-6, dof):.1f}")
    assert outside == 0
    assert min_exp >= 5
    assert stat < chi2.ppf(1 - 1e-6, dof)


# ------------------------------------------------------------------------------ GPU-case preconditions
def test_gpu_case_preconditions():
    n_rows = n_close = 0
    for case in C.KERNEL_CASES:
        c = C.make_case(*case)
        tok, kept, gap, pm = C.reference(*case)
        assert pm.min() >= C.P_MARGIN, f"{case}: top-p margin {pm.min():.2e}"
        sampled = c.T > 0
        n_rows += int(sampled.sum())
        n_close += int((gap[sampled] < C.GAP_MIN).sum())
        assert kept[np.arange(c.rows), tok].all()
        if c.rows >= 6:  # every path is present
            assert (c.T == 0).any() and (c.top_p == 1).any() and (c.top_p < 1).sum() >= c.rows // 3
            assert set(C.top_ks(c.V)) == set(int(k) for k in c.top_k)
            assert (kept.sum(axis=1)[sampled] == 1).any() and (kept.sum(axis=1) == c.V).any()
    print(f"{n_close} of {n_rows} sampled rows have a top-two gap below {C.GAP_MIN}")
    assert n_close <= C.GAP_ROWS_MAX * n_rows


def test_reference_contract_details():
    V = 16
    l = torch.tensor([[0.0, 3.0, 3.0, 1.0, -2.0, 2.0, 2.0, 2.0, 0.5, 0.5, -1.0, -1.0, 0.0, 0.0, 0.0, 9.0]],
                     dtype=torch.bfloat16)
    # columns >= V are never candidates; greedy takes the lowest index on ties
    tok, kept, _, _ = S.sample_reference(l, V - 1, 0.0, 0, 1.0, 1, 1)
    assert tok[0] == 1 and kept.sum() == 1
    # top-k keeps every tie at the threshold: the 3rd largest of the first 15 is a 2.0 (x3)
    _, kept, _, _ = S.sample_reference(l, V - 1, 1.0, 3, 1.0, 1, 1)
    assert sorted(np.nonzero(kept[0])[0]) == [1, 2, 5, 6, 7]
    # top-p cuts by value-groups: the two 3.0 hold 2 e^3 / Z of the mass
    z = l[0, :V - 1].double().numpy()
    m = np.exp(z) / np.exp(z).sum()
    top = m[1] + m[2]
    _, kept, _, pm = S.sample_reference(l, V - 1, 1.0, 0, top - 0.01, 1, 1)
    assert sorted(np.nonzero(kept[0])[0]) == [1, 2] and abs(pm[0] - 0.01) < 1e-6
    _, kept, _, _ = S.sample_reference(l, V - 1, 1.0, 0, top + 0.01, 1, 1)
    assert sorted(np.nonzero(kept[0])[0]) == [1, 2, 5, 6, 7]
    # 64-bit seeds on both sides of 2^63 in one call are taken exactly (no float round trip)
    seeds = [8915428126640357772, 13432243115640325029, (1 << 64) - 1]
    lg = torch.randn((3, 64), generator=torch.Generator().manual_seed(1)).to(torch.bfloat16)
    tok, _, _, _ = S.sample_reference(lg, 64, 1.0, 0, 1.0, seeds, [5, 6, 7])
    for r in range(3):
        one, _, _, _ = S.sample_reference(lg[r:r + 1], 64, 1.0, 0, 1.0, seeds[r], 5 + r)
        z = lg[r].double().numpy() + S.gumbel_from_bits(S.noise_bits(seeds[r], 5 + r, np.arange(64)))
        assert tok[r] == one[0] == int(z.argmax())
    # k >= V and p == 1: nothing filtered
    _, kept, _, _ = S.sample_reference(l, V, 1.0, V + 5, 1.0, 1, 1)
    assert kept.all()


# ------------------------------------------------------------------------------ SamplingParams
def test_sampling_params_validation():
    assert SamplingParams().greedy and SamplingParams(seed=5).seed == 5
    a, b = SamplingParams(0.7), SamplingParams(0.7)
    assert 0 <= a.seed < 1 << 64 and a.seed != b.seed  # drawn and stored
    assert SamplingParams(0.7, seed=a.seed) == a
    for bad in (dict(temperature=-0.1), dict(temperature=float("nan")), dict(top_k=-1), dict(top_p=0.0),
                dict(top_p=1.5), dict(seed=-1), dict(seed=1 << 64)):
        with pytest.raises(ValueError):
            SamplingParams(**bad)
    assert SamplingParams.from_dict({"text": "x"}) is None
    sp = SamplingParams.from_dict({"temperature": 0.6, "top_p": 0.9, "seed": 3, "top_k": None})
    assert (sp.temperature, sp.top_k, sp.top_p, sp.seed) == (0.6, 0, 0.9, 3)


# ------------------------------------------------------------------------------ CPU engine
SEED = 11


def _engine(cfg, slots=4, **kw):
    return StageEngine(cfg, 0, cfg.num_hidden_layers, "cpu", torch.float32, has_embed=True, has_head=True,
                       source=RandomSource(cfg, SEED), max_slots=slots, max_seq=128, **kw)


def _prefill(eng, prompts):
    slots = list(range(len(prompts)))
    slot, pos = eng.prefill_rows(slots, [len(p) for p in prompts])
    h = eng.forward(eng.embed(torch.tensor([t for p in prompts for t in p])), slot, pos)
    eng.advance(slots, [len(p) for p in prompts])
    last = list(np.cumsum([len(p) for p in prompts]) - 1)
    return h, [int(i) for i in last]


def _prompts(cfg, lens=(5, 9, 3, 12)):
    g = torch.Generator().manual_seed(5)
    return [torch.randint(3, cfg.vocab_size, (n,), generator=g).tolist() for n in lens]


def test_cpu_engine_greedy_limits_and_seeds():
    cfg = tiny(layers=2)
    eng = _engine(cfg)
    prompts = _prompts(cfg)
    h, last = _prefill(eng, prompts)
    smp = Sampler(eng)
    pos = [len(p) for p in prompts]
    greedy = eng.head(h, last).tolist()
    assert smp.sample(h, last, [SamplingParams(0.0, seed=1)] * 4, pos).tolist() == greedy
    assert smp.sample(h, last, [SamplingParams(0.9, top_k=1, seed=s) for s in range(4)], pos).tolist() == greedy
    lg = smp.logits(h, last)
    assert lg.dtype == torch.bfloat16 and lg.shape == (4, cfg.head_rows)
    ps = [SamplingParams(1.0, top_k=50, top_p=0.95, seed=100 + i) for i in range(4)]
    a = smp.sample(h, last, ps, pos)
    assert a.tolist() == smp.sample(h, last, ps, pos).tolist()
    # many seeds on one row: not all the same token, and every token valid
    many = smp.sample(h, [last[0]] * 32, [SamplingParams(1.0, seed=s) for s in range(32)], [pos[0]] * 32)
    assert len(set(many.tolist())) > 1 and int(many.max()) < cfg.vocab_size
    # the position is part of the noise
    other = smp.sample(h, [last[0]] * 32, [SamplingParams(1.0, seed=s) for s in range(32)], [pos[0] + 1] * 32)
    assert many.tolist() != other.tolist()


def test_eager_twin_replays_from_the_seed():
    cfg = tiny(layers=2)
    outs = []
    for seed in (7, 7, 8):
        eng = _engine(cfg, slots=2)
        prompts = _prompts(cfg, (6, 4))
        h, last = _prefill(eng, prompts)
        ps = [SamplingParams(1.0, top_p=0.95, seed=seed), SamplingParams(0.0)]
        first = Sampler(eng).sample(h, last, ps, [len(p) for p in prompts])
        g = EagerSamplingDecode(eng, 2, "full", history_len=6)
        for i, p in enumerate(ps):
            g.set_params(i, p)
        g.tokens.copy_(first.to(torch.int32))
        for _ in range(6):
            g.replay()
        outs.append(g.history.clone())
        assert eng.seq_len[:2] == [12, 10]
    assert torch.equal(outs[0], outs[1])
    assert not torch.equal(outs[0][:, 0], outs[2][:, 0])       # another seed diverges
    assert torch.equal(outs[0][:, 1], outs[2][:, 1])           # the greedy row does not care
    with pytest.raises(ValueError):
        EagerSamplingDecode(_engine(cfg), 1, "first")


def test_split_head_is_rejected():
    cfg = tiny(layers=2)
    eng = _engine(cfg, head_cols=(0, cfg.head_rows // 2))
    with pytest.raises(NotImplementedError, match="split head"):
        Sampler(eng)


# ------------------------------------------------------------------------------ server
def _server(cfg, world=1, rank=0):
    st = plan_stages(cfg, world).stages[rank]
    return PipelineServer(cfg, RandomSource(cfg, SEED), rank, world, st.start, st.end, device="cpu", batch=2,
                          microbatches=2, max_seq=128, prefill_budget=16, dtype=torch.float32)


def _run(cfg, prompts, params, new=6):
    srv = _server(cfg)
    rids = [srv.submit(p, new, eos_ids=(), sampling=sp) for p, sp in zip(prompts, params)]
    srv.serve(stop_when_idle=True)
    return srv, [srv.requests[r].output_ids for r in rids]


def test_server_outputs_do_not_depend_on_placement():
    cfg = tiny(layers=2)
    prompts = _prompts(cfg, (3, 9, 40, 1, 17, 6))
    params = [SamplingParams(0.8, top_k=40, top_p=0.95, seed=50 + i) if i != 2 else None for i in range(len(prompts))]
    srv, together = _run(cfg, prompts, params)
    assert srv.sampling_on and srv.sampler is not None
    order = [4, 0, 5, 2, 1, 3]
    _, shuffled = _run(cfg, [prompts[i] for i in order], [params[i] for i in order])
    for j, i in enumerate(order):
        assert shuffled[j] == together[i], f"request {i} changed with its position in the queue"
    for i in (0, 3):
        _, alone = _run(cfg, [prompts[i]], [params[i]])
        assert alone[0] == together[i], f"request {i} alone differs from the same request among others"
    # the greedy request among them is the all-greedy server's
    g_srv, g_out = _run(cfg, prompts, [None] * len(prompts))
    assert g_out[2] == together[2]
    assert not g_srv.sampling_on and g_srv.sampler is None       # never built a sampling path
    assert any(a != b for a, b in zip(g_out, together))           # and sampling did sample
    # temperature 0 is greedy, and is not treated as a sampling request
    z_srv, z_out = _run(cfg, prompts[:2], [SamplingParams(0.0, top_k=5, seed=1)] * 2)
    assert z_out == g_out[:2] and not z_srv.sampling_on


def test_server_rejects_sampling_with_more_than_one_stage():
    cfg = tiny(layers=2)
    srv = _server(cfg, world=2)
    with pytest.raises(ValueError, match="single-stage"):
        srv.submit([3, 4, 5], 4, sampling=SamplingParams(0.7, seed=1))
    srv.submit([3, 4, 5], 4)                                      # greedy requests are still taken
    srv.submit([3, 4, 5], 4, sampling=SamplingParams(0.0))


# ------------------------------------------------------------------------------ plumbing
class _FakeServer:
    def __init__(self):
        self.calls = []

    def submit(self, ids, n_new, **kw):
        self.calls.append((list(ids), n_new, kw))
        return len(self.calls) - 1


class _FakeReplies:
    def __init__(self):
        self.errors = []

    def error(self, reply_to, reason, request_id=None):
        self.errors.append(reason)


def test_submit_message_sampling_keys():
    from llm_sharding_amd.parallel.ingress import submit_message
    srv, rep = _FakeServer(), _FakeReplies()
    assert submit_message(srv, {"input_ids": [3, 4]}, None, 8, rep) == 1
    assert "sampling" not in srv.calls[-1][2]                     # absent keys: the plain greedy call
    msg = {"input_ids": [[3, 4], [5]], "temperature": 0.7, "top_k": 20, "top_p": 0.9, "seed": 12, "max_new_tokens": 5}
    assert submit_message(srv, msg, None, 8, rep) == 2
    for ids, n_new, kw in srv.calls[-2:]:
        sp = kw["sampling"]
        assert n_new == 5 and (sp.temperature, sp.top_k, sp.top_p, sp.seed) == (0.7, 20, 0.9, 12)
    assert submit_message(srv, {"input_ids": [3], "temperature": 0.7}, None, 8, rep) == 1
    assert isinstance(srv.calls[-1][2]["sampling"].seed, int)     # a seed was drawn and stored
    assert submit_message(srv, {"input_ids": [3], "top_p": 2.0}, None, 8, rep) == 0
    assert rep.errors and "top_p" in rep.errors[-1]


def test_inference_cli_flags(capsys):
    import inference
    a = inference.build_parser().parse_args([])
    assert inference.sampling_from_args(a) is None                # the default stays greedy
    a = inference.build_parser().parse_args(["--temperature", "0.7", "--top-k", "40", "--top-p", "0.9", "--seed", "5"])
    sp = inference.sampling_from_args(a)
    assert (sp.temperature, sp.top_k, sp.top_p, sp.seed) == (0.7, 40, 0.9, 5)
    assert inference.sampling_from_args(inference.build_parser().parse_args(["--top-k", "5"])) is None  # T = 0
    with pytest.raises(SystemExit):
        inference.main(["--random", "tiny", "--temperature", "0.7", "--hf-compare", "x"])
    argv = ["--random", "tiny", "--device", "cpu", "--max-new-tokens", "5", "--prompt", "hello"]
    greedy = inference.main(argv)
    s1 = inference.main(argv + ["--temperature", "1.0", "--seed", "3"])
    s2 = inference.main(argv + ["--temperature", "1.0", "--seed", "3"])
    assert len(greedy) <= 5 and s1 == s2
    assert "seed 3" in capsys.readouterr().out
