"""Per-token log-probabilities, CPU side: the numpy reference against torch's fp64 log-softmax
and a stable sort, SamplingParams, the CPU-engine server against the reference on each step's
logits, the reply plumbing, score_prompt against transformers and ``inference.py --score``."""
import math

import numpy as np
import pytest
import torch

import logprob_cases as C
from llm_sharding_amd.config import LlamaConfig, tiny
from llm_sharding_amd.ops import logprobs as LP
from llm_sharding_amd.parallel.scheduler import plan_stages
from llm_sharding_amd.parallel.server import PipelineServer
from llm_sharding_amd.runtime.engine import RandomSource, StageEngine
from llm_sharding_amd.runtime.sampling import (EagerSamplingDecode, Sampler, SamplingParams, score_prompt)

SEED = 11


# ------------------------------------------------------------------------------ reference vs torch
def _torch_oracle(lg: torch.Tensor, n_top, target):
    """fp64 log-softmax + a stable sort by (-logit, index)."""
    rows, V = lg.shape
    x = lg.double()
    lp = torch.log_softmax(x, dim=-1)
    lse = torch.logsumexp(x, dim=-1)
    order = torch.sort(-x, dim=-1, stable=True).indices
    top_id = np.full((rows, LP.TOP_MAX), -1, dtype=np.int64)
    top_lp = np.full((rows, LP.TOP_MAX), -np.inf)
    tok_lp, rank = np.zeros(rows), np.zeros(rows, dtype=np.int64)
    for r in range(rows):
        n = min(n_top[r], LP.TOP_MAX, V)
        top_id[r, :n] = order[r, :n].numpy()
        top_lp[r, :n] = lp[r, order[r, :n]].numpy()
        tok_lp[r] = float(lp[r, target[r]])
        rank[r] = 1 + int((x[r] > x[r, target[r]]).sum())
    return LP.Logprobs(lse.numpy(), tok_lp, rank, top_id, top_lp)


@pytest.mark.parametrize("V", [1, 7, 4099])
def test_reference_equals_torch(V):
    lg, tg, kinds = C.every_kind(V)
    mixed, tg2, n_top2 = C.mixed_batch(12, V, 3)
    lg, tg = torch.cat([lg, mixed]), tg + tg2
    n_top = [20] * len(kinds) + n_top2
    ref = C.logprobs_reference(lg, V, n_top, tg)
    want = _torch_oracle(lg, n_top, tg)
    assert (ref.top_id == want.top_id).all() and (ref.tok_rank == want.tok_rank).all()
    for a, b in ((ref.lse, want.lse), (ref.tok_lp, want.tok_lp), (ref.top_lp, want.top_lp)):
        fin = np.isfinite(b)
        assert (a[~fin] == b[~fin]).all()
        assert np.abs(a[fin] - b[fin]).max(initial=0.0) <= 1e-12
    # the contract's edges: a skipped row, a target outside the vocabulary, columns >= V
    wide = torch.cat([lg, torch.full((lg.shape[0], 3), float("nan"), dtype=lg.dtype)], dim=1)
    r2 = C.logprobs_reference(wide, V, [-1] + n_top[1:], [tg[0], V] + tg[2:])
    assert np.isnan(r2.lse[0]) and r2.tok_rank[0] == 0 and (r2.top_id[0] == -1).all()
    assert np.isnan(r2.tok_lp[1]) and r2.tok_rank[1] == 0 and r2.lse[1] == ref.lse[1]
    assert (r2.top_id[2:] == ref.top_id[2:]).all() and (r2.lse[2:] == ref.lse[2:]).all()


def test_constant_and_near_constant_rows_go_by_index():
    V = 4099
    ref = C.logprobs_reference(torch.stack([C.constant_row(V), C.near_constant_row(V)]), V, 20, [V - 1, 0])
    assert ref.top_id[0].tolist() == list(range(20)) and ref.top_id[1].tolist() == list(range(1, 41, 2))
    assert ref.tok_rank.tolist() == [1, V // 2 + 1]
    assert abs(ref.tok_lp[0] + math.log(V)) < 1e-12


# ------------------------------------------------------------------------------ parameters
def test_sampling_params_logprobs():
    assert SamplingParams(seed=1).logprobs is None and SamplingParams(seed=1).plain
    for ok in (0, 1, 5, 20):
        sp = SamplingParams(seed=1, logprobs=ok)
        assert sp.logprobs == ok and sp.greedy and not sp.plain and not sp.penalized and sp.n_top == ok
    assert SamplingParams(seed=1).n_top == -1
    for bad in (-1, 21, 2.5, "3", True, float("nan")):
        with pytest.raises(ValueError, match="logprobs"):
            SamplingParams(seed=1, logprobs=bad)
    sp = SamplingParams.from_dict({"logprobs": 3, "seed": 9, "top_k": None})
    assert (sp.temperature, sp.logprobs, sp.seed) == (0.0, 3, 9)
    assert SamplingParams.from_dict({"logprobs": 0}).logprobs == 0
    assert SamplingParams.from_dict({"logprobs": None, "text": "x"}) is None
    assert SamplingParams.from_dict({"temperature": 0.5, "seed": 1}).logprobs is None
    with pytest.raises(ValueError):
        SamplingParams.from_dict({"logprobs": 21})


# ------------------------------------------------------------------------------ CPU server
def _engine(cfg, slots=1):
    return StageEngine(cfg, 0, cfg.num_hidden_layers, "cpu", torch.float32, has_embed=True, has_head=True,
                       source=RandomSource(cfg, SEED), max_slots=slots, max_seq=128)


def _server(cfg, world=1, rank=0, batch=2, microbatches=2):
    st = plan_stages(cfg, world).stages[rank]
    return PipelineServer(cfg, RandomSource(cfg, SEED), rank, world, st.start, st.end, device="cpu", batch=batch,
                          microbatches=microbatches, max_seq=128, prefill_budget=16, dtype=torch.float32)


def _prompts(cfg, lens):
    g = torch.Generator().manual_seed(5)
    return [torch.randint(3, cfg.vocab_size, (n,), generator=g).tolist() for n in lens]


@pytest.fixture
def sampled(monkeypatch):
    """Records every ``Sampler.sample_logits`` call: the bf16 logits the tokens were drawn from
    (after the penalties) and the rows' parameters. ``rows_of(sp)`` -> the logits rows of the
    request whose parameters are the object ``sp``, in step order."""
    calls, plain = [], Sampler.sample_logits

    def recording(self, logits, params_list, positions):
        calls.append((logits.clone(), list(params_list)))
        return plain(self, logits, params_list, positions)

    monkeypatch.setattr(Sampler, "sample_logits", recording)
    return lambda sp: torch.stack([lg[i] for lg, pl in calls for i, p in enumerate(pl) if p is sp])


def test_cpu_server_collects_logprobs(sampled):
    cfg = tiny(layers=2)
    prompts = _prompts(cfg, (7, 12, 5))
    srv = _server(cfg)
    params = [SamplingParams(0.0, logprobs=3), None, SamplingParams(0.8, top_k=40, seed=4, logprobs=0)]
    rids = [srv.submit(p, 8, eos_ids=(), sampling=sp) for p, sp in zip(prompts, params)]
    srv.serve(stop_when_idle=True)
    reqs = [srv.requests[r] for r in rids]
    assert srv.sampling_on and srv.logprobs_on
    r0, r1, r2 = reqs
    assert len(r0.output_ids) == len(r0.token_logprobs) == len(r0.ranks) == len(r0.top_logprobs) == 8
    assert r1.token_logprobs is None and r1.ranks is None and r1.top_logprobs is None
    assert len(r2.token_logprobs) == 8 and r2.top_logprobs is None
    for r, n in ((r0, 3), (r2, 0)):
        lg = sampled(r.sampling)      # one row per generated token: the step's own logits
        assert lg.shape[0] == 8
        ref = C.logprobs_reference(lg, cfg.vocab_size, n, r.output_ids)
        np.testing.assert_allclose(r.token_logprobs, ref.tok_lp, rtol=0, atol=2e-6)  # stored as fp32
        assert r.ranks == ref.tok_rank.tolist()
        if n:
            assert [[i for i, _ in t] for t in r.top_logprobs] == ref.top_id[:, :n].tolist()
            np.testing.assert_allclose([[v for _, v in t] for t in r.top_logprobs], ref.top_lp[:, :n], rtol=0,
                                       atol=2e-6)
    assert r0.ranks == [1] * 8 and all(t[0][0] == tok for t, tok in zip(r0.top_logprobs, r0.output_ids))
    # a server that never sees such a request builds none of it
    s2 = _server(cfg)
    s2.generate(prompts[:1], 4, eos_ids=())
    assert not s2.sampling_on and not s2.logprobs_on and s2.sampler is None


def test_replies_carry_logprobs_only_when_asked(monkeypatch):
    from llm_sharding_amd.parallel import ingress, protocol
    cfg = tiny(layers=2)
    prompts = _prompts(cfg, (6, 9))
    sent = []
    replies = ingress.Replies(None, verbose=False)
    monkeypatch.setattr(replies, "_send", lambda reply_to, payload: sent.append(protocol.decode(payload)))
    srv = _server(cfg)
    assert ingress.submit_message(srv, {"input_ids": prompts[0], "logprobs": 2, "reply_to": "a"}, None, 5, replies) == 1
    assert ingress.submit_message(srv, {"input_ids": prompts[1], "reply_to": "b"}, None, 5, replies) == 1
    bad = {"input_ids": prompts[1], "logprobs": 21, "reply_to": "c"}
    assert ingress.submit_message(srv, bad, None, 5, replies) == 0
    srv.serve(stop_when_idle=True)
    by_id = {m["request_id"]: m for m in sent if "error" not in m}
    assert set(by_id[1]) == {"request_id", "output_ids", "text", "ttft_ms", "tpot_ms"}     # today's reply
    lp = by_id[0]["logprobs"]
    assert set(by_id[0]) == set(by_id[1]) | {"logprobs"} and set(lp) == {"token_logprobs", "ranks", "top_logprobs"}
    assert len(lp["token_logprobs"]) == len(lp["ranks"]) == len(lp["top_logprobs"]) == 5
    assert all(len(t) == 2 and t[0][0] == tok for t, tok in zip(lp["top_logprobs"], by_id[0]["output_ids"]))
    assert any("error" in m and "logprobs" in m["error"] for m in sent)


def test_multi_stage_server_rejects_logprobs():
    srv = _server(tiny(layers=2), world=2)
    with pytest.raises(ValueError, match="single-stage"):
        srv.submit([3, 4, 5], 4, sampling=SamplingParams(0.0, logprobs=0))
    srv.submit([3, 4, 5], 4, sampling=SamplingParams(0.0, seed=1))


def test_eager_twin_keeps_the_lp_history(sampled):
    cfg = tiny(layers=2)
    prompt = _prompts(cfg, (7,))[0]
    eng = _engine(cfg, slots=2)
    sp = SamplingParams(0.9, seed=3, logprobs=4)
    slot, pos = eng.prefill_rows([1], [len(prompt)])
    h = eng.forward(eng.embed(torch.tensor(prompt)), slot, pos)
    eng.advance([1], [len(prompt)])
    first, lp0 = Sampler(eng).sample(h, [len(prompt) - 1], [sp], [len(prompt)], return_logprobs=True)
    g = EagerSamplingDecode(eng, 1, "full", slots=[1], history_len=5, logprobs=True)
    g.set_params(0, sp)
    g.tokens.copy_(first.to(torch.int32))
    for _ in range(5):
        g.replay()
    out = [int(first[0])] + g.history[:, 0].tolist()
    ref = C.logprobs_reference(sampled(sp), cfg.vocab_size, 4, out)
    got = [float(lp0.tok_lp[0])] + g.lp_history[:, 0].tolist()
    np.testing.assert_allclose(got, ref.tok_lp, rtol=0, atol=2e-6)
    assert g.lp.top_id[0, :4].tolist() == ref.top_id[-1, :4].tolist()
    with pytest.raises(RuntimeError, match="logprobs"):
        EagerSamplingDecode(eng, 1, "full", slots=[1]).set_params(0, sp)


def test_split_head_is_rejected():
    cfg = tiny(layers=2)
    eng = StageEngine(cfg, 0, cfg.num_hidden_layers, "cpu", torch.float32, has_embed=True, has_head=True,
                      source=RandomSource(cfg, SEED), max_slots=2, max_seq=128, head_cols=(0, cfg.head_rows // 2))
    with pytest.raises(NotImplementedError, match="split head"):
        score_prompt(eng, [3, 4, 5])


# ------------------------------------------------------------------------------ score_prompt vs transformers
@pytest.fixture(scope="module")
def hf(tmp_path_factory):
    pytest.importorskip("transformers")
    from test_llama_hf_parity import _hf_model
    from llm_sharding_amd.utils.model_sharder import ModelSharder
    tmp = tmp_path_factory.mktemp("lp_llama")
    m, d = _hf_model(tmp, "llama2")
    shards = ModelSharder(d, "llama", str(tmp / "shards"), dtype=torch.float32, verbose=False).save_shards()
    return m, shards


def test_score_prompt_against_transformers(hf, monkeypatch):
    """Per token |lp - hf| <= 2^-8 * max|logit of that row| + 1e-4: the CPU Sampler rounds the
    logits to bf16, which moves each by at most 2^-9 |l|, and a log-softmax moves by at most twice
    the largest logit perturbation."""
    from llm_sharding_amd.runtime.engine import ShardFolderSource
    import llm_sharding_amd.runtime.sampling as RS
    m, shards = hf
    cfg = LlamaConfig.from_pretrained(shards)
    eng = StageEngine(cfg, 0, cfg.num_hidden_layers, "cpu", torch.float32, has_embed=True, has_head=True,
                      source=ShardFolderSource(shards, cfg), max_slots=1, max_seq=64)
    ids = torch.randint(3, cfg.vocab_size - 1, (40,), generator=torch.Generator().manual_seed(6)).tolist()
    with torch.no_grad():
        logits = m(torch.tensor([ids])).logits[0, :-1].double()
    want = torch.log_softmax(logits, dim=-1)[torch.arange(39), torch.tensor(ids[1:])]
    bound = logits.abs().max(dim=-1).values * 2.0 ** -8 + 1e-4
    got = score_prompt(eng, ids, top=3)
    assert got.tok_lp.dtype == torch.float32 and got.tok_lp.shape == (39,)
    err = (got.tok_lp.double() - want).abs()
    print(f"max |lp - hf| {float(err.max()):.3e}, smallest bound {float(bound.min()):.3e}")
    assert bool((err <= bound).all())
    assert got.top_id.shape == (39, LP.TOP_MAX) and bool((got.top_id[:, 3:] == -1).all())
    # chunked logits give the same values
    monkeypatch.setattr(RS, "SCORE_CHUNK_BYTES", 7 * 2 * cfg.head_rows)
    eng.reset()
    again = score_prompt(eng, ids, top=3)
    assert all(torch.equal(a, b) for a, b in zip(got[1:], again[1:]))
    with pytest.raises(ValueError):
        score_prompt(eng, ids[:1])


def test_inference_cli_score_and_logprobs(hf, capsys):
    import inference
    _, shards = hf
    lps = inference.main(["--shards", shards, "--device", "cpu", "--score", "--prompt", "abc xyz, hello"])
    text = capsys.readouterr().out
    nll = -sum(lps) / len(lps)
    line = [ln for ln in text.splitlines() if "perplexity" in ln][0]
    assert float(line.split("perplexity")[1]) == pytest.approx(math.exp(nll), rel=1e-5)
    assert float(line.split("mean NLL")[1].split()[0]) == pytest.approx(nll, abs=1e-5)
    # --logprobs: a line per generated token (temperature 0: every token has rank 1)
    argv = ["--random", "tiny", "--device", "cpu", "--max-new-tokens", "6", "--prompt", "hello"]
    out = inference.main(argv + ["--logprobs", "2"])
    text = capsys.readouterr().out
    assert sum("logprob" in ln and "rank 1" in ln and "top [" in ln for ln in text.splitlines()) == len(out)
