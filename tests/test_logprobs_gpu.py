"""Per-token log-probabilities on the device (csrc/sampling/logprobs.hip): the kernel against the
fp64 reference on the shared cases (tests/logprob_cases.py: ids and ranks exactly, values to the
derived 1e-4), skipped rows and targets, bitwise determinism and placement independence, the
captured SamplingDecodeGraph with and without the logprobs launch, penalised rows, the fp8 and
GPT-2 heads and score_prompt on the HIP engine."""
import numpy as np
import pytest
import torch

import logprob_cases as C
from llm_sharding_amd.config import LlamaConfig, tiny, tiny_gpt2
from llm_sharding_amd.ops import logprobs as LP
from llm_sharding_amd.ops import penalties as P
from llm_sharding_amd.runtime.engine import RandomSource, StageEngine
from llm_sharding_amd.runtime.sampling import (PenaltyState, Sampler, SamplingDecodeGraph, SamplingParams,
                                               score_prompt)

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT_F, SENT_I = 12345.0, -77  # prefilled into the outputs: what an unwritten entry keeps


def _launch(view: torch.Tensor, V: int, n_top, target, sentinel: bool = False) -> LP.Logprobs:
    """lsa_logprobs on a device view -> host tensors."""
    rows = view.shape[0]
    out = LP.alloc_outputs(rows, DEV)
    if sentinel:
        for t in out:
            t.fill_(SENT_F if t.dtype == torch.float32 else SENT_I)
    LP.logprobs(view, V, rows, torch.tensor(n_top, dtype=torch.int32, device=DEV),
                torch.tensor(target, dtype=torch.int32, device=DEV), out)
    torch.cuda.synchronize()
    return LP.Logprobs(*(t.cpu() for t in out))


def _equal(a: LP.Logprobs, b: LP.Logprobs, ra=slice(None), rb=slice(None)) -> bool:
    """Bitwise equality of two results (NaN patterns included)."""
    return all(torch.equal(x[ra].contiguous().view(torch.int32), y[rb].contiguous().view(torch.int32))
               for x, y in zip(a, b))


# ------------------------------------------------------------------------------ shapes
def test_v1():
    lg = torch.tensor([[3.25], [-7.0]], dtype=torch.bfloat16)
    got = _launch(lg.to(DEV), 1, [20, 0], [0, 0])
    C.check(got, C.logprobs_reference(lg, 1, [20, 0], [0, 0]), what="V=1")
    assert got.tok_lp.tolist() == [0.0, 0.0] and got.top_id[0].tolist() == [0] + [-1] * 19


def test_v7_tail():
    lg = C.gaussian_rows(4, 7, 1)
    lg[1] = 0.5                    # all seven tie
    lg[2, 3] = float("-inf")
    tg = [0, 6, 3, 2]
    got = _launch(lg.to(DEV), 7, [20] * 4, tg)
    C.check(got, C.logprobs_reference(lg, 7, 20, tg), what="V=7")
    assert (got.top_id[:, 7:] == -1).all() and torch.isneginf(got.top_lp[:, 7:]).all()
    assert got.top_id[1, :7].tolist() == list(range(7))


def test_unaligned_rows_and_nan_padding():
    """V = 32003 in an ld = 32016 buffer whose other columns are NaN, the view one element into
    the buffer: no row base is 16-byte aligned and a column >= V that was read would poison lse."""
    V, ld, rows = 32003, 32016, 5
    lg, tg, n_top = C.mixed_batch(rows, V, 4)
    tg[1], n_top[1] = V - 1, 20
    buf, _ = C.padded(lg, ld, offset=1)
    dbuf = buf.to(DEV)
    view = dbuf[1:1 + rows * ld].view(rows, ld)
    assert view.data_ptr() % 16 != 0 and (view.stride(0) * 2) % 16 == 0
    got = _launch(view, V, n_top, tg)
    C.check(got, C.logprobs_reference(lg, V, n_top, tg), what="V=32003 unaligned")


def test_v128256():
    V = 128256
    lg = C.gaussian_rows(3, V, 5)
    lg[2] = C.constant_row(V)      # three index levels of the tie break
    tg = [C.targets_of(lg[0])[1], V - 1, V - 1]
    got = _launch(lg.to(DEV), V, [20, 5, 20], tg)
    C.check(got, C.logprobs_reference(lg, V, [20, 5, 20], tg), what="V=128256")


@pytest.mark.parametrize("V", [4099, 32000])
def test_every_row_kind(V):
    lg, tg, kinds = C.every_kind(V)
    got = _launch(lg.to(DEV), V, [20] * len(tg), tg)
    ref = C.logprobs_reference(lg, V, 20, tg)
    for i in range(0, len(tg), 3):
        C.check(got, ref, rows=slice(i, i + 3), what=f"{kinds[i]} V={V}")
    k = kinds.index("near_constant")
    assert got.top_id[k].tolist() == list(range(1, 41, 2))


def test_mixed_n_top():
    V = 32000
    lg, tg, n_top = C.mixed_batch(24, V, 6)
    assert set(n_top) == {0, 1, 5, 20}
    got = _launch(lg.to(DEV), V, n_top, tg)
    C.check(got, C.logprobs_reference(lg, V, n_top, tg), what="mixed n_top")
    for r, n in enumerate(n_top):
        assert (got.top_id[r, n:] == -1).all() and (got.top_id[r, :n] >= 0).all()


# ------------------------------------------------------------------------------ skipped rows / targets
@pytest.fixture(scope="module")
def batch129():
    V, ld = 50257, 50304
    lg, tg, n_top = C.mixed_batch(129, V, 8)
    n_top = [-1 if r % 3 == 1 else n for r, n in enumerate(n_top)]
    _, view = C.padded(lg, ld)
    dev = view.to(DEV)
    return V, lg, tg, n_top, dev, _launch(dev, V, n_top, tg, sentinel=True)


def test_skipped_rows_keep_the_sentinel(batch129):
    V, lg, tg, n_top, _, got = batch129
    skip = np.array(n_top) < 0
    assert skip.sum() == 43
    for t in got:
        s = t[torch.from_numpy(skip)]
        assert bool((s == (SENT_F if t.dtype == torch.float32 else SENT_I)).all())
    live = np.nonzero(~skip)[0]
    ref = C.logprobs_reference(lg[live], V, [n_top[i] for i in live], [tg[i] for i in live])
    C.check(LP.Logprobs(*(t[live] for t in got)), ref, what="129 rows, a third skipped")


def test_target_outside_the_vocabulary():
    V = 4099
    lg, _, n_top = C.mixed_batch(8, V, 9)
    tg = [-1, 5, V, 7, -1, V + 3, 0, V - 1]
    got = _launch(lg.to(DEV), V, n_top, tg, sentinel=True)
    off = torch.tensor([t < 0 or t >= V for t in tg])
    assert bool((got.tok_lp[off] == SENT_F).all()) and bool((got.tok_rank[off] == SENT_I).all())
    ref = C.logprobs_reference(lg, V, n_top, tg)
    on = np.nonzero(~off.numpy())[0]
    C.check(LP.Logprobs(*(t[on] for t in got)), LP.Logprobs(*(t[on] for t in ref)), what="valid targets")
    # lse and the top-n of the rows without a target are written all the same
    np.testing.assert_allclose(got.lse.numpy(), ref.lse, atol=C.TOL, rtol=0)
    assert (got.top_id.numpy() == ref.top_id).all()


def test_lp_history_rows_and_argument_checks():
    """The history write lands in row ``step_ctr - 1`` and only for counters 1..len: a sentinel
    frame around the history stays intact. The binding rejects mismatched arguments."""
    V, rows, hl = 777, 3, 2
    lg = C.gaussian_rows(rows, V, 12).to(DEV)
    nt = torch.tensor([0, -1, 3], dtype=torch.int32, device=DEV)
    tg = torch.tensor([5, 6, V - 1], dtype=torch.int32, device=DEV)
    frame = torch.full((hl + 2, rows), SENT_F, dtype=torch.float32, device=DEV)
    hist = frame[1:1 + hl]
    for ctr in (0, 1, 2, 3, 1 << 30):
        frame.fill_(SENT_F)
        out = LP.alloc_outputs(rows, DEV)
        LP.logprobs(lg, V, rows, nt, tg, out, lp_history=hist,
                    step_ctr=torch.tensor([ctr], dtype=torch.int32, device=DEV))
        torch.cuda.synchronize()
        want = torch.full_like(frame, SENT_F)
        if 1 <= ctr <= hl:
            want[ctr, 0], want[ctr, 2] = out.tok_lp[0], out.tok_lp[2]   # frame row ctr = history row ctr - 1
        assert torch.equal(frame, want), f"step counter {ctr}"
    out = LP.alloc_outputs(rows, DEV)
    for bad in (dict(n_top=nt[:2]), dict(target=tg.long()), dict(rows=4), dict(V=V + 1), dict(logits=lg.float()),
                dict(out=LP.Logprobs(*out[:3], out.top_id[:2], out.top_lp)), dict(lp_history=hist[:, :2]),
                dict(lp_history=hist)):
        kw = dict(logits=lg, V=V, rows=rows, n_top=nt, target=tg, out=out)
        kw.update(bad)
        with pytest.raises((ValueError, RuntimeError)):
            LP.logprobs(**kw)


# ------------------------------------------------------------------------------ determinism, placement
def test_bitwise_determinism(batch129):
    V, _, tg, n_top, dev, got = batch129
    for _ in range(2):
        assert _equal(_launch(dev, V, n_top, tg, sentinel=True), got)


def test_row_permutation(batch129):
    V, _, tg, n_top, dev, got = batch129
    perm = np.random.default_rng(5).permutation(129)
    p = _launch(dev[torch.from_numpy(perm).to(DEV)].contiguous(), V, [n_top[i] for i in perm],
                [tg[i] for i in perm], sentinel=True)
    assert _equal(p, got, rb=torch.from_numpy(perm))


def test_row_alone_equals_row_in_batch(batch129):
    V, _, tg, n_top, dev, got = batch129
    for r in (0, 2, 12, 17, 128):  # a Gaussian row, the constant, spread and -inf rows, the last row
        assert n_top[r] >= 0
        one = _launch(dev[r:r + 1], V, [n_top[r]], [tg[r]], sentinel=True)
        assert _equal(one, got, rb=slice(r, r + 1)), f"row {r}"


# ------------------------------------------------------------------------------ graphs
def _tiny_engine(slots=4):
    cfg = tiny(layers=2)
    return cfg, StageEngine(cfg, 0, 2, DEV, torch.bfloat16, has_embed=True, has_head=True,
                            source=RandomSource(cfg, 0), max_slots=slots, max_seq=128, max_prefill_rows=64)


def _graph_run(eng, params, steps, penalties=None, **kw):
    """Prefill four prompts, sample the first tokens, capture a graph and replay ``steps`` times.
    Returns (graph, first tokens, per-step (logits, raw logits, tokens, lp) copies)."""
    g = torch.Generator().manual_seed(3)
    prompts = [torch.randint(3, eng.cfg.vocab_size, (n,), generator=g).tolist() for n in (5, 9, 3, 7)]
    eng.reset()
    sl, po = eng.prefill_rows([0, 1, 2, 3], [len(p) for p in prompts])
    h = eng.forward(eng.embed(torch.tensor([t for p in prompts for t in p], device=DEV)), sl, po)
    eng.advance([0, 1, 2, 3], [len(p) for p in prompts])
    last = [int(i) for i in np.cumsum([len(p) for p in prompts]) - 1]
    if penalties is not None:
        penalties.state.zero_()
        for s, p in enumerate(prompts):
            penalties.admit(s, p)
    smp = Sampler(eng, penalties)
    first = smp.sample(h, last, params, [len(p) for p in prompts],
                       slots=[0, 1, 2, 3] if penalties is not None else None)
    gr = SamplingDecodeGraph(eng, 4, "full", history_len=steps, penalties=penalties, **kw)
    for i, p in enumerate(params):
        gr.set_params(i, p)
    gr.tokens.copy_(first.to(torch.int32))
    gr.capture()
    rec = []
    for _ in range(steps):
        gr.replay()
        torch.cuda.synchronize()
        rec.append((gr.logits.cpu(), None if gr.raw_logits is None else gr.raw_logits.cpu(), gr.tokens.cpu(),
                    None if gr.lp is None else LP.Logprobs(*(t.cpu().clone() for t in gr.lp))))
    return gr, first.cpu(), rec


PARAMS = [SamplingParams(0.7, top_p=0.9, seed=11, logprobs=5), SamplingParams(1.0, top_k=50, seed=12),
          SamplingParams(0.0, logprobs=0), SamplingParams(1.3, top_k=200, top_p=0.95, seed=14, logprobs=20)]


def test_graph_logprobs_over_replays():
    cfg, eng = _tiny_engine()
    V = cfg.vocab_size
    gr, _, rec = _graph_run(eng, PARAMS, 4, logprobs=True)
    n_top = [p.n_top for p in PARAMS]
    assert gr.n_top.tolist() == [5, -1, 0, 20]
    live = [0, 2, 3]
    hist = gr.lp_history.cpu()
    for s, (lg, _, tok, lp) in enumerate(rec):
        assert tok.tolist() == gr.history[s].tolist()
        ref = C.logprobs_reference(lg[live], V, [n_top[i] for i in live], [int(tok[i]) for i in live])
        C.check(LP.Logprobs(*(t[live] for t in lp)), ref, what=f"replay {s}")
        assert torch.equal(hist[s, live].view(torch.int32), lp.tok_lp[live].view(torch.int32))
        assert bool(torch.isnan(hist[s, 1])) and bool(torch.isnan(lp.tok_lp[1])) and int(lp.top_id[1, 0]) == -1
        assert int(lp.tok_rank[2]) == 1 and int(lp.top_id[0, 0]) == int(lg[0, :V].float().argmax())
    with pytest.raises(RuntimeError):
        SamplingDecodeGraph(eng, 4, "full").set_params(0, PARAMS[0])


def test_graph_without_logprobs_is_todays_graph():
    """Built without ``logprobs`` (the default, and explicitly): no logprobs buffers, and the token
    history of the same seeds is identical - also to the graph that does run the extra launch,
    which only reads."""
    _, eng = _tiny_engine()
    plain = [SamplingParams(p.temperature, p.top_k, p.top_p, p.seed) for p in PARAMS]
    g0, f0, _ = _graph_run(eng, plain, 4)
    g1, f1, _ = _graph_run(eng, plain, 4, logprobs=False)
    g2, f2, _ = _graph_run(eng, PARAMS, 4, logprobs=True)
    assert g0.lp is None and g0.n_top is None and g0.lp_history is None and g1.lp is None
    assert torch.equal(f0, f1) and torch.equal(g0.history, g1.history)
    assert torch.equal(f0, f2) and torch.equal(g0.history, g2.history)


def test_penalised_rows_describe_the_penalised_logits():
    cfg, eng = _tiny_engine()
    V = cfg.vocab_size
    pen = PenaltyState(eng, 4)
    params = [SamplingParams(0.8, seed=21, repetition_penalty=1.3, frequency_penalty=0.4, logprobs=20),
              SamplingParams(0.0, presence_penalty=1.5, logprobs=3), SamplingParams(0.9, seed=23, logprobs=2),
              SamplingParams(0.0, repetition_penalty=1.2)]
    gr, first, rec = _graph_run(eng, params, 3, penalties=pen, debug_raw=True, logprobs=True)
    # replay the penalty state on the host from the prompts and the tokens fed to each step
    g = torch.Generator().manual_seed(3)
    prompts = [torch.randint(3, V, (n,), generator=g).tolist() for n in (5, 9, 3, 7)]
    state0 = np.zeros((4, cfg.head_rows), dtype=np.uint16)
    for s, p in enumerate(prompts):
        state0[s, p] = P.PROMPT_BIT
    fed, changed = first.to(torch.int32), False
    rep, pres, freq = ([getattr(p, k) for p in params] for k in ("repetition_penalty", "presence_penalty",
                                                                  "frequency_penalty"))
    for s, (lg, raw, tok, lp) in enumerate(rec):
        want, state0 = P.penalize_reference(raw, V, state0, [0, 1, 2, 3], fed.tolist(), rep, pres, freq)
        assert torch.equal(want[:, :V].view(torch.int16), lg[:, :V].view(torch.int16))
        changed |= not torch.equal(raw[:3, :V].view(torch.int16), lg[:3, :V].view(torch.int16))
        ref = C.logprobs_reference(want[:3], V, [20, 3, 2], tok[:3].tolist())
        C.check(LP.Logprobs(*(t[:3] for t in lp)), ref, what=f"penalised, replay {s}")
        fed = tok
    assert changed, "the penalties never edited a logit: the case shows nothing"


def test_server_rebuilds_its_graphs_for_logprobs():
    """Graph-mode server: no logprobs launch until the first request that asks (here behind a
    sampling request, so the graphs are rebuilt a second time); then per-token values that agree
    with each other - rank 1 and the first alternative for a temperature-0 request, the token's
    own entry in the alternatives for a sampled one."""
    from llm_sharding_amd.parallel.server import PipelineServer
    cfg = tiny(layers=2)
    srv = PipelineServer(cfg, RandomSource(cfg, 11), 0, 1, 0, cfg.num_hidden_layers, device=DEV, batch=2,
                         microbatches=2, max_seq=128, prefill_budget=16)
    g = torch.Generator().manual_seed(5)
    prompts = [torch.randint(3, cfg.vocab_size, (n,), generator=g).tolist() for n in (3, 9, 20, 6)]
    srv.submit(prompts[0], 6, eos_ids=(), sampling=SamplingParams(0.9, seed=4))
    srv.serve(stop_when_idle=True)
    assert srv.sampling_on and not srv.logprobs_on and all(x.lp is None for x in srv.graphs)
    params = [SamplingParams(0.0, logprobs=2), None, SamplingParams(1.0, seed=7, logprobs=20)]
    rids = [srv.submit(p, 8, eos_ids=(), sampling=sp) for p, sp in zip(prompts[1:], params)]
    srv.serve(stop_when_idle=True)
    assert srv.logprobs_on and all(x.lp is not None for x in srv.graphs)
    r0, r1, r2 = (srv.requests[r] for r in rids)
    assert r1.token_logprobs is None and r1.top_logprobs is None and len(r1.output_ids) == 8
    assert len(r0.token_logprobs) == len(r0.top_logprobs) == 8 and r0.ranks == [1] * 8
    for tok, lp, top in zip(r0.output_ids, r0.token_logprobs, r0.top_logprobs):
        assert len(top) == 2 and top[0] == [tok, lp] and top[1][1] <= lp < 0.0
    assert len(r2.token_logprobs) == len(r2.ranks) == len(r2.top_logprobs) == 8
    for tok, lp, rk, top in zip(r2.output_ids, r2.token_logprobs, r2.ranks, r2.top_logprobs):
        vals = [v for _, v in top]
        assert len(top) == 20 and vals == sorted(vals, reverse=True) and sum(np.exp(vals)) <= 1.0 + 1e-4
        assert rk <= 20 or tok not in [i for i, _ in top]
        if rk <= 20:
            assert top[rk - 1][1] == lp      # equal logits share the rank and the value


# ------------------------------------------------------------------------------ fp8 / GPT-2 heads
@pytest.mark.parametrize("kind", ["fp8", "gpt2"])
def test_fp8_and_gpt2_heads(kind):
    from test_sampling_gpu import _CpuGen
    cfg = (tiny(layers=1, hidden=1024, heads=8, kv_heads=8, head_dim=128, inter=2048, vocab=4096) if kind == "fp8"
           else tiny_gpt2(layers=1))
    eng = StageEngine(cfg, 0, 1, DEV, torch.bfloat16, weight_dtype="fp8" if kind == "fp8" else "bf16",
                      has_embed=True, has_head=True, source=_CpuGen(cfg, 4), max_slots=2, max_seq=64,
                      max_prefill_rows=64)
    assert (eng.lm_head_s is not None) == (kind == "fp8")
    V = cfg.vocab_size
    h = torch.randn((9, cfg.hidden_size), generator=torch.Generator().manual_seed(2)).to(torch.bfloat16).to(DEV)
    smp = Sampler(eng)
    lg = smp.logits(h, [7, 0, 3, 3, 8])
    tg = [int(lg[0, :V].float().argmax()), V - 1, 0, 5, 17]
    got = smp.logprobs(lg, tg, [20, 0, 5, -1, 1])
    ref = C.logprobs_reference(lg.cpu(), V, [20, 0, 5, -1, 1], tg)
    C.check(LP.Logprobs(*(t.cpu() for t in got)), ref, what=f"{kind} head")
    assert int(got.top_id.max()) < V  # the padded vocabulary never shows up
    tok, lp = smp.sample(h, [1, 2], [SamplingParams(0.0, logprobs=2), SamplingParams(1.0, seed=3)], [4, 4],
                         return_logprobs=True)
    assert int(lp.tok_rank[0]) == 1 and int(lp.top_id[0, 0]) == int(tok[0]) and int(lp.top_id[1, 0]) == -1


# ------------------------------------------------------------------------------ score_prompt
def test_score_prompt_on_the_hip_engine(monkeypatch):
    """A 100-token prompt on the 7B-shaped two-layer config: the kernel's values against the
    reference on the engine's own logits (chunked: the chunk size is forced down so that the
    prompt takes four logits chunks)."""
    import llm_sharding_amd.runtime.sampling as RS
    cfg = LlamaConfig(num_hidden_layers=2, vocab_size=4096, max_position_embeddings=1024, name="7b-2L")
    eng = StageEngine(cfg, 0, 2, DEV, torch.bfloat16, has_embed=True, has_head=True, source=RandomSource(cfg, 0),
                      max_slots=1, max_seq=256, max_prefill_rows=128)
    ids = torch.randint(3, cfg.vocab_size, (100,), generator=torch.Generator().manual_seed(9)).tolist()
    seen, plain_logits = [], Sampler.logits

    def recording(self, h, rows_idx=None):  # the engine's own logits, as score_prompt sees them
        seen.append(plain_logits(self, h, rows_idx))
        return seen[-1]

    monkeypatch.setattr(Sampler, "logits", recording)
    for chunk_rows, n_chunks in ((None, 1), (30, 4)):
        if chunk_rows is not None:
            monkeypatch.setattr(RS, "SCORE_CHUNK_BYTES", chunk_rows * 2 * cfg.head_rows)
        seen.clear()
        eng.reset()
        got = score_prompt(eng, ids, top=5)
        assert got.tok_lp.shape == (99,) and got.tok_lp.dtype == torch.float32 and got.top_id.shape == (99, 20)
        assert len(seen) == n_chunks and max(s.numel() * 2 for s in seen) <= RS.SCORE_CHUNK_BYTES
        ref = C.logprobs_reference(torch.cat(seen).cpu(), cfg.vocab_size, 5, ids[1:])
        C.check(got, ref, what=f"score_prompt in {n_chunks} chunk(s)")


# Mean-NLL difference between the fp64 log-softmax of Sampler.logits (the path that existed before
# lsa_logprobs) and transformers' fp32 on this checkpoint and prompt, measured on an MI355X
# (profiles/logprobs.md); the new path has to stay within twice that.
NLL_DIFF_PARENT_PATH = 1.595e-4


def test_score_prompt_mean_nll_against_transformers(tmp_path):
    pytest.importorskip("transformers")
    from test_llama_hf_parity import _hf_model
    from llm_sharding_amd.runtime.engine import ShardFolderSource
    from llm_sharding_amd.utils.model_sharder import ModelSharder
    m, d = _hf_model(tmp_path, "llama2", hidden=256, heads=4, kv=2, inter=512, vocab=512, layers=3, scale=4.0)
    shards = ModelSharder(d, "llama", str(tmp_path / "shards"), dtype=torch.bfloat16, verbose=False).save_shards()
    cfg = LlamaConfig.from_pretrained(shards)
    eng = StageEngine(cfg, 0, cfg.num_hidden_layers, DEV, torch.bfloat16, has_embed=True, has_head=True,
                      source=ShardFolderSource(shards, cfg), max_slots=1, max_seq=128, max_prefill_rows=128)
    ids = torch.randint(3, cfg.vocab_size - 1, (100,), generator=torch.Generator().manual_seed(10)).tolist()
    with torch.no_grad():
        hf_lp = torch.log_softmax(m(torch.tensor([ids])).logits[0, :-1].float(), dim=-1)
    hf_nll = -float(hf_lp[torch.arange(99), torch.tensor(ids[1:])].double().mean())
    # the parent's path: Sampler.logits -> fp64 log-softmax on the host
    sl, po = eng.prefill_rows([0], [100])
    h = eng.forward(eng.embed(torch.tensor(ids, device=DEV)), sl, po)
    lg = Sampler(eng).logits(h, list(range(99)))[:, :cfg.vocab_size].cpu().double()
    parent_nll = -float(torch.log_softmax(lg, dim=-1)[torch.arange(99), torch.tensor(ids[1:])].mean())
    eng.reset()
    nll = -float(score_prompt(eng, ids).tok_lp.double().mean())
    print(f"mean NLL: transformers fp32 {hf_nll:.6f}, fp64 log-softmax of Sampler.logits {parent_nll:.6f} "
          f"(diff {parent_nll - hf_nll:+.3e}), score_prompt {nll:.6f} (diff {nll - hf_nll:+.3e})")
    assert abs(nll - hf_nll) <= 2.0 * NLL_DIFF_PARENT_PATH
