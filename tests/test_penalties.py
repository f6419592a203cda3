"""Repetition / presence / frequency penalties, CPU side: the numpy reference against
transformers' RepetitionPenaltyLogitsProcessor (bitwise) and against a direct per-element
formula, SamplingParams, the CPU-engine server against a host loop (Sampler.logits ->
penalize_reference -> sample_reference), slot reuse, and the request / command-line plumbing."""
import numpy as np
import pytest
import torch

import penalty_cases as C
from llm_sharding_amd.config import tiny
from llm_sharding_amd.ops import penalties as P
from llm_sharding_amd.ops import sampling as S
from llm_sharding_amd.parallel.scheduler import plan_stages
from llm_sharding_amd.parallel.server import PipelineServer
from llm_sharding_amd.runtime.engine import RandomSource, StageEngine
from llm_sharding_amd.runtime.sampling import EagerSamplingDecode, PenaltyState, Sampler, SamplingParams


# ------------------------------------------------------------------------------ reference vs HF
def _hf_inputs(V=777, rows=4, L=23):
    rng = np.random.default_rng(7)
    ids = rng.integers(0, V, (rows, L))
    ids[:, 5] = ids[:, 2]                       # duplicates
    ids[:, 9:12] = ids[:, 0:1]
    scores = (3.0 * rng.standard_normal((rows, V))).astype(np.float32)
    scores[0, ids[0, 0]], scores[1, ids[1, 1]] = 0.0, -0.0
    state = np.zeros((rows + 2, V), dtype=np.uint16)
    slot = [3, 0, 5, 1]
    for r in range(rows):                       # the set of ids, split over prompt bits and counts
        for j, t in enumerate(ids[r]):
            if j % 3 == 0:
                state[slot[r], t] |= P.PROMPT_BIT
            else:
                state[slot[r], t] = (state[slot[r], t] & P.PROMPT_BIT) | min((state[slot[r], t] & 0x7FFF) + 1, 0x7FFF)
    return ids, scores, state, slot


@pytest.mark.parametrize("rho", [1.2, 0.8, 1.7])
def test_repetition_penalty_equals_hf_bitwise(rho):
    from transformers import RepetitionPenaltyLogitsProcessor
    ids, scores, state, slot = _hf_inputs()
    V = scores.shape[1]
    proc = RepetitionPenaltyLogitsProcessor(penalty=rho)
    # bf16 scores
    sc = torch.from_numpy(scores).to(torch.bfloat16)
    hf = proc(torch.from_numpy(ids), sc.clone())
    got, st = P.penalize_reference(sc, V, state, slot, None, rho, 0.0, 0.0)
    assert got.dtype == torch.bfloat16 and hf.dtype == torch.bfloat16
    assert torch.equal(got.view(torch.int16), hf.view(torch.int16))
    assert (st == state).all()                  # no input token: nothing counted
    assert not torch.equal(got.view(torch.int16), sc.view(torch.int16))
    # fp32 scores (the bf16 values upcast): the value before the bf16 rounding
    up = sc.float()
    hf32 = proc(torch.from_numpy(ids), up.clone()).numpy()
    for r in range(ids.shape[0]):
        x, _, applied = P.penalized_values(up[r].numpy(), state[slot[r]], -1, rho, 0.0, 0.0)
        assert (x.view(np.uint32) == hf32[r].view(np.uint32)).all()
        assert sorted(np.nonzero(applied)[0]) == sorted(set(ids[r].tolist()))


def test_all_off_rows_are_untouched():
    c = C.make_case(4, 1003, 1008, 6)
    lg, st = P.penalize_reference(c.logits, c.V, c.state, c.slot, c.tokens, 1.0, 0.0, 0.0)
    assert (lg == c.logits).all() and (st == c.state).all()
    # inside a mixed launch too, and the inputs are never modified
    before = (c.logits.copy(), c.state.copy())
    lg, st = C.reference(4, 1003, 1008, 6)
    off = np.nonzero((c.rep == 1) & (c.pres == 0) & (c.freq == 0))[0]
    assert off.size and (lg[off] == c.logits[off]).all() and (st[c.slot[off]] == c.state[c.slot[off]]).all()
    assert (c.logits == before[0]).all() and (c.state == before[1]).all()
    assert (lg[:, c.V:] == C.LOGIT_PAD).all() and (st[:, c.V:] == C.STATE_PAD).all()
    on = np.setdiff1d(np.arange(c.rows), off)
    assert all((lg[r] != c.logits[r]).any() for r in on)


# ------------------------------------------------------------------------------ presence / frequency
@pytest.mark.parametrize("rho, alpha, beta", [(1.0, 0.5, 0.0), (1.0, 0.0, 0.3), (1.3, 0.7, 0.25), (1.7, -0.4, -0.15),
                                              (0.8, 0.0, 0.0), (1.0, 0.0, 0.0)])
def test_reference_equals_the_direct_formula(rho, alpha, beta):
    V = 203
    rng = np.random.default_rng(3)
    bits = C.bf16_bits(4.0 * rng.standard_normal(V))
    bits[:4] = C.bf16_bits(np.array([0.0, -0.0, 2.0 ** -20, -(2.0 ** -20)], dtype=np.float32))
    st = np.zeros((2, V), dtype=np.uint16)
    hot = rng.random(V) < 0.3
    st[1, hot] = (rng.integers(0, 6, V).astype(np.uint16) | (rng.random(V) < 0.5).astype(np.uint16) * 0x8000)[hot]
    st[1, :4] = [2, 0x8000, 0x8001, 0]
    st[1, 100], st[1, 101] = 32766, 0x8000 | 32767
    for t in (0, 3, 100, 101, 57, V - 1, -1):
        want_l, want_s = C.direct(bits, st[1], t, rho, alpha, beta)
        got_l, got_s = P.penalize_reference(bits, V, st, [1], [t], [rho], [alpha], [beta])
        assert (got_l == want_l).all(), f"t={t}: logits differ at {np.nonzero(got_l != want_l)[0][:8]}"
        assert (got_s[1] == want_s).all() and (got_s[0] == 0).all()


def test_counts_saturate_at_32767():
    V = 16
    bits = C.bf16_bits(np.linspace(-3, 3, V))
    st = np.zeros((1, V), dtype=np.uint16)
    st[0, 4], st[0, 5] = 32766, 0x8000 | 32766
    for _ in range(3):
        _, st = P.penalize_reference(bits, V, st, [0], [4], 1.0, 0.0, 0.001)
        _, st = P.penalize_reference(bits, V, st, [0], [5], 1.0, 0.0, 0.001)
    assert st[0, 4] == 32767 and st[0, 5] == (0x8000 | 32767) and (np.delete(st[0], [4, 5]) == 0).all()
    lg, _ = P.penalize_reference(bits, V, st, [0], [4], 1.0, 0.25, 0.001)
    pen = np.float32(np.float32(np.float32(32767) * np.float32(0.001)) + np.float32(0.25))
    x = np.float32(P.bf16_bits_to_f32(bits)[4] - pen)
    assert lg[4] == P.bf16_rne_bits(np.array([x]))[0]


# ------------------------------------------------------------------------------ SamplingParams
def test_sampling_params_penalty_fields():
    sp = SamplingParams(0.7, 40, 0.9, 5)        # four positional arguments: unchanged
    assert (sp.temperature, sp.top_k, sp.top_p, sp.seed) == (0.7, 40, 0.9, 5)
    assert (sp.repetition_penalty, sp.presence_penalty, sp.frequency_penalty) == (1.0, 0.0, 0.0)
    assert not sp.penalized and not sp.plain and not sp.greedy
    assert SamplingParams(0.0, seed=1).plain and SamplingParams(0.0, seed=1).greedy
    p = SamplingParams(0.0, seed=1, repetition_penalty=1.2)
    assert p.greedy and p.penalized and not p.plain
    assert SamplingParams(seed=1, presence_penalty=-0.5).penalized
    assert SamplingParams(seed=1, frequency_penalty=0.1).penalized
    nan, inf = float("nan"), float("inf")
    for bad in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.2), dict(repetition_penalty=nan),
                dict(repetition_penalty=inf), dict(presence_penalty=nan), dict(presence_penalty=inf),
                dict(presence_penalty=-inf), dict(frequency_penalty=nan), dict(frequency_penalty=inf),
                dict(temperature=nan), dict(temperature=inf)):
        with pytest.raises(ValueError):
            SamplingParams(**bad)
    sp = SamplingParams.from_dict({"repetition_penalty": 1.2, "presence_penalty": 0.5, "frequency_penalty": 0.25,
                                   "seed": 9, "top_k": None})
    assert (sp.temperature, sp.repetition_penalty, sp.presence_penalty, sp.frequency_penalty, sp.seed) == \
        (0.0, 1.2, 0.5, 0.25, 9)
    assert SamplingParams.from_dict({"text": "x"}) is None


# ------------------------------------------------------------------------------ server vs a host loop
SEED = 11


def _engine(cfg, slots=1):
    return StageEngine(cfg, 0, cfg.num_hidden_layers, "cpu", torch.float32, has_embed=True, has_head=True,
                       source=RandomSource(cfg, SEED), max_slots=slots, max_seq=128)


def _prompts(cfg, lens):
    g = torch.Generator().manual_seed(5)
    out = [torch.randint(3, cfg.vocab_size, (n,), generator=g).tolist() for n in lens]
    for p in out:                                # prompts repeat tokens, as real ones do
        if len(p) > 4:
            p[3] = p[1]
    return out


def host_loop(cfg, prompt, sp, n_new):
    """One request, token by token on the host: Sampler.logits -> penalize_reference ->
    sample_reference."""
    eng, V = _engine(cfg), cfg.vocab_size
    smp = Sampler(eng)
    state = np.zeros((1, V), dtype=np.uint16)
    state[0, prompt] = P.PROMPT_BIT
    slot, pos = eng.prefill_rows([0], [len(prompt)])
    h = eng.forward(eng.embed(torch.tensor(prompt)), slot, pos)[-1:]
    eng.advance([0], [len(prompt)])
    out, t_in = [], None
    for i in range(n_new):
        lg = smp.logits(h, [0])
        lg, state = P.penalize_reference(lg, V, state, [0], t_in, sp.repetition_penalty, sp.presence_penalty,
                                         sp.frequency_penalty)
        tok, _, _, _ = S.sample_reference(lg, V, sp.temperature, sp.top_k, sp.top_p, sp.seed, len(prompt) + i)
        out.append(int(tok[0]))
        t_in = [out[-1]]
        slot, pos = eng.prefill_rows([0], [1])
        h = eng.forward(eng.embed(torch.tensor(t_in)), slot, pos)
        eng.advance([0], [1])
    return out


def _server(cfg, world=1, rank=0, batch=2, microbatches=2):
    st = plan_stages(cfg, world).stages[rank]
    return PipelineServer(cfg, RandomSource(cfg, SEED), rank, world, st.start, st.end, device="cpu", batch=batch,
                          microbatches=microbatches, max_seq=128, prefill_budget=16, dtype=torch.float32)


def _run(cfg, prompts, params, new=10, **kw):
    srv = _server(cfg, **kw)
    rids = [srv.submit(p, new, eos_ids=(), sampling=sp) for p, sp in zip(prompts, params)]
    srv.serve(stop_when_idle=True)
    return srv, [srv.requests[r].output_ids for r in rids]


REP = SamplingParams(0.0, seed=1, repetition_penalty=1.3)
PF = SamplingParams(0.8, seed=77, presence_penalty=0.5, frequency_penalty=0.3)


def test_server_equals_the_host_loop_and_leaves_neighbours_alone():
    cfg = tiny(layers=2)
    prompts = _prompts(cfg, (7, 12, 5))
    srv, out = _run(cfg, prompts, [REP, PF, None])
    assert srv.sampling_on and srv.penalties is not None
    assert out[0] == host_loop(cfg, prompts[0], REP, 10)
    assert out[1] == host_loop(cfg, prompts[1], PF, 10)
    # the penalties did something: the same requests without them give other tokens
    s2, bare = _run(cfg, prompts, [None, SamplingParams(0.8, seed=77), None])
    # (a negative presence penalty makes the first generated token win every later step)
    _, stuck = _run(cfg, prompts[:1], [SamplingParams(0.0, seed=1, presence_penalty=-1e4)], new=6)
    assert stuck[0] == [bare[0][0]] * 6 and bare[0][:6] != stuck[0]
    sp = SamplingParams(0.0, seed=1, repetition_penalty=50.0, presence_penalty=1e4)
    _, hard = _run(cfg, prompts[:1], [sp], new=24)
    assert len(set(hard[0])) == 24                                # nothing generated is ever chosen again
    assert hard[0] == host_loop(cfg, prompts[0], sp, 24)
    # the plain greedy request: as in a sampling-enabled server with no penalised neighbour
    assert s2.sampling_on and s2.penalties is None
    assert out[2] == bare[2]
    # the counts the server holds are the request's generated tokens but the last
    cnt = srv.penalties.counts(0)
    want = np.bincount(out[0][:-1], minlength=cfg.vocab_size)
    assert (cnt.numpy() == want).all()
    # an all-greedy and a sampling-only server never build the table
    s3, _ = _run(cfg, prompts[:1], [SamplingParams(0.0, seed=3)])
    assert not s3.sampling_on and s3.penalties is None


def test_slot_reuse_reproduces_a_fresh_server():
    cfg = tiny(layers=2)
    prompts = _prompts(cfg, (7, 9, 6, 11))
    dirty = [SamplingParams(0.9, seed=20 + i, repetition_penalty=1.5, frequency_penalty=0.4) for i in range(4)]
    # one slot: every request but the first enters a slot a penalised request has just left
    srv, out = _run(cfg, prompts + [prompts[0], prompts[1]], dirty + [PF, REP], batch=1, microbatches=1)
    _, fresh = _run(cfg, [prompts[0]], [PF], batch=1, microbatches=1)
    _, fresh2 = _run(cfg, [prompts[1]], [REP], batch=1, microbatches=1)
    assert out[4] == fresh[0] and out[5] == fresh2[0]
    # an unpenalised request after a penalised one in the same slot is not penalised
    _, mixed = _run(cfg, [prompts[0], prompts[2]], [dirty[0], None], batch=1, microbatches=1)
    _, plain = _run(cfg, [prompts[2]], [None], batch=1, microbatches=1)
    assert mixed[1] == plain[0]


def test_server_rejects_penalties_with_more_than_one_stage():
    cfg = tiny(layers=2)
    srv = _server(cfg, world=2)
    with pytest.raises(ValueError, match="single-stage"):
        srv.submit([3, 4, 5], 4, sampling=SamplingParams(0.0, seed=1, repetition_penalty=1.2))
    with pytest.raises(ValueError, match="single-stage"):
        srv.submit([3, 4, 5], 4, sampling=SamplingParams(0.0, seed=1, presence_penalty=0.5))
    srv.submit([3, 4, 5], 4, sampling=SamplingParams(0.0, seed=1))


def test_split_head_is_rejected():
    cfg = tiny(layers=2)
    eng = StageEngine(cfg, 0, cfg.num_hidden_layers, "cpu", torch.float32, has_embed=True, has_head=True,
                      source=RandomSource(cfg, SEED), max_slots=2, max_seq=128, head_cols=(0, cfg.head_rows // 2))
    with pytest.raises(NotImplementedError, match="split head"):
        PenaltyState(eng, 2)


def test_eager_twin_counts_and_penalises():
    cfg = tiny(layers=2)
    prompt = _prompts(cfg, (7,))[0]
    eng = _engine(cfg, slots=2)
    pen = PenaltyState(eng, 2)
    pen.admit(1, prompt)
    slot, pos = eng.prefill_rows([1], [len(prompt)])
    h = eng.forward(eng.embed(torch.tensor(prompt)), slot, pos)
    eng.advance([1], [len(prompt)])
    first = Sampler(eng, pen).sample(h, [len(prompt) - 1], [PF], [len(prompt)], slots=[1])
    g = EagerSamplingDecode(eng, 1, "full", slots=[1], history_len=9, penalties=pen)
    g.set_params(0, PF)
    g.tokens.copy_(first.to(torch.int32))
    for _ in range(9):
        g.replay()
    assert [int(first[0])] + g.history[:, 0].tolist() == host_loop(cfg, prompt, PF, 10)
    with pytest.raises(RuntimeError, match="PenaltyState"):
        Sampler(eng).sample(h, [0], [PF], [3])


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


def test_submit_message_penalty_keys():
    from llm_sharding_amd.parallel.ingress import submit_message
    srv, rep = _FakeServer(), _FakeReplies()
    msg = {"input_ids": [3, 4], "repetition_penalty": 1.2, "presence_penalty": 0.5, "frequency_penalty": 0.25}
    assert submit_message(srv, msg, None, 8, rep) == 1
    sp = srv.calls[-1][2]["sampling"]
    assert (sp.temperature, sp.repetition_penalty, sp.presence_penalty, sp.frequency_penalty) == (0.0, 1.2, 0.5, 0.25)
    assert submit_message(srv, {"input_ids": [3], "repetition_penalty": 0.0}, None, 8, rep) == 0
    assert rep.errors and "repetition_penalty" in rep.errors[-1]


def test_inference_cli_penalty_flags(capsys):
    import inference
    a = inference.build_parser().parse_args([])
    assert inference.sampling_from_args(a) is None
    a = inference.build_parser().parse_args(["--repetition-penalty", "1.2"])
    sp = inference.sampling_from_args(a)
    assert sp.greedy and sp.repetition_penalty == 1.2 and not sp.plain
    a = inference.build_parser().parse_args(["--temperature", "0.7", "--presence-penalty", "0.5",
                                             "--frequency-penalty", "0.25", "--seed", "4"])
    sp = inference.sampling_from_args(a)
    assert (sp.temperature, sp.presence_penalty, sp.frequency_penalty, sp.seed) == (0.7, 0.5, 0.25, 4)
    with pytest.raises(SystemExit):
        inference.main(["--random", "tiny", "--repetition-penalty", "1.2", "--hf-compare", "x"])
    argv = ["--random", "tiny", "--device", "cpu", "--max-new-tokens", "12", "--prompt", "hello hello"]
    greedy = inference.main(argv)
    r1 = inference.main(argv + ["--repetition-penalty", "1.5", "--presence-penalty", "2.0"])
    r2 = inference.main(argv + ["--repetition-penalty", "1.5", "--presence-penalty", "2.0"])
    assert r1 == r2 and len(r1) <= 12
    assert "penalties: repetition 1.5" in capsys.readouterr().out
    assert len(greedy) <= 12
