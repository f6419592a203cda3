"""Whole forwards at every row count where the route signature changes (tests/engine_edge_cases.py).

Two-layer engines at Llama-2-7B and Llama-2-13B layer shapes, vocab 4096, 512 slots of 64
positions. One case is one row count R: a 2-token prompt in the first R slots (a 2R-row prefill),
then one teacher-forced decode step of R rows. The weights are drawn once per shape set and shared
by every engine and by the fp32 golden model, which runs once for all 512 sequences (they are
independent, so a case compares with ``[:R]``).

* golden: hidden states after the prefill and after the captured decode step against
  ReferenceLlama in fp32 at ``utils.numerics.rel_err < 3e-2`` (the engine tolerance of
  tests/test_engine_gpu.py: global, worst 16x16 tile and worst row), greedy tokens wherever the
  golden top-2 margin is clear;
* bitwise twins (``torch.equal``): the DecodeGraph replay and the eager step; layers [0, 2) in one
  engine and engines [0, 1) then [1, 2); ``kv_layout="paged"`` on a shuffled pool and the static
  engine; in 385..512 rows ``LSA_GEMM_SKP=1`` and ``0`` wherever the plan keeps gemm_sk's tile and
  split (the rule of tests/test_gemm_skp_gpu.py::test_engine_route_on_and_off; elsewhere its
  tolerance);
* quantised weights (fp8, int4): above the native limits the engine dequantises into ``w_scratch``
  and runs the bf16 kernels, so it equals, bit for bit, a plain StageEngine whose packed
  projections were overwritten with bf16(dequantise(quantise(w))); at and below the limits (and
  for int4 up to 128 rows, where the int4 engine skips the coop EPI_PARTIAL route) it is held to
  3e-2 against the fp32 golden model built on the dequantised weights.

"The eager step" is ``_forward_hip(..., nsplit=decode_nsplit(R))``, the body DecodeGraph captures:
``forward`` itself sends more than 128 rows to the flash-prefill attention instead.
"""
import os
from contextlib import contextmanager

import pytest
import torch

import engine_edge_cases as E
from llm_sharding_amd.models.reference import ReferenceLlama
from llm_sharding_amd.ops import hip, int4, packing
from llm_sharding_amd.runtime.engine import DecodeGraph, RandomSource, StageEngine, WeightSource
from llm_sharding_amd.runtime.engine_int4 import make_stage_engine
from llm_sharding_amd.runtime.engine_skp import SKP_MAX_ROWS, SKP_MIN_ROWS
from llm_sharding_amd.utils.numerics import rel_err
from test_gemm_skp_gpu import _sk_equal_ranges
from test_kv_paged_gpu import _shuffle_pool

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 3e-2      # tests/test_engine_gpu.py
SLOTS, P = 512, 2
SEED = 17
ENGINE_KW = dict(max_slots=SLOTS, max_seq=E.MAX_SEQ, max_prefill_rows=E.MAX_PREFILL_ROWS)
PROJ = ("qkv", "o", "gate_up", "down")


@contextmanager
def _skp(on: bool):
    old = os.environ.get("LSA_GEMM_SKP")
    os.environ["LSA_GEMM_SKP"] = "1" if on else "0"
    try:
        yield
    finally:
        if old is None:
            del os.environ["LSA_GEMM_SKP"]
        else:
            os.environ["LSA_GEMM_SKP"] = old


class _Drawn(WeightSource):
    """RandomSource's draws, made once on the device and handed to every engine and golden model."""

    def __init__(self, cfg):
        src = RandomSource(cfg, SEED)
        bf = torch.bfloat16
        self.layers = [src.layer(i, DEV, bf) for i in range(cfg.num_hidden_layers)]
        self.embed, self.norm, self.head = src.embedding(DEV, bf), src.final_norm(DEV, bf), src.lm_head(DEV, bf)

    def layer(self, i, device, dtype):
        return self.layers[i]

    def embedding(self, device, dtype):
        return self.embed

    def final_norm(self, device, dtype):
        return self.norm

    def lm_head(self, device, dtype):
        return self.head


class _Set:
    """The engines, golden runs and per-row-count results of one shape set, built on first use."""

    def __init__(self, shape: str):
        self.shape, self.cfg = shape, E.SHAPE_SETS[shape]()
        self.src = _Drawn(self.cfg)
        self.ids = torch.randint(3, self.cfg.vocab_size, (SLOTS, P), generator=torch.Generator().manual_seed(5)).to(DEV)
        self._eng, self._gold, self._runs = {}, {}, {}
        self.tok = self.golden("bf16")["lg_p"].argmax(-1).to(torch.int32)  # the decode step's input, for every engine

    # ---- engines
    def _make(self, start=0, end=2, plain=False, **kw):
        kw = dict(ENGINE_KW, has_embed=True, has_head=True, source=self.src, **kw)
        if plain:
            return StageEngine(self.cfg, start, end, DEV, torch.bfloat16, **kw)
        return make_stage_engine(self.cfg, start, end, DEV, torch.bfloat16, **kw)

    def engine(self, name: str):
        if name not in self._eng:
            if name == "base":
                e = self._make()
            elif name in ("stage0", "stage1"):
                e = self._make(*((0, 1) if name == "stage0" else (1, 2)))
            elif name == "paged":
                e = self._make(kv_layout="paged")
            elif name in ("fp8", "int4"):
                e = self._make(weight_dtype=name)
            else:
                raise KeyError(name)
            self._eng[name] = e
        return self._eng[name]

    def twin(self, kind: str):
        """(plain StageEngine holding bf16(dequantise(quantise(w))), golden layers of the fp32
        dequantised weights); the quantised engine is checked to hold exactly quantise(w)."""
        key = "twin_" + kind
        if key not in self._eng:
            eq, t = self.engine(kind), self._make(plain=True)
            gold = []
            for lq, lt in zip(eq.layers, t.layers):
                deq = {}
                for name, (N, K) in zip(PROJ, StageEngine.proj_shapes(self.cfg)):
                    wp = getattr(lt, name)
                    w = packing.unpack_b(wp)
                    if kind == "fp8":
                        q, sc = packing.quantize_fp8_rows(w)
                        assert torch.equal(getattr(lq, name), packing.pack_b_fp8(q)) and torch.equal(getattr(lq, name + "_s"), sc)
                        deq[name] = packing.dequantize_fp8_rows(q, sc)
                    else:
                        q, sc = int4.quantize_int4_groups(w)
                        assert torch.equal(getattr(lq, name), int4.pack_b_int4(q))
                        assert torch.equal(getattr(lq, name + "_s"), int4.pack_scales_int4(sc))
                        deq[name] = int4.dequantize_int4_groups(q, sc)
                    wp.copy_(packing.pack_b(deq[name].to(torch.bfloat16)))
                gold.append(E.unfuse_layer(self.cfg, *(deq[n] for n in PROJ)))
            self._eng[key] = t
            self._gold[kind + "_layers"] = gold
        return self._eng[key]

    # ---- golden
    def golden(self, kind: str = "bf16") -> dict:
        """fp32 hidden states of all 512 sequences: ``hp`` [512, 2, H] after the prompt, ``hd``
        [512, H] after the decode step fed ``tok``; ``lg_p`` / ``lg_d`` the logits behind them."""
        if kind not in self._gold:
            if kind == "bf16":
                layers = self.src.layers
            else:
                self.twin(kind)
                layers = self._gold.pop(kind + "_layers")
            ref = ReferenceLlama(self.cfg, self.src.embed, layers, self.src.norm, self.src.head, max_pos=E.MAX_SEQ)
            ref.cos, ref.sin = ref.cos.to(DEV), ref.sin.to(DEV)
            hp = ref.forward_hidden(ref.embed[self.ids.long()])
            lg_p = ref.logits(hp[:, -1])
            tok = lg_p.argmax(-1) if kind == "bf16" else self.tok.long()
            hd = ref.forward_hidden(ref.embed[tok[:, None]])[:, -1]
            self._gold[kind] = dict(hp=hp, hd=hd, lg_p=lg_p, lg_d=ref.logits(hd))
            del ref
        return self._gold[kind]

    # ---- forwards
    def prefill(self, e, R: int) -> torch.Tensor:
        e.reset()
        slots = list(range(R))
        sl, po = e.prefill_rows(slots, [P] * R)
        h = e.forward(e.embed(self.ids[:R].reshape(-1)), sl, po).clone()
        e.advance(slots, [P] * R)
        return h

    @staticmethod
    def step_rows(e, R: int):
        slots = list(range(R))
        sl, po = e.prefill_rows(slots, [1] * R)
        if getattr(e, "paged", False):
            for s in slots:
                e.kv_reserve(s, P + 1)
        return e._i32(sl), e._i32(po)

    def eager_step(self, e, R: int, h=None) -> torch.Tensor:
        """The body a DecodeGraph captures, launched eagerly."""
        sl, po = self.step_rows(e, R)
        h = e.embed(self.tok[:R]) if h is None else h.clone()
        out = e._forward_hip(h, sl, po, None, R, nsplit=e.decode_nsplit(R)).clone()
        e.advance(list(range(R)), [1] * R)
        return out

    def static_run(self, R: int, skp: bool = True) -> dict:
        """The base engine's prefill and eager decode step (hidden states), with the gemm_skp route
        on (the default) or off; outside 385..512 rows the switch changes nothing."""
        skp = skp or not (SKP_MIN_ROWS <= R <= SKP_MAX_ROWS)
        if (R, skp) not in self._runs:
            e = self.engine("base")
            with _skp(skp):
                hp = self.prefill(e, R)
                self._runs[(R, skp)] = dict(hp=hp, hd=self.eager_step(e, R), plans=e.skp_plans(R))
        return self._runs[(R, skp)]


_SETS = {}


def _set(shape: str) -> _Set:
    if shape not in _SETS:
        _SETS[shape] = _Set(shape)
    return _SETS[shape]


@pytest.fixture(scope="module", autouse=True)
def _free_sets():
    yield
    _SETS.clear()
    torch.cuda.empty_cache()


def _cases(kind: str = "bf16", keep=lambda shape, R: True) -> list:
    return [pytest.param(shape, R, id=f"{shape}-{R}") for shape in sorted(E.SHAPE_SETS)
            for R in E.edge_rows(E.SHAPE_SETS[shape](), kind) if keep(shape, R)]


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype == torch.bfloat16
    if not torch.equal(a.view(torch.int16), b.view(torch.int16)):
        d = a.view(torch.int16) != b.view(torch.int16)
        rows = d.any(-1).nonzero().flatten()
        raise AssertionError(f"{what}: {int(d.sum())} of {d.numel()} bf16 values differ, in {rows.numel()} rows "
                             f"(first {rows[:8].tolist()}), rel err {float(rel_err(a, b)):.3e}")


# ------------------------------------------------------------------------------ golden
@pytest.mark.parametrize("shape,R", _cases())
def test_prefill_and_captured_step_vs_golden(shape, R):
    S = _set(shape)
    e, G = S.engine("base"), S.golden()
    hp = S.prefill(e, R)
    err = rel_err(hp.view(R, P, -1), G["hp"][:R])
    print(f"{shape} {R} rows: prefill {err!r}")
    assert err < TOL
    dg = DecodeGraph(e, R, "full", history_len=1)
    dg.tokens.copy_(S.tok[:R])
    dg.capture()
    dg.replay()
    torch.cuda.synchronize()
    err = rel_err(dg.out_hidden, G["hd"][:R])
    print(f"{shape} {R} rows: decode step {err!r}")
    assert err < TOL
    lg = G["lg_d"]
    top2 = lg.topk(2, dim=-1).values
    clear = (top2[:, 0] - top2[:, 1]) > 0.05 * lg.abs().amax(-1)
    assert bool(clear.any())  # (of the 512 sequences)
    got, want = dg.history[0].long(), lg.argmax(-1)[:R]
    assert bool((got[clear[:R]] == want[clear[:R]]).all())
    # the replay is the eager step, bit for bit
    _same(dg.out_hidden.clone(), S.static_run(R)["hd"], f"{shape} {R} rows: graph replay vs eager step")
    _same(hp, S.static_run(R)["hp"], f"{shape} {R} rows: the prefill, run twice")


def test_704_row_prefill_vs_golden():
    """704 rows (352 two-token prompts) of the 7B shapes: the down projection's tuned row counts
    640 and 768 are equally far, so the partial planner's tie rule decides this forward."""
    S = _set("7b")
    e, R = S.engine("base"), 352
    assert e.part_k is not None and 704 <= e.part_k.shape[1]
    calls = []
    real = hip.gemm_sk_partial_plan
    hip.gemm_sk_partial_plan = lambda *a: (calls.append(a), real(*a))[1]
    try:
        hp = S.prefill(e, R)
    finally:
        hip.gemm_sk_partial_plan = real
    assert (704, 4096, 11008) in calls
    err = rel_err(hp.view(R, P, -1), S.golden()["hp"][:R])
    print(f"7b 704-row prefill: {err!r}")
    assert err < TOL


# ------------------------------------------------------------------------------ bitwise twins
@pytest.mark.parametrize("shape,R", _cases())
def test_two_stages_equal_one(shape, R):
    """engine.py: "a layer range computes the same bits whichever stage it starts"."""
    S = _set(shape)
    e0, e1, one = S.engine("stage0"), S.engine("stage1"), S.static_run(R)
    h0 = S.prefill(e0, R)
    e1.reset()
    slots = list(range(R))
    sl, po = e1.prefill_rows(slots, [P] * R)
    hp = e1.forward(h0, sl, po).clone()
    e1.advance(slots, [P] * R)
    _same(hp, one["hp"], f"{shape} {R} rows ({E.describe(S.cfg, 2 * R)}): prefill through two stages")
    hd = S.eager_step(e1, R, h=S.eager_step(e0, R))
    _same(hd, one["hd"], f"{shape} {R} rows ({E.describe(S.cfg, R)}): decode step through two stages")


@pytest.mark.parametrize("shape,R", _cases("paged"))
def test_paged_equals_static(shape, R):
    """A shuffled page pool; both shape sets have one query head per KV head, where the paged
    engine promises the static engine's bits. It does not take the gemm_skp route."""
    S = _set(shape)
    ep, one = S.engine("paged"), S.static_run(R, skp=False)
    ep.reset()
    _shuffle_pool(ep, R)
    _same(S.prefill(ep, R), one["hp"], f"{shape} {R} rows: paged prefill")
    _same(S.eager_step(ep, R), one["hd"], f"{shape} {R} rows: paged decode step")
    pages = [p for s in range(R) for p in ep.pool.pages_of(s)]
    assert len(set(pages)) == R and 0 not in pages and (R < 16 or sorted(pages) != pages)


@pytest.mark.parametrize("shape,R", _cases(keep=lambda shape, R: SKP_MIN_ROWS <= R <= SKP_MAX_ROWS))
def test_skp_route_on_and_off(shape, R):
    S = _set(shape)
    cfg = S.cfg
    on, off = S.static_run(R, skp=True), S.static_run(R, skp=False)
    assert off["plans"] is None
    _same(on["hp"], off["hp"], f"{shape} {R} rows: the prefill does not take the route")
    plans = on["plans"] or (None, None)
    assert shape != "7b" or any(plans)  # ops/skp_tuning.txt lists the 7B residual projections
    shapes = ((cfg.hidden_size, cfg.q_size), (cfg.hidden_size, cfg.intermediate_size))
    same_bits = all(p is None or _sk_equal_ranges(hip, R, N, K) == p[:3] for (N, K), p in zip(shapes, plans))
    if same_bits:
        _same(on["hd"], off["hd"], f"{shape} {R} rows: gemm_skp {plans} keeps gemm_sk's tile and split")
    else:
        assert rel_err(on["hd"], off["hd"]) < TOL


# ------------------------------------------------------------------------------ quantised weights
def _quant_cases():
    return [pytest.param(kind, shape, R, id=f"{kind}-{shape}-{R}") for kind in ("fp8", "int4")
            for shape in sorted(E.SHAPE_SETS) for R in E.edge_rows(E.SHAPE_SETS[shape](), kind)]


@pytest.mark.parametrize("kind,shape,R", _quant_cases())
def test_quantised_engine(kind, shape, R):
    S = _set(shape)
    eq, t = S.engine(kind), S.twin(kind)
    hp, hd = S.prefill(eq, R), S.eager_step(eq, R)
    if 2 * R > packing.GEMV_MAX_ROWS:  # the prefill runs the bf16 kernels on the dequantised weights
        _same(hp, S.prefill(t, R), f"{kind} {shape} {R} rows: prefill vs the bf16 twin")
    if R > packing.GEMV_MAX_ROWS:
        _same(hd, S.eager_step(t, R), f"{kind} {shape} {R} rows: decode step vs the bf16 twin")
        return
    G = S.golden(kind)
    e_p, e_d = rel_err(hp.view(R, P, -1), G["hp"][:R]), rel_err(hd, G["hd"][:R])
    print(f"{kind} {shape} {R} rows: prefill {e_p!r}\n{kind} {shape} {R} rows: decode step {e_d!r}")
    assert e_p < TOL and e_d < TOL
