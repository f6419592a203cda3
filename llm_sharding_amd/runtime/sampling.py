"""Seeded temperature / top-k / top-p sampling on top of :class:`StageEngine`.

Greedy decode (``StageEngine.head``, ``DecodeGraph``) is untouched: everything here is an extra
path that exists only when a request asks for it.

* :class:`SamplingParams` - one request's ``temperature / top_k / top_p / seed``.
* :class:`Sampler` - bf16 logits of selected rows through the existing lm_head kernels
  (``EPI_STORE``) and one sampled token per row (``ops.sampling.sample``; the fp64 reference on
  a CPU engine). Used for the first token after a prefill.
* :class:`SamplingDecodeGraph` - a :class:`DecodeGraph` whose step ends in logits ->
  ``lsa_sample`` -> ``argmax_finalize`` instead of the fused argmax, with per-row parameters on
  the device (:meth:`SamplingDecodeGraph.set_params` between replays).
* :class:`EagerSamplingDecode` - the same interface for CPU engines.
* Logit stages (:mod:`.logit_stages`, re-exported here): :class:`PenaltyState`,
  :class:`GrammarState` and :class:`ConstraintState`, optional per-slot state that edits the logits
  between the lm_head and the draw. Each exists only once a request asks for it, and a Sampler or
  graph built without one runs exactly the code above. Their order is defined once, in
  ``logit_stages.STAGE_CLASSES``; the stages are followed by sample -> finalise -> logprobs.
* Log-probabilities (``SamplingParams.logprobs``, ``ops.logprobs``): :meth:`Sampler.logprobs`,
  ``SamplingDecodeGraph(..., logprobs=True)`` (one ``lsa_logprobs`` launch behind
  ``argmax_finalize``; a graph built without it captures exactly the step above) and
  :func:`score_prompt`. The numbers describe the bf16 row ``lsa_sample`` reads: after the
  stages, before temperature and the top-k / top-p filters.

A request's tokens depend only on its own logits, seed and positions (the noise is a pure
function of seed, position and vocabulary index), not on the row, slot or batch it runs in.
"""
from __future__ import annotations

import math
import numbers
import os
from dataclasses import dataclass
from typing import Any, Optional, Sequence

import torch

from ..ops import constraints as K
from ..ops import grammar as G
from ..ops import logprobs as LP
from ..ops import sampling as S
from .engine import DecodeGraph, EagerDecode, StageEngine
from .logit_stages import (STAGE_CLASSES, CompiledConstraint, ConstraintState, GrammarState,  # noqa: F401
                           PenaltyState, _check_full_head, check_vocab_cache, compile_constraints, ordered_stages)


@dataclass
class SamplingParams:
    """``temperature == 0`` is greedy (the filters are then ignored). ``top_k == 0`` and
    ``top_p == 1`` switch the filters off. ``seed=None`` draws 64 bits from ``os.urandom`` and
    stores them, so any run can be replayed from ``params.seed``. ``repetition_penalty`` (HF's,
    over prompt + generated tokens; 1 = off), ``presence_penalty`` and ``frequency_penalty``
    (OpenAI / vLLM's, over generated tokens; 0 = off) edit the logits before the filters and the
    draw - also at temperature 0, which then takes the arg-max of the penalised logits.
    ``logprobs`` (None = off): ``0`` returns the chosen token's log-probability and rank, ``1..20``
    also that many most likely alternatives - of the penalised logits at temperature 1, before the
    top-k / top-p filters.

    Constrained decoding (``ops.constraints``; every field off by default): ``logit_bias`` (token ->
    a finite value or ``-inf``, added to the logit) and ``banned_token_ids`` (a bias of ``-inf``)
    share 320 entries; ``min_tokens`` masks every EOS id of the configuration until that many
    tokens have been generated; ``min_p`` in (0, 1] masks tokens with ``p_i < min_p * p_max`` at
    the request's temperature (ignored at temperature 0); ``allowed_token_ids`` (only these tokens
    - include EOS if the output may end), ``choices`` (the output is exactly one of these token-id
    sequences, then EOS) and ``automaton`` (an explicit :class:`ops.constraints.TokenAutomaton`,
    the hook of an external regex / grammar compiler) exclude one another, and ``banned_token_ids``,
    a ``-inf`` bias and ``min_tokens``: the automaton decides what may appear and when the output
    ends, so a row can never lose every column.

    ``regex`` (``ops.grammar``): the output, as bytes, fully matches this pattern - compiled here
    into a byte-level DFA (:attr:`grammar`), so a syntax error surfaces at construction. It excludes
    ``allowed_token_ids``, ``choices``, ``automaton``, ``banned_token_ids``, a ``-inf`` bias and
    ``min_tokens`` for the same reason; a finite ``logit_bias``, ``min_p``, the penalties, top-k /
    top-p and ``logprobs`` combine with it.

    ``json_object`` (``ops.pda``): the output, as bytes, is one JSON object (RFC 8259, whitespace
    runs bounded by the server's ``json_max_ws``, nesting up to 64), then EOS - OpenAI's
    ``response_format: {"type": "json_object"}``. It excludes ``regex`` and what ``regex``
    excludes, for the same reason, and combines with what ``regex`` combines with; at temperature 0
    the request still takes the sampling path (the arg-max of the masked logits)."""
    temperature: float = 0.0
    top_k: int = 0
    top_p: float = 1.0
    seed: Optional[int] = None
    repetition_penalty: float = 1.0
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    logprobs: Optional[int] = None
    logit_bias: Optional[dict] = None
    banned_token_ids: Optional[list] = None
    min_tokens: int = 0
    min_p: Optional[float] = None
    allowed_token_ids: Optional[list] = None
    choices: Optional[list] = None
    automaton: Optional[Any] = None
    regex: Optional[str] = None
    json_object: bool = False

    def __post_init__(self):
        self._check_constraints()
        self._grammar = None
        if not isinstance(self.json_object, bool):
            raise ValueError(f"json_object must be a bool, got {self.json_object!r}")
        if self.json_object:
            clash = [k for k in ("regex", "allowed_token_ids", "choices", "automaton", "banned_token_ids")
                     if getattr(self, k) is not None]
            if self.min_tokens:
                clash.append("min_tokens")
            if any(b == float("-inf") for _, b in self.bias_entries()) and "banned_token_ids" not in clash:
                clash.append("a -inf bias")
            if clash:
                raise ValueError(f"json_object cannot be combined with {' / '.join(clash)}: the JSON grammar decides "
                                 "what may appear and when the output ends")
        if self.regex is not None:
            if not isinstance(self.regex, str):
                raise ValueError(f"regex must be a str, got {self.regex!r}")
            clash = [k for k in ("allowed_token_ids", "choices", "automaton", "banned_token_ids")
                     if getattr(self, k) is not None]
            if self.min_tokens:
                clash.append("min_tokens")
            if any(b == float("-inf") for _, b in self.bias_entries()) and "banned_token_ids" not in clash:
                clash.append("a -inf bias")
            if clash:
                raise ValueError(f"regex cannot be combined with {' / '.join(clash)}: the pattern decides what may "
                                 "appear and when the output ends")
            self._grammar = _compile_regex(self.regex)
        self.temperature, self.top_k, self.top_p = float(self.temperature), int(self.top_k), float(self.top_p)
        if not self.temperature >= 0.0 or self.temperature == float("inf"):
            raise ValueError(f"temperature must be a finite value >= 0, got {self.temperature}")
        if self.top_k < 0 or self.top_k >= 1 << 31:
            raise ValueError(f"top_k must be >= 0 (0 = off), got {self.top_k}")
        if not 0.0 < self.top_p <= 1.0:
            raise ValueError(f"top_p must be in (0, 1], got {self.top_p}")
        if self.seed is None:
            self.seed = int.from_bytes(os.urandom(8), "little")
        self.seed = int(self.seed)
        if not 0 <= self.seed < 1 << 64:
            raise ValueError(f"seed must be a 64-bit unsigned value, got {self.seed}")
        self.repetition_penalty = float(self.repetition_penalty)
        self.presence_penalty, self.frequency_penalty = float(self.presence_penalty), float(self.frequency_penalty)
        if not 0.0 < self.repetition_penalty < float("inf"):
            raise ValueError(f"repetition_penalty must be a finite value > 0 (1 = off), got {self.repetition_penalty}")
        for k in ("presence_penalty", "frequency_penalty"):
            if not abs(getattr(self, k)) < float("inf"):
                raise ValueError(f"{k} must be finite (0 = off), got {getattr(self, k)}")
        if self.logprobs is not None:
            lp = self.logprobs
            if isinstance(lp, bool) or not isinstance(lp, numbers.Integral) or not 0 <= lp <= LP.TOP_MAX:
                raise ValueError(f"logprobs must be None (off) or an integer in [0, {LP.TOP_MAX}], got {lp!r}")
            self.logprobs = int(lp)

    @property
    def greedy(self) -> bool:
        return self.temperature == 0.0

    @property
    def penalized(self) -> bool:
        return self.repetition_penalty != 1.0 or self.presence_penalty != 0.0 or self.frequency_penalty != 0.0

    def _check_constraints(self) -> None:
        """The checks of the constraint fields that need no vocabulary (``compile_constraints``
        does the rest against a configuration)."""
        def ids(x, what):
            if isinstance(x, (str, bytes)) or not hasattr(x, "__iter__"):
                raise ValueError(f"{what} must be a list of token ids, got {x!r}")
            out = []
            for t in x:
                if isinstance(t, bool) or not isinstance(t, numbers.Integral) or t < 0:
                    raise ValueError(f"{what}: token ids are integers >= 0, got {t!r}")
                out.append(int(t))
            return out

        if self.logit_bias is not None:
            if not isinstance(self.logit_bias, dict):
                raise ValueError(f"logit_bias must be a dict of token id -> bias, got {self.logit_bias!r}")
            lb = {}
            for k, v in self.logit_bias.items():
                try:
                    t, b = int(k), float(v)
                except (TypeError, ValueError):
                    raise ValueError(f"logit_bias: token id -> number, got {k!r}: {v!r}") from None
                if t < 0 or isinstance(k, (bool, float)):
                    raise ValueError(f"logit_bias: token ids are integers >= 0, got {k!r}")
                if math.isnan(b) or b == float("inf"):
                    raise ValueError(f"logit_bias[{t}] must be finite or -inf, got {b}")
                lb[t] = b
            self.logit_bias = lb or None
        if self.banned_token_ids is not None:
            self.banned_token_ids = sorted(set(ids(self.banned_token_ids, "banned_token_ids"))) or None
        if len(self.bias_entries()) > K.BIAS_MAX:
            raise ValueError(f"logit_bias and banned_token_ids together hold {len(self.bias_entries())} entries, more "
                             f"than {K.BIAS_MAX}")
        mt = self.min_tokens
        if isinstance(mt, bool) or not isinstance(mt, numbers.Integral) or not 0 <= mt < 1 << 30:
            raise ValueError(f"min_tokens must be an integer >= 0, got {mt!r}")
        self.min_tokens = int(mt)
        if self.min_p is not None:
            self.min_p = float(self.min_p)
            if not 0.0 < self.min_p <= 1.0:
                raise ValueError(f"min_p must be in (0, 1], got {self.min_p}")
        if self.allowed_token_ids is not None:
            self.allowed_token_ids = sorted(set(ids(self.allowed_token_ids, "allowed_token_ids")))
            if not self.allowed_token_ids:
                raise ValueError("allowed_token_ids: at least one token")
        if self.choices is not None:
            if isinstance(self.choices, (str, bytes)) or not hasattr(self.choices, "__iter__"):
                raise ValueError("choices must be a list of token-id sequences")
            self.choices = [ids(c, "choices") for c in self.choices]
            if not self.choices or any(not c for c in self.choices):
                raise ValueError("choices: at least one choice, and no empty choice")
        if self.automaton is not None and not isinstance(self.automaton, K.TokenAutomaton):
            raise ValueError("automaton must be an ops.constraints.TokenAutomaton")
        kinds = [k for k in ("allowed_token_ids", "choices", "automaton") if getattr(self, k) is not None]
        if len(kinds) > 1:
            raise ValueError(f"at most one of allowed_token_ids / choices / automaton, got {kinds}")
        if kinds and (self.min_tokens or any(b == float("-inf") for _, b in self.bias_entries())):
            raise ValueError(f"{kinds[0]} cannot be combined with banned_token_ids, a -inf bias or min_tokens: the "
                             "automaton decides what may appear and when the output ends")

    def bias_entries(self) -> list:
        """``[(token, bias)]`` of ``logit_bias`` and ``banned_token_ids`` (``-inf``; a ban wins),
        distinct tokens in ascending order."""
        e = dict(self.logit_bias or {})
        e.update({int(t): float("-inf") for t in self.banned_token_ids or ()})
        return sorted(e.items())

    @property
    def constrained(self) -> bool:
        """Any constraint field is on: the request needs a :class:`ConstraintState`."""
        return bool(self.logit_bias or self.banned_token_ids or self.min_tokens or self.min_p is not None
                    or self.allowed_token_ids is not None or self.choices is not None or self.automaton is not None)

    @property
    def grammar(self):
        """The compiled :class:`ops.grammar.ByteDFA` of ``regex`` (None without one): the request
        needs a :class:`GrammarState`."""
        return self._grammar

    @property
    def plain(self) -> bool:
        """Needs no sampling path at all: temperature 0, every penalty off, no logprobs, no
        constraint, no regex, no json_object."""
        return (self.greedy and not self.penalized and self.logprobs is None and not self.constrained
                and self._grammar is None and not self.json_object)

    @property
    def n_top(self) -> int:
        """The row's ``n_top`` of ``lsa_logprobs``: -1 (skip the row) without ``logprobs``."""
        return -1 if self.logprobs is None else self.logprobs

    @classmethod
    def from_dict(cls, d: dict) -> Optional["SamplingParams"]:
        """``temperature / top_k / top_p / seed / repetition_penalty / presence_penalty /
        frequency_penalty / logprobs / logit_bias / banned_token_ids / min_tokens / min_p /
        allowed_token_ids / choices / regex / json_object`` keys of a request dict (``logit_bias`` with string or
        integer keys), and ``response_format: {"type": "json_object"}`` (``"text"``: nothing; any
        other type: ValueError); None (greedy) when none of them is present."""
        keys = ("temperature", "top_k", "top_p", "seed", "repetition_penalty", "presence_penalty", "frequency_penalty",
                "logprobs", "logit_bias", "banned_token_ids", "min_tokens", "min_p", "allowed_token_ids", "choices",
                "regex", "json_object")
        kw = {k: d[k] for k in keys if d.get(k) is not None and not (k == "json_object" and d[k] is False)}
        fmt = d.get("response_format")
        if fmt is not None:
            kind = fmt.get("type") if isinstance(fmt, dict) else None
            if kind == "json_object":
                kw["json_object"] = True
            elif kind != "text":
                raise ValueError(f"response_format: {{'type': 'json_object'}} or {{'type': 'text'}}, got {fmt!r}")
        if not kw:
            return None
        return cls(**kw)


_REGEX_CACHE: dict = {}


def _compile_regex(pattern: str):
    """``ByteDFA.from_regex`` behind a small cache: a ByteDFA is immutable, and servers see the same
    patterns again and again."""
    dfa = _REGEX_CACHE.get(pattern)
    if dfa is None:
        dfa = G.ByteDFA.from_regex(pattern)
        if len(_REGEX_CACHE) >= 256:
            _REGEX_CACHE.pop(next(iter(_REGEX_CACHE)))
        _REGEX_CACHE[pattern] = dfa
    return dfa


GREEDY = SamplingParams(0.0, 0, 1.0, 0)


class Sampler:
    """Logits and sampled tokens of a stage that holds the whole lm_head. ``penalties``,
    ``constraints``, ``grammar``: its logit stages (:mod:`.logit_stages`), applied by :meth:`sample`
    to the rows given ``slots``, in the stages' one order."""

    def __init__(self, eng: StageEngine, penalties: Optional[PenaltyState] = None,
                 constraints: Optional[ConstraintState] = None, grammar: Optional[GrammarState] = None):
        _check_full_head(eng)
        self.eng, self.penalties, self.constraints, self.grammar = eng, penalties, constraints, grammar

    # ------------------------------------------------------------------ logits
    def logits(self, h: torch.Tensor, rows_idx=None) -> torch.Tensor:
        """final norm -> lm_head of the selected rows: bf16 ``[n, head_rows]`` (columns
        ``>= vocab_size`` are padding)."""
        eng = self.eng
        if rows_idx is None:
            rows_idx = list(range(h.shape[0]))
        if not eng.gpu:
            hs = h[torch.as_tensor(rows_idx, device=h.device, dtype=torch.long)]
            return eng.logits_torch(hs).to(torch.bfloat16)
        idx = eng._i32(rows_idx)
        out = torch.empty((idx.numel(), eng.cfg.head_rows), dtype=torch.bfloat16, device=eng.device)
        self.logits_into(h, idx.numel(), out, a_rows=idx)
        return out

    def logits_into(self, h: torch.Tensor, rows: int, out: torch.Tensor, a_rows: Optional[torch.Tensor] = None) -> None:
        """GPU: logits of ``rows`` rows of ``h`` (``a_rows``: int32 row gather) into bf16 ``out``
        [>= rows, head_rows], on the existing projection kernels with the EPI_STORE epilogue -
        the kernel family per row count mirrors ``StageEngine.head_gemv``."""
        from ..ops import hip
        eng, cfg = self.eng, self.eng.cfg
        N, H, eps, D = cfg.head_rows, cfg.hidden_size, cfg.rms_norm_eps, eng.DECODE_MAX_ROWS
        if out.dtype != torch.bfloat16 or out.shape[0] < rows or out.shape[1] != N:
            raise ValueError(f"logits_into: out must be bf16 [>= {rows}, {N}]")
        ep = hip.make_epi(out=out, ldo=out.stride(0), bias=eng.head_bias)
        if rows > D and (not cfg.is_gpt2 and eng.lm_head_s is None and eng.sk_ws is not None and N % 128 == 0
                         and rows <= eng.buf_xn.shape[0]):
            xn = eng.buf_xn[:rows]
            src = h[:rows] if a_rows is None else h.index_select(0, a_rows.long())
            hip.rmsnorm(src, None, xn, rows, eps, H)
            hip.gemm_sk(xn, eng.lm_head, rows, N, H, hip.EPI_STORE, ep, ws=eng.sk_ws)
            return
        if rows > D:  # the GEMV kernels take <= 128 rows per launch
            for c0 in range(0, rows, D):
                c = min(D, rows - c0)
                if a_rows is None:
                    self.logits_into(h[c0:c0 + c], c, out[c0:c0 + c])
                else:
                    self.logits_into(h, c, out[c0:c0 + c], a_rows=a_rows[c0:c0 + c])
            return
        if cfg.is_gpt2:  # ln_f (mean + bias) runs as its own kernel in front of a plain GEMV
            xn = eng.buf_xn[:rows]
            src = h if a_rows is None else h.index_select(0, a_rows.long())
            hip.layernorm(src, xn, eng.final_norm, eng.final_norm_b, rows, eps)
            if eng.lm_head_s is not None:
                hip.proj_fp8(xn, eng.lm_head.view(-1), eng.lm_head_s, rows, N, H, hip.EPI_STORE, ep, ws=eng.coop_ws)
            else:
                hip.gemv(xn, eng.lm_head, rows, N, H, hip.EPI_STORE, ep, ws=eng.coop_ws)
            return
        if eng.lm_head_s is not None:
            hip.proj_fp8(h, eng.lm_head.view(-1), eng.lm_head_s, rows, N, H, hip.EPI_STORE, ep, norm=True, eps=eps,
                         a_rows=a_rows, ws=eng.coop_ws)
        else:
            hip.gemv(h, eng.lm_head, rows, N, H, hip.EPI_STORE, ep, ws=eng.coop_ws, norm=True, eps=eps, a_rows=a_rows)

    # ------------------------------------------------------------------ tokens
    def sample_logits(self, logits: torch.Tensor, params_list: Sequence[SamplingParams], positions) -> torch.Tensor:
        """One token per row of bf16 ``logits`` [n, >= vocab_size]; ``positions[i]`` is the
        position the sampled token will occupy (its Philox counter). Returns int64 [n]."""
        eng, V = self.eng, self.eng.cfg.vocab_size
        n = logits.shape[0]
        positions = [int(p) for p in (positions.tolist() if isinstance(positions, torch.Tensor) else positions)]
        if len(params_list) != n or len(positions) != n:
            raise ValueError(f"sample: {n} rows, {len(params_list)} params, {len(positions)} positions")
        if not eng.gpu:
            tok, _, _, _ = S.sample_reference(logits.to(torch.bfloat16), V, [p.temperature for p in params_list],
                                              [p.top_k for p in params_list], [p.top_p for p in params_list],
                                              [p.seed for p in params_list], positions)
            return torch.from_numpy(tok)
        from ..ops import hip
        dev = eng.device
        arr = device_params(params_list, dev)
        ctr = torch.tensor(positions, dtype=torch.int32, device=dev)
        keys = torch.zeros(n, dtype=torch.int64, device=dev)
        S.sample(logits, V, n, arr["temperature"], arr["top_k"], arr["top_p"], arr["seed"], ctr, keys)
        out = torch.empty(n, dtype=torch.int32, device=dev)
        for c0 in range(0, n, 1024):  # argmax_finalize takes <= 1024 rows
            c = min(1024, n - c0)
            hip.argmax_finalize(keys[c0:c0 + c], c, out[c0:c0 + c])
        return out.long()

    def logprobs(self, logits: torch.Tensor, targets, n_top) -> LP.Logprobs:
        """Log-probabilities of bf16 ``logits`` [n, >= vocab_size] (``ops.logprobs``' contract):
        ``targets`` / ``n_top`` per row (or one value for all). ``lsa_logprobs`` on the GPU, the
        fp64 reference on a CPU engine. Returns :class:`ops.logprobs.Logprobs` of torch tensors on
        the logits' device: ``lse`` / ``tok_lp`` fp32 [n], ``tok_rank`` int32 [n], ``top_id`` int32
        and ``top_lp`` fp32 [n, TOP_MAX]; rows with ``n_top = -1`` hold NaN / 0 / -1 / -inf."""
        eng, V, n = self.eng, self.eng.cfg.vocab_size, logits.shape[0]

        def per_row(x):
            x = x.tolist() if isinstance(x, torch.Tensor) else x
            x = [int(v) for v in x] if isinstance(x, (list, tuple)) else [int(x)] * n
            if len(x) != n:
                raise ValueError(f"logprobs: {len(x)} per-row values for {n} rows")
            return x

        targets, n_top = per_row(targets), per_row(n_top)
        if any(k > LP.TOP_MAX for k in n_top):
            raise ValueError(f"logprobs: n_top above {LP.TOP_MAX}")
        if not eng.gpu:
            ref = LP.logprobs_reference(logits.to(torch.bfloat16), V, n_top, targets)
            return LP.Logprobs(torch.from_numpy(ref.lse).float(), torch.from_numpy(ref.tok_lp).float(),
                               torch.from_numpy(ref.tok_rank).int(), torch.from_numpy(ref.top_id).int(),
                               torch.from_numpy(ref.top_lp).float())
        dev = eng.device
        out = LP.alloc_outputs(n, dev)
        nt = torch.tensor(n_top, dtype=torch.int32, device=dev)
        tg = torch.tensor(targets, dtype=torch.int32, device=dev)
        for c0 in range(0, n, 32768):
            c = min(32768, n - c0)
            LP.logprobs(logits[c0:c0 + c], V, c, nt[c0:c0 + c], tg[c0:c0 + c],
                        LP.Logprobs(*(t[c0:c0 + c] for t in out)))
        return out

    def sample(self, h: torch.Tensor, rows_idx, params_list: Sequence[SamplingParams], positions,
               slots=None, tokens_in=None, return_logprobs: bool = False):
        """Sampled tokens (int64 [n]) of the selected rows of the final hidden ``h``: the first
        token after a prefill uses ``positions[i]`` = the prompt length. ``slots`` (with a logit
        stage): row i belongs to sequence slot ``slots[i]`` and is edited first by every stage one of
        the rows' parameters asks for (:mod:`.logit_stages`, in their order); ``tokens_in[i]`` is the
        token the row's step was fed - None for the first token after a prefill, which only sees the prompt.
        ``return_logprobs``: returns ``(tokens, Logprobs)`` - the log-probabilities of the sampled
        tokens under the edited logits, for the rows whose parameters ask for them."""
        logits = self.logits(h, rows_idx)
        for cls in STAGE_CLASSES:
            if any(cls.wants(p) for p in params_list):
                stage = getattr(self, cls.name)
                if stage is None or slots is None:
                    raise RuntimeError(cls.needs())
                logits = stage.apply(logits, slots, tokens_in, params_list=params_list, positions=positions)
        tok = self.sample_logits(logits, params_list, positions)
        if not return_logprobs:
            return tok
        return tok, self.logprobs(logits, tok, [p.n_top for p in params_list])


def device_params(params_list: Sequence[SamplingParams], device) -> dict:
    """Per-row device arrays of ``lsa_sample``."""
    return {
        "temperature": torch.tensor([p.temperature for p in params_list], dtype=torch.float32, device=device),
        "top_k": torch.tensor([p.top_k for p in params_list], dtype=torch.int32, device=device),
        "top_p": torch.tensor([p.top_p for p in params_list], dtype=torch.float32, device=device),
        "seed": torch.tensor([S.seed_to_i64(p.seed) for p in params_list], dtype=torch.int64, device=device),
    }


class SamplingDecodeGraph(DecodeGraph):
    """A captured decode step that samples: ... layers -> bf16 logits -> ``lsa_sample`` ->
    ``argmax_finalize`` (modes ``"full"`` and ``"last"``). Every row starts greedy
    (``temperature`` 0: the arg-max of the bf16 logits); :meth:`set_params` writes a row's
    parameters between replays. The row's Philox counter is its device position + 1 - the
    position the sampled token will occupy - so no host work happens per token.

    With ``penalties``, ``grammar`` or ``constraints`` (logit stages that cover this graph's slots,
    :mod:`.logit_stages`) the step holds one launch per stage between the logits and ``lsa_sample``,
    in the stages' order, on the step's input tokens (``self.tokens``) and the per-slot device
    tables; rows whose slots hold nothing for a stage are skipped by its kernel, and the
    log-probabilities describe the edited row. ``debug_raw`` keeps a captured copy of the unedited
    logits in ``raw_logits``.

    With ``logprobs=True`` the step ends in one more launch, ``lsa_logprobs`` on the same logits
    with the freshly written ``self.tokens`` as targets: the per-row ``n_top`` (-1 = the row is
    skipped, written by :meth:`set_params`) and the outputs ``lp`` (:class:`ops.logprobs.Logprobs`)
    live on the device; with a token history, ``lp_history`` keeps ``tok_lp`` of the same steps
    (NaN where a row was skipped).

    Without any one of them the captured step is exactly what it would be if that one did not exist.
    The logits buffer (``rows x head_rows`` bf16, 32 MB at 512 x 32000) is allocated only here."""

    def __init__(self, eng: StageEngine, rows: int, mode: str, slots: Optional[list] = None,
                 history_len: int = 0, scratch: int = 0, penalties: Optional[PenaltyState] = None,
                 debug_raw: bool = False, logprobs: bool = False, constraints: Optional[ConstraintState] = None,
                 grammar: Optional[GrammarState] = None):
        if mode not in ("full", "last"):
            raise ValueError("SamplingDecodeGraph runs the head: mode 'full' or 'last'")
        self.sampler = Sampler(eng, penalties, constraints, grammar)
        super().__init__(eng, rows, mode, slots=slots, history_len=history_len, scratch=scratch)
        dev = eng.device
        self.params = [GREEDY] * rows
        for k, v in device_params(self.params, dev).items():
            setattr(self, k, v)
        self.logits = torch.zeros((rows, eng.cfg.head_rows), dtype=torch.bfloat16, device=dev)
        self.raw_logits = torch.zeros_like(self.logits) if debug_raw else None
        self.penalties, self.constraints, self.grammar = penalties, constraints, grammar
        self.stages = ordered_stages(penalties, constraints, grammar)
        self.stage_rows = {}  # stage name -> its per-row device arrays
        for st in self.stages:
            st.check_covers(eng, self.slots, rows)
            self.stage_rows[st.name] = st.device_rows(self.params, dev)
        self.lp = self.n_top = self.lp_history = None
        if logprobs:
            self.n_top = torch.full((rows,), -1, dtype=torch.int32, device=dev)
            self.lp = LP.alloc_outputs(rows, dev)
            if self.history is not None:
                self.lp_history = torch.full(self.history.shape, float("nan"), dtype=torch.float32, device=dev)

    def set_params(self, row: int, params: Optional[SamplingParams]) -> None:
        """Small host-to-device copies on the current stream (like ``set_positions``)."""
        p = _checked_params(self, params)
        self.params[row] = p
        self.temperature[row] = p.temperature
        self.top_k[row] = p.top_k
        self.top_p[row] = p.top_p
        self.seed[row] = S.seed_to_i64(p.seed)
        for st in self.stages:
            st.write_row(self.stage_rows[st.name], row, p)
        if self.lp is not None:
            self.n_top[row] = p.n_top

    def capture(self, warmup: bool = True) -> "SamplingDecodeGraph":
        """The warm-up run advances the stages' per-slot state (token counts, automaton and DFA
        states): the graph's rows are restored."""
        idx = self.slot.long()
        saved = [st.snapshot(idx) for st in self.stages]
        super().capture(warmup)
        for st, kept in zip(self.stages, saved):
            st.restore(idx, kept)
        if self.lp_history is not None:
            self.lp_history.fill_(float("nan"))
        return self

    def _step(self) -> None:
        hip, eng, rows = self._hip, self.eng, self.rows
        h = eng.buf_h[:rows]
        if self.mode == "full":
            hip.embed(self.tokens, eng.embed_w, h)
        else:
            h.copy_(self.h_in)
        eng._forward_hip(h, self.slot, self.pos, None, rows, nsplit=eng.decode_nsplit(rows))
        self.sampler.logits_into(h, rows, self.logits)
        if self.raw_logits is not None:
            self.raw_logits.copy_(self.logits)
        for st in self.stages:
            st.launch(self)
        S.sample(self.logits, eng.cfg.vocab_size, rows, self.temperature, self.top_k, self.top_p, self.seed, self.pos,
                 self.keys, ctr_add=1)
        hip.argmax_finalize(self.keys, rows, self.tokens, self.pos, 1, self.history,
                            self.step_ctr if self.history is not None else None)
        if self.lp is not None:
            LP.logprobs(self.logits, eng.cfg.vocab_size, rows, self.n_top, self.tokens, self.lp,
                        lp_history=self.lp_history, step_ctr=self.step_ctr if self.lp_history is not None else None)


def _checked_params(graph, params: Optional[SamplingParams]) -> SamplingParams:
    """``params`` (None: greedy), or RuntimeError: they need a stage or logprobs ``graph`` lacks."""
    p = GREEDY if params is None else params
    owner = type(graph).__name__
    for cls in STAGE_CLASSES:
        if cls.wants(p) and getattr(graph, cls.name) is None:
            raise RuntimeError(cls.needs(owner))
    if p.logprobs is not None and graph.lp is None:
        raise RuntimeError(f"a request with logprobs needs {owner}(..., logprobs=True)")
    return p


class EagerSamplingDecode(EagerDecode):
    """:class:`SamplingDecodeGraph`'s interface on devices without graphs (CPU engines)."""

    def __init__(self, eng: StageEngine, rows: int, mode: str, slots: Optional[list] = None, history_len: int = 0,
                 penalties: Optional[PenaltyState] = None, logprobs: bool = False,
                 constraints: Optional[ConstraintState] = None, grammar: Optional[GrammarState] = None):
        if mode not in ("full", "last"):
            raise ValueError("EagerSamplingDecode runs the head: mode 'full' or 'last'")
        super().__init__(eng, rows, mode, slots=slots, history_len=history_len)
        self.sampler = Sampler(eng, penalties, constraints, grammar)
        self.penalties, self.constraints, self.grammar = penalties, constraints, grammar
        self.stages = ordered_stages(penalties, constraints, grammar)
        self.params = [GREEDY] * rows
        self.lp = self.lp_history = None
        if logprobs:
            self.lp = self.sampler.logprobs(torch.zeros((rows, eng.cfg.head_rows), dtype=torch.bfloat16), 0, -1)
            if self.history is not None:
                self.lp_history = torch.full(self.history.shape, float("nan"), dtype=torch.float32)

    def set_params(self, row: int, params: Optional[SamplingParams]) -> None:
        self.params[row] = _checked_params(self, params)

    def _body(self) -> None:
        eng = self.eng
        h = eng.embed(self.tokens) if self.mode == "full" else self.h_in
        slot, pos = eng.prefill_rows(self.slots, [1] * self.rows)
        h = eng.forward(h, slot, pos)
        eng.advance(self.slots, [1] * self.rows)
        pen = {"slots": self.slots, "tokens_in": self.tokens.tolist()} if self.stages else {}
        tok = self.sampler.sample(h, None, self.params, [p + 1 for p in pos], return_logprobs=self.lp is not None,
                                  **pen)
        if self.lp is not None:
            tok, self.lp = tok
        self.tokens.copy_(tok.to(torch.int32))
        if self.history is not None and self.step < self.history.shape[0]:
            self.history[self.step] = self.tokens
            if self.lp_history is not None:
                self.lp_history[self.step] = self.lp.tok_lp
        self.step += 1
        self._out = h

    replay = _body


SCORE_CHUNK_BYTES = 64 << 20  # score_prompt: no more logits than this exist at once


def score_prompt(eng: StageEngine, ids, top: int = 0, slot: int = 0):
    """Teacher-forced log-probabilities of a prompt: prefills ``ids`` into KV slot ``slot`` (from
    position 0) and returns :class:`ops.logprobs.Logprobs` of host tensors with ``len(ids) - 1``
    rows - ``tok_lp[t] = log p(ids[t + 1] | ids[..t])`` (fp32), ``tok_rank``, and the ``top``
    (0..20) most likely tokens per position in ``top_id`` / ``top_lp``. The logits are produced and
    reduced in chunks of at most 64 MiB; GPU and CPU engines, bf16 and fp8 heads; needs the whole
    model's head on this engine (NotImplementedError on a split head)."""
    sampler = Sampler(eng)
    if not eng.has_embed:
        raise RuntimeError("[ERROR] score_prompt needs the stage that owns the embedding")
    ids = [int(t) for t in ids]
    top = int(top)
    if len(ids) < 2:
        raise ValueError("score_prompt needs at least two tokens")
    if not 0 <= top <= LP.TOP_MAX:
        raise ValueError(f"top must be in [0, {LP.TOP_MAX}], got {top}")
    if len(ids) > eng.max_seq:
        raise ValueError(f"prompt ({len(ids)}) exceeds max_seq {eng.max_seq}")
    n = len(ids) - 1
    chunk = max(1, min(SCORE_CHUNK_BYTES // (2 * eng.cfg.head_rows), eng.max_prefill_rows))
    parts = []
    eng.seq_len[slot] = 0
    for c0 in range(0, len(ids), eng.max_prefill_rows):  # the prefill, in chunks the engine's scratch holds
        c = min(eng.max_prefill_rows, len(ids) - c0)
        h = eng.forward(eng.embed(torch.tensor(ids[c0:c0 + c], dtype=torch.int64)), [slot] * c,
                        list(range(c0, c0 + c)))
        eng.seq_len[slot] = c0 + c
        for r0 in range(0, min(c, n - c0), chunk):
            k = min(chunk, min(c, n - c0) - r0)
            logits = sampler.logits(h, list(range(r0, r0 + k)))
            lp = sampler.logprobs(logits, ids[c0 + r0 + 1:c0 + r0 + k + 1], top)
            parts.append([t.cpu() for t in lp])
            del logits
    return LP.Logprobs(*(torch.cat([p[i] for p in parts]) for i in range(5)))


__all__ = ["SamplingParams", "GREEDY", "Sampler", "PenaltyState", "ConstraintState", "GrammarState", "CompiledConstraint",
           "compile_constraints", "SamplingDecodeGraph", "EagerSamplingDecode",
           "device_params", "score_prompt", "SCORE_CHUNK_BYTES"]
