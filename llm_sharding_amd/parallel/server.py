"""Continuous-batching serving over the layer-sharded pipeline (one process per GPU).

The reference serves one request at a time around a ZMQ ring, and in serve mode never even
reads requests (``/root/reference/utils/node_worker.py:493-559``). Here the
stages are the ranks of one ``torch.distributed`` job (RCCL over xGMI on GPUs, gloo on CPU)
and rank 0 - the stage that owns the embedding - is also the ingress and the scheduler:

* ``M`` micro-batches of ``B`` KV-cache slots; each micro-batch has at most ONE command in
  flight, so with ``M >= world`` every stage always has work (the same schedule as
  :mod:`.pipeline`).
* Per visit of a micro-batch, rank 0 first collects the token ids the last stage returned for
  its previous command (ring back-edge), updates the requests (streaming output, EOS /
  ``max_new_tokens``), frees finished slots, then issues the next command:
  ``PREFILL`` (admit waiting requests into free slots; long prompts are prefilled in chunks
  under a token budget, only the final chunk emits the first token) or ``DECODE`` (one step of
  every slot of the micro-batch: the captured hipGraph of :class:`DecodeGraph` on GPUs,
  positions on the device, eager active rows on CPU).
* Commands are small int32 headers sent by rank 0 to every rank over a separate gloo (CPU)
  group, so no stage ever blocks its GPU to learn what to do next; activations go rank r ->
  r+1 and token ids last -> 0 over the data group (RCCL).

A slot whose request finished is re-armed (device position reset) with the next command of
its micro-batch; a free slot still rides along in graph replays (its outputs are ignored),
which keeps the graph static.

Prefix pool (``prefix_slots=P``): the engine gets ``B * M + P`` KV slots; slots ``>= B * M`` are
never decoded and belong to no micro-batch or graph. A request that declares ``cache_prefix=L``
has ``input_ids[:L]`` prefilled into a pool slot (ordinary ``PREFILL`` items ``(pool_slot, p0, n,
0)`` in its own micro-batch's commands), and every admitted request forks the longest pooled match
of its prompt into its slot with ``FORK`` - items ``(src, dst, len, 0)``, executed by every rank on
its own layers (:func:`..ops.kvcache.fork_jobs`), nothing returned - and prefills only the rest.
:meth:`submit_n` queues ``n`` samples of one prompt behind one prefill the same way. Rank 0 keeps
the registry (tokens, ready flag, pin count, LRU stamp per pool slot); with ``streams > 1`` a fork
waits on the event of the command that finished filling its entry, and the refill of an evicted
entry on the events of the forks that read it.

Live re-sharding (the reference's hot re-configuration, ``/root/reference/utils/node_worker.py
:445-474``, on the deployed pipeline): :meth:`request_replan` (rank 0; the master's ``replan``
command arrives through the ingress) stops admitting requests, lets every request in flight
finish on the current layer split, then broadcasts ``REPLAN`` with the new stage boundaries in
the same ordered command stream; every rank drains its sends, frees its engine, loads its new
``[start, end)`` range, rebuilds KV cache and decode graphs, and rank 0 resumes admission. The
ring edges (and their communicators) are unchanged - only the layer ranges move.
"""
from __future__ import annotations

import contextlib
import queue
import threading
import time
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional

import torch

from ..runtime.engine import DecodeGraph, StageEngine
from ..runtime.logit_stages import STAGE_CLASSES, STAGE_ORDER, ordered_stages
from ..runtime.sampling import SamplingParams
from ..utils import tracing
from .pipeline import DistP2P, _percentile

CMD_DECODE, CMD_PREFILL, CMD_STOP, CMD_REPLAN, CMD_FORK = 1, 2, 3, 4, 5
WAITING, PREFILLING, DECODING, DONE = "waiting", "prefilling", "decoding", "done"
FORKING = "forking"  # admitted, waiting to fork its prefix from a pool entry

# Default of ``prefix_min_match``: the shortest undeclared match worth a fork. Measured on an MI355X
# (profiles/kv_fork.md part b, scripts/bench_prefix.py breakeven; Llama-2-7B): fork(j) + a suffix
# prefill against a whole prefill of j + suffix tokens, suffixes 32, 31 and 1. j = 1 loses 0.03 -
# 0.04 ms at two of the three suffixes (the fork costs 0.06 ms and a prefill command's time is a step
# function of its rows); j = 8 is the smallest measured j that wins at all three (by 0.09 - 0.46 ms).
PREFIX_MIN_MATCH = 8


@dataclass
class Request:
    rid: int
    input_ids: List[int]
    max_new_tokens: int
    eos_ids: tuple
    on_token: Optional[Callable] = None
    reply_to: Optional[str] = None
    sampling: Optional[SamplingParams] = None  # None: greedy
    # sampling.logprobs set: one entry per generated token (else they stay None)
    token_logprobs: Optional[List[float]] = None
    ranks: Optional[List[int]] = None
    top_logprobs: Optional[List[list]] = None  # logprobs >= 1: [[id, logprob], ...] per token
    state: str = WAITING
    slot: int = -1
    prefilled: int = 0
    output_ids: List[int] = field(default_factory=list)
    t_submit: float = 0.0
    t_first: float = 0.0
    t_done: float = 0.0
    cache_prefix: Optional[int] = None  # declared: input_ids[:cache_prefix] is worth keeping in the pool
    group: Optional[dict] = None  # submit_n: the state its children share
    entry: Optional["_PoolEntry"] = None  # FORKING: the pool entry it forks from ...
    fork_len: int = 0  # ... and how many tokens
    constraint: Optional[object] = None  # sampling.constrained: its CompiledConstraint (automaton acquired)
    grammar: Optional[object] = None  # sampling.regex: its ByteDFA (rows of the DFA arena acquired)

    @property
    def ttft_ms(self) -> float:
        return (self.t_first - self.t_submit) * 1e3

    @property
    def tpot_ms(self) -> float:
        n = len(self.output_ids)
        return (self.t_done - self.t_first) * 1e3 / (n - 1) if n > 1 else 0.0


@dataclass(eq=False)
class _PoolEntry:
    """One slot of the prefix pool (rank 0's registry)."""
    slot: int
    tokens: List[int]
    filler: Optional[Request] = None  # the request whose micro-batch carries the fill
    filled: int = 0  # tokens of the fill issued so far
    ready: bool = False  # the whole fill is issued: later commands may fork from it
    pins: int = 0  # admitted requests (and unadmitted submit_n children) that have yet to fork from it
    stamp: int = 0  # least recently used = smallest
    fill_event: object = None  # streams > 1: recorded behind the last fill command

    @property
    def length(self) -> int:
        return len(self.tokens)


class _Header:
    """int32 command header: [cmd, mb, n_items, n_resets, items (slot, p0, n, emit)..., resets...];
    FORK: items are (src, dst, len, 0); REPLAN: [cmd, 0, world + 1, 0, stage boundaries...]."""

    def __init__(self, batch: int, world: int = 1):
        self.size = 4 + max(4 * batch + batch, world + 1)

    def pack(self, cmd, mb, items=(), resets=()) -> torch.Tensor:
        t = torch.zeros(self.size, dtype=torch.int32)
        t[0], t[1], t[2], t[3] = cmd, mb, len(items), len(resets)
        o = 4
        for it in items:
            t[o:o + 4] = torch.tensor(it, dtype=torch.int32)
            o += 4
        for s in resets:
            t[o] = s
            o += 1
        return t

    @staticmethod
    def unpack(t: torch.Tensor):
        v = t.tolist()
        cmd, mb, ni, nr = v[:4]
        items = [tuple(v[4 + 4 * i: 8 + 4 * i]) for i in range(ni)]
        resets = v[4 + 4 * ni: 4 + 4 * ni + nr]
        return cmd, mb, items, resets


class PipelineServer:
    """One rank of a continuous-batching pipeline server. Rank 0 additionally owns the
    request queue (:meth:`submit`, :meth:`serve`); the other ranks run :meth:`serve` too and
    follow rank 0's commands until ``STOP``."""

    def __init__(self, cfg, source, rank: int = 0, world: int = 1, start: int = 0, end: Optional[int] = None,
                 device="cpu", batch: int = 8, microbatches: int = 1, max_seq: int = 2048,
                 prefill_budget: int = 2048, use_graph: bool = True, dtype=torch.bfloat16,
                 ctrl_group=None, p2p=None, causal: bool = True, verbose: bool = False, streams: int = 1,
                 prefix_slots: int = 0, prefix_min_match: int = PREFIX_MIN_MATCH, state_rows: int = 256,
                 vocab_bytes=None, dfa_rows: int = 4096, kv_dtype: str = "bf16", json_max_ws: int = 2,
                 kv_layout: str = "static", kv_pages: Optional[int] = None):
        """``kv_layout="paged"``: the KV cache of a GPU stage is a pool of ``kv_pages`` 64-token pages
        (runtime/engine_paged.py; default: what every slot at ``max_seq`` would fill). Every rank
        drives its own ``PagePool`` from the command stream (:meth:`_exec_body`); rank 0 admits a
        request only while the pages of all admitted requests, each ``pages_for(prompt +
        max_new_tokens)``, fit the pool. On a CPU stage the cache stays static and the same
        accounting runs."""
        self.cfg, self.rank, self.world = cfg, rank, world
        if isinstance(json_max_ws, bool) or not isinstance(json_max_ws, int) or not 0 <= json_max_ws <= 8:
            raise ValueError(f"json_max_ws must be an integer in [0, 8], got {json_max_ws!r}")
        self.json_max_ws = json_max_ws
        from ..runtime.engine_kv8 import check_kv_dtype
        check_kv_dtype(kv_dtype)
        if kv_dtype == "fp8" and int(prefix_slots) > 0:
            raise ValueError("prefix_slots > 0 needs kv_dtype='bf16': the KV fork kernel copies bf16 tensors")
        self.kv_dtype = kv_dtype
        from ..ops import kv_paged
        from ..runtime.engine_paged import check_kv_layout
        check_kv_layout(kv_layout, kv_pages, "bf16", kv_dtype)
        self.kv_paged = kv_layout == "paged"
        if self.kv_paged:
            kv_paged.check_max_seq(int(min(max_seq, cfg.max_position_embeddings)))
            if int(prefix_slots) > 0:
                raise ValueError("prefix_slots > 0 needs kv_layout='static': the KV fork kernel copies static tensors")
            if kv_pages is None:
                kv_pages = batch * microbatches * (int(min(max_seq, cfg.max_position_embeddings)) // kv_paged.PAGE) + 1
        self.kv_pages = None if kv_pages is None else int(kv_pages)
        self.kv_pool = None            # this rank's page allocator (the paged engine's own on a GPU)
        self.kv_len: Dict[int, int] = {}   # this rank's count of every live slot's length
        self.kv_held: Dict[int, int] = {}  # rank 0: pages reserved by the request in each slot, admission to finish
        self.peak_in_flight = 0
        # prefix pool: engine slots >= B * M, never decoded, in no micro-batch and no graph
        self.P = int(prefix_slots)
        if self.P < 0 or int(prefix_min_match) < 1:
            raise ValueError("prefix_slots must be >= 0 and prefix_min_match >= 1")
        if self.P > 0 and not causal:
            raise ValueError("prefix caching needs causal attention: under the unmasked prefill a prefix's K/V "
                             "depend on the tokens after it")
        self.prefix_min_match = int(prefix_min_match)
        self.pool: List[Optional[_PoolEntry]] = [None] * self.P
        self._pool_reads: List[list] = [[] for _ in range(self.P)]  # fork events that outlive an evicted entry
        self._stamp = 0
        self.prefix_stats = {"prefix_hits": 0, "prefix_tokens_forked": 0, "prefix_fills": 0, "prefix_evictions": 0,
                             "prefix_bypass": 0}
        end = cfg.num_hidden_layers if end is None else end
        self.first, self.last = rank == 0, rank == world - 1
        self.B, self.M = batch, microbatches
        self.device = torch.device(device)
        self.gpu = self.device.type == "cuda"
        self.graph_mode = use_graph and self.gpu
        self.dtype = torch.bfloat16 if self.gpu else dtype
        self.budget = int(prefill_budget)
        self.verbose = verbose
        self.source, self.causal, self.max_seq = source, causal, max_seq
        self.start, self.end = start, end
        self.eng = self._build_engine(start, end)
        self.p2p = p2p if p2p is not None else DistP2P()
        self.ctrl = ctrl_group
        self.hdr = _Header(batch, world)
        self.graphs: List = []
        # Concurrent micro-batches (one GPU, graph mode): every command of micro-batch mb -
        # prefill, decode replay, result collection - runs on stream mb % S against engine
        # scratch set mb % S (sized for the prefill budget), so up to S micro-batches share the
        # GPU at once (see pipeline.PipelineStage); a micro-batch's own commands stay ordered.
        self.S = max(1, min(streams, microbatches)) if (self.graph_mode and world == 1) else 1
        self.streams = [torch.cuda.Stream(self.device) for _ in range(self.S)] if self.S > 1 else []
        # sampling (world == 1): off until the first non-greedy request is admitted - an all-greedy
        # server never builds a Sampler, a sampling graph or a logits buffer
        self.sampling_on = False
        self.sampler = None
        # logit stages (runtime.logit_stages): each one's tables exist, and the graphs carry its
        # launch, from the first request that asks for it on - the penalties' token statistics, the
        # constraints' automaton arena (state_rows rows), the DFA arena of a regex (dfa_rows rows of
        # 512 B; vocab_bytes, an ops.grammar.VocabBytes, is what such requests need; the same stage
        # serves json_object requests with the automaton BytePDA.json(max_ws=json_max_ws)). The host
        # allocators of the two arenas exist from the first such submit on.
        self.penalties = self.constraints = self.grammar = None
        self._json = None  # (BytePDA or None, the vocabulary check's error or None), from the first use on
        self.state_rows, self.vocab_bytes, self.dfa_rows = int(state_rows), vocab_bytes, int(dfa_rows)
        self._arena = self._garena = self._gcheck = None
        # logprobs: the graphs carry the lsa_logprobs launch from the first request that asks on
        self.logprobs_on = False
        self._lp_out: List = [None] * microbatches  # logprobs of a micro-batch's outstanding command
        self._build_graphs()
        # rank 0 state
        self.incoming: "queue.Queue[Request]" = queue.Queue()
        self.waiting: List[Request] = []
        self.by_slot: Dict[int, Request] = {}
        self.requests: Dict[int, Request] = {}
        self.finished: List[Request] = []
        self.outstanding: List = [None] * microbatches
        self.pending_resets: List[list] = [[] for _ in range(microbatches)]
        self.cur_tok: Dict[int, int] = {}  # eager mode: next input token per slot
        self._next_id = 0
        self._ctrl_works: list = []
        self._send_works: list = []
        self._lock = threading.Lock()
        self._replan: Optional[list] = None  # rank 0: stage boundaries waiting for a drained pipeline
        self.replans = 0
        self.tokens_generated = 0
        self.t_start = None
        self.tl = tracing.from_env(rank, self.device)  # LSA_TRACE=dir -> per-rank Chrome trace

    # ------------------------------------------------------------------ engine (re)build
    def _build_engine(self, start: int, end: int) -> StageEngine:
        from ..runtime.engine_int4 import make_stage_engine
        eng = make_stage_engine(self.cfg, start, end, self.device, self.dtype, has_embed=self.first,
                                 has_head=self.last, source=self.source, max_slots=self.B * self.M + self.P,
                                 max_seq=self.max_seq, max_prefill_rows=max(self.budget, self.B), causal=self.causal,
                                 kv_dtype=self.kv_dtype, kv_layout="paged" if self.kv_paged else "static",
                                 kv_pages=self.kv_pages)
        if self.kv_paged:  # a fresh engine: every page is free again
            from ..ops import kv_paged
            self.kv_pool = eng.pool if getattr(eng, "paged", False) else kv_paged.PagePool(self.kv_pages, eng.max_slots,
                                                                                          eng.max_seq)
            self.kv_len = {}
            self.kv_held = {}
        return eng

    # ------------------------------------------------------------------ pages (every rank)
    def _kv_reserve(self, slot: int, n_tokens: int) -> None:
        if getattr(self.eng, "paged", False):
            self.eng.kv_reserve(slot, n_tokens)  # (pushes the changed table entries)
        else:
            self.kv_pool.reserve(slot, n_tokens)

    def _kv_release(self, slot: int) -> None:
        self.kv_len.pop(slot, None)
        if getattr(self.eng, "paged", False):
            self.eng.kv_release(slot)
        else:
            self.kv_pool.release(slot)

    def _apply_resets(self, resets) -> None:
        for s in resets:
            self._set_pos(s, 0)
            if self.kv_paged and s < self.B * self.M:
                self._kv_release(s)

    def _kv_account(self, cmd, mb, items) -> None:
        """The pages this command writes, reserved before it runs (its resets have released theirs:
        a finished request's slot is reset by the first command after it, whoever takes the slot).
        PREFILL item (slot, p0, n, emit): ``p0 + n`` tokens. DECODE: one more token for every live
        slot of the micro-batch."""
        if cmd == CMD_PREFILL:
            for (s, p0, n, _) in items:
                self.kv_len[s] = p0 + n
                self._kv_reserve(s, p0 + n)
        elif cmd == CMD_DECODE:
            for s in self._slots(mb):
                if s in self.kv_len:
                    self.kv_len[s] = min(self.kv_len[s] + 1, self.eng.max_seq)
                    self._kv_reserve(s, self.kv_len[s])

    def _build_graphs(self) -> None:
        for k in range(1, self.S):
            self.eng.decode_scratch(k, rows=self.eng.max_prefill_rows)
        self.graphs = []
        if self.graph_mode:
            mode = "full" if self.world == 1 else ("first" if self.first else ("last" if self.last else "mid"))
            for mb in range(self.M):
                if self.sampling_on:
                    from ..runtime.sampling import SamplingDecodeGraph
                    g = SamplingDecodeGraph(self.eng, self.B, mode, slots=self._slots(mb), scratch=mb % self.S,
                                            logprobs=self.logprobs_on, **self._stage_kw())
                else:
                    g = DecodeGraph(self.eng, self.B, mode, slots=self._slots(mb), scratch=mb % self.S)
                self.graphs.append(g.capture())
        for st in self.streams:  # after weight loading and graph capture on the current stream
            st.wait_stream(torch.cuda.current_stream(self.device))

    def _enable_sampling(self, penalties: bool = False, logprobs: bool = False, constraints: bool = False,
                         grammar: bool = False) -> None:
        """First non-greedy request (world == 1): build the Sampler and, in graph mode, replace
        every micro-batch's greedy graph by a SamplingDecodeGraph that takes over its device
        positions and tokens. Rows start greedy; a slot's parameters are written on admission.
        From here on greedy requests of this server take the arg-max of the bf16 logits in the
        decode graph (the first token still comes from the fused argmax)."""
        from ..runtime.sampling import Sampler
        first = {"penalties": penalties, "constraints": constraints, "grammar": grammar}
        for name in STAGE_ORDER:  # the first non-greedy request asks for stages too: one rebuild for all
            if first[name]:
                setattr(self, name, self._new_stage(name))
        self.logprobs_on = self.logprobs_on or logprobs
        self.sampler = Sampler(self.eng, **self._stage_kw())
        self.sampling_on = True
        self._swap_sampling_graphs()

    def _stage_kw(self) -> dict:
        """The logit stages (or None) by the keyword a Sampler or a graph takes them by."""
        return {name: getattr(self, name) for name in STAGE_ORDER}

    def _allocator(self, attr: str, rows: int):
        """The host allocator of an arena's rows, kept in ``attr`` and created on first use."""
        from ..ops.constraints import ArenaAllocator
        with self._lock:
            if getattr(self, attr) is None:
                setattr(self, attr, ArenaAllocator(rows))
            return getattr(self, attr)

    def _new_stage(self, name: str):
        from ..runtime import logit_stages as LS
        n = self.B * self.M
        return {
            "penalties": lambda: LS.PenaltyState(self.eng, n),
            "constraints": lambda: LS.ConstraintState(self.eng, n, self.state_rows,
                                                      allocator=self._allocator("_arena", self.state_rows)),
            "grammar": lambda: LS.GrammarState(self.eng, n, self.vocab_bytes, self.dfa_rows,
                                               allocator=self._allocator("_garena", self.dfa_rows),
                                               pda=self._json_pda()[0]),
        }[name]()

    def _json_pda(self) -> tuple:
        """``(pda, None)``: the JSON automaton of this server, checked against its vocabulary; or
        ``(None, error)`` when the vocabulary cannot spell JSON (or the configuration has no EOS id)
        - then json_object requests are refused at submit and the stage serves regexes alone."""
        from ..ops.pda import BytePDA, check_vocab
        with self._lock:
            if self._json is None:
                pda = BytePDA.json(max_ws=self.json_max_ws)
                try:
                    if not list(self.cfg.eos_ids):
                        raise ValueError("json_object needs an EOS id in the configuration: the output ends with it")
                    check_vocab(pda, self.vocab_bytes, self.cfg.eos_ids)
                    self._json = (pda, None)
                except ValueError as e:
                    self._json = (None, str(e))
            return self._json

    def _enable_stage(self, name: str) -> None:
        """First request that asks for the logit stage ``name`` (sampling already on): allocate its
        state and, in graph mode, replace every sampling graph by one whose step holds its launch,
        carrying positions, tokens and the rows' parameters over. Until then no graph holds that
        kernel and no table is allocated."""
        setattr(self, name, self._new_stage(name))
        setattr(self.sampler, name, getattr(self, name))
        self._swap_sampling_graphs()

    def _enable_logprobs(self) -> None:
        """First request with ``logprobs`` (sampling already on): in graph mode, replace every
        sampling graph by one whose step ends in ``lsa_logprobs``, carrying positions, tokens and
        the rows' parameters over. A server that never sees such a request runs the graphs
        without that launch."""
        self.logprobs_on = True
        self._swap_sampling_graphs()

    def _swap_sampling_graphs(self) -> None:
        from ..runtime.sampling import SamplingDecodeGraph
        if not self.graph_mode:
            return
        torch.cuda.synchronize(self.device)
        old, self.graphs = self.graphs, []
        for mb in range(self.M):
            g = SamplingDecodeGraph(self.eng, self.B, "full", slots=self._slots(mb), scratch=mb % self.S,
                                    logprobs=self.logprobs_on, **self._stage_kw())
            g.pos.copy_(old[mb].pos)
            g.tokens.copy_(old[mb].tokens)
            for i, p in enumerate(getattr(old[mb], "params", ())):
                g.set_params(i, p)
            self.graphs.append(g.capture())
        del old
        for st in self.streams:
            st.wait_stream(torch.cuda.current_stream(self.device))
        torch.cuda.synchronize(self.device)

    def _sample_rows(self, h, rows_idx, slots, positions, tok: torch.Tensor, tokens_in=None,
                     mb: int = 0) -> torch.Tensor:
        """Replace the greedy tokens ``tok`` of the rows whose request samples: row
        ``rows_idx[i]`` of ``h`` belongs to ``slots[i]`` and its new token will sit at
        ``positions[i]``. ``tokens_in[i]``: the token the row was fed (a decode step), counted
        by the penalties; None after a prefill. With logprobs on, the log-probabilities of the
        rows that ask for them wait in ``_lp_out[mb]`` for the command's collection."""
        reqs = [self.by_slot.get(s) for s in slots]
        sel = [i for i, r in enumerate(reqs) if r is not None and r.sampling is not None]
        if sel:
            pen = {}
            if ordered_stages(**self._stage_kw()):
                pen = {"slots": [slots[i] for i in sel],
                       "tokens_in": None if tokens_in is None else [tokens_in[i] for i in sel]}
            want_lp = self.logprobs_on and any(reqs[i].sampling.logprobs is not None for i in sel)
            t = self.sampler.sample(h, [rows_idx[i] for i in sel], [reqs[i].sampling for i in sel],
                                    [positions[i] for i in sel], return_logprobs=want_lp, **pen)
            if want_lp:
                t, lp = t
                self._lp_out[mb] = ([slots[i] for i in sel], self._lp_to_host(lp))
            tok[torch.tensor(sel, dtype=torch.long, device=tok.device)] = t.to(tok.dtype)
        return tok

    def _lp_to_host(self, lp):
        """(tok_lp, tok_rank, top_id, top_lp) on their way to the host, like :meth:`_to_host`."""
        return [self._to_host(t) for t in (lp.tok_lp, lp.tok_rank, lp.top_id, lp.top_lp)]

    def _take_logprobs(self, mb: int) -> dict:
        """The logprobs the micro-batch's collected command left: slot -> (lp, rank, ids, lps)."""
        o, self._lp_out[mb] = self._lp_out[mb], None
        if o is None:
            return {}
        slots, parts = o
        lp, rank, ids, lps = (self._host_list(p) for p in parts)
        return {s: (lp[i], rank[i], ids[i], lps[i]) for i, s in enumerate(slots)}

    @staticmethod
    def _record_logprobs(r: Request, entry) -> None:
        """Append one generated token's logprobs to a request that asked for them."""
        if r.sampling is None or r.sampling.logprobs is None or entry is None:
            return
        lp, rank, ids, lps = entry
        if r.token_logprobs is None:
            r.token_logprobs, r.ranks = [], []
            r.top_logprobs = [] if r.sampling.logprobs > 0 else None
        r.token_logprobs.append(float(lp))
        r.ranks.append(int(rank))
        if r.top_logprobs is not None:
            n = r.sampling.logprobs
            r.top_logprobs.append([[int(i), float(v)] for i, v in zip(ids[:n], lps[:n]) if i >= 0])

    def _reshard(self, start: int, end: int) -> None:
        """Every rank, pipeline drained: free this stage's engine, load layers [start, end),
        rebuild the KV cache and the decode graphs (same slots, micro-batches and streams)."""
        self._flush_sends()
        if self.gpu:
            torch.cuda.synchronize(self.device)
        with self.tl.span("replan", start=start, end=end):
            self.graphs = []
            self.eng = None
            if self.gpu:
                torch.cuda.empty_cache()
            self.eng = self._build_engine(start, end)
            self.start, self.end = start, end
            if self.sampling_on:
                from ..runtime.sampling import Sampler
                self.sampler = None
                for name in STAGE_ORDER:  # drained: no slot holds statistics or an automaton; waiting
                    if getattr(self, name) is not None:  # requests keep their references in the allocators
                        setattr(self, name, None)
                        if self.gpu:
                            torch.cuda.empty_cache()
                        setattr(self, name, self._new_stage(name))
                self.sampler = Sampler(self.eng, **self._stage_kw())
            self._build_graphs()
            if self.gpu:
                torch.cuda.synchronize(self.device)
        # the pool's K/V went with the engine: same prefix_slots, empty registry
        self.pool = [None] * self.P
        self._pool_reads = [[] for _ in range(self.P)]
        self.cur_tok.clear()
        self.pending_resets = [[] for _ in range(self.M)]
        self.replans += 1
        if self.verbose:
            print(f"[INFO] rank {self.rank}: re-sharded to layers [{start}, {end})", flush=True)

    def request_replan(self, stages) -> None:
        """Rank 0 (thread-safe): move the layer split to ``stages`` ([[start, end], ...] per rank,
        contiguous from 0 to num_hidden_layers). New requests wait; requests in flight finish
        on the current split first (:meth:`serve` applies it once the pipeline is drained)."""
        if not self.first:
            raise RuntimeError("re-plans are requested on rank 0 (the pipeline's command stream)")
        st = [(int(a), int(b)) for a, b in stages]
        L = self.cfg.num_hidden_layers
        ok = (len(st) == self.world and st[0][0] == 0 and st[-1][1] == L
              and all(a < b for a, b in st) and all(x[1] == y[0] for x, y in zip(st, st[1:])))
        if not ok:
            raise ValueError(f"replan: {st} is not a contiguous split of {L} layers over {self.world} stages")
        with self._lock:
            self._replan = [a for a, _ in st] + [L]

    def _apply_replan(self) -> None:
        with self._lock:
            bounds, self._replan = self._replan, None
        t = torch.zeros(self.hdr.size, dtype=torch.int32)
        t[0], t[2] = CMD_REPLAN, len(bounds)
        t[4:4 + len(bounds)] = torch.tensor(bounds, dtype=torch.int32)
        self._bcast_header(t)
        self._reshard(bounds[0], bounds[1])

    # ------------------------------------------------------------------ helpers
    def _mb_ctx(self, mb: int):
        """Stream + engine scratch set of micro-batch ``mb`` (no-op with one stream)."""
        if self.S == 1:
            return contextlib.nullcontext()
        es = contextlib.ExitStack()
        es.enter_context(torch.cuda.stream(self.streams[mb % self.S]))
        es.enter_context(self.eng.use_scratch(mb % self.S))
        return es

    def _slots(self, mb: int) -> list:
        return list(range(mb * self.B, (mb + 1) * self.B))

    def _set_pos(self, slot: int, p: int) -> None:
        self.eng.seq_len[slot] = p
        if self.graph_mode and slot < self.B * self.M:  # a pool slot has no device position
            mb, i = divmod(slot, self.B)
            self.graphs[mb].pos[i] = p

    def _to_host(self, t: torch.Tensor):
        """Token ids -> host without serialising the host behind later GPU work: a pinned
        non-blocking copy enqueued right behind the producing kernels, plus an event."""
        if not self.gpu:
            return t.tolist()
        h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
        h.copy_(t, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        return (h, ev)

    @staticmethod
    def _host_list(local):
        if isinstance(local, tuple):
            h, ev = local
            ev.synchronize()
            return h.tolist()
        return local

    def _send(self, t, dst):
        self._send_works.append((self.p2p.isend(t, dst), t))
        if len(self._send_works) > 4 * self.M:
            w, _ = self._send_works.pop(0)
            w.wait()

    def _flush_sends(self):
        for w, _ in self._send_works:
            w.wait()
        self._send_works.clear()

    def _bcast_header(self, hdr: torch.Tensor) -> None:
        if self.world == 1:
            return
        import torch.distributed as dist
        for r in range(1, self.world):
            self._ctrl_works.append((dist.isend(hdr, r, group=self.ctrl), hdr))
        while len(self._ctrl_works) > 8 * self.world:
            w, _ = self._ctrl_works.pop(0)
            w.wait()

    # ------------------------------------------------------------------ command execution (every rank)
    def _exec(self, cmd, mb, items, resets, ids=None):
        """Run one command on this stage. Returns the last stage's token ids (world == 1)."""
        name = {CMD_PREFILL: "prefill", CMD_DECODE: "decode", CMD_FORK: "fork"}.get(cmd, "cmd")
        with self.tl.span(name, mb=mb, items=len(items)), self._mb_ctx(mb):
            return self._exec_body(cmd, mb, items, resets, ids)

    def _exec_body(self, cmd, mb, items, resets, ids=None):
        eng, H = self.eng, self.cfg.hidden_size
        self._apply_resets(resets)
        if self.kv_paged:
            self._kv_account(cmd, mb, items)
        if cmd == CMD_FORK:  # items (src, dst, len, 0) on this stage's layers; nothing returns
            from ..ops.kvcache import MAX_FANOUT, fork_jobs
            by_src: Dict[tuple, list] = {}
            for (src, dst, n, _) in items:
                by_src.setdefault((src, n), []).append(dst)
            fork_jobs(eng, [(src, n, d[i:i + MAX_FANOUT]) for (src, n), d in by_src.items()
                            for i in range(0, len(d), MAX_FANOUT)])
            for (_, dst, n, _) in items:
                self._set_pos(dst, n)
            return None
        if cmd == CMD_PREFILL:
            slot, pos, emit_rows = [], [], []
            for (s, p0, n, emit) in items:
                eng.seq_len[s] = p0
                slot += [s] * n
                pos += list(range(p0, p0 + n))
                if emit:
                    emit_rows.append(len(pos) - 1)
            rows = len(slot)
            if self.first:
                h = eng.embed(torch.tensor(ids, dtype=torch.int64))
            else:
                h = torch.empty((rows, H), dtype=self.dtype, device=self.device)
                self.p2p.recv(h, self.rank - 1)
            h = eng.forward(h, slot, pos)
            for (s, p0, n, emit) in items:
                self._set_pos(s, p0 + n)
            if self.last:
                if not emit_rows:
                    return []
                tok = eng.head(h, emit_rows).to(torch.int32)
                if self.sampling_on:
                    em = [it for it in items if it[3]]
                    for st in ordered_stages(**self._stage_kw()):  # the requests that ask for a stage enter their slots
                        for (s, _, _, _) in em:
                            r = self.by_slot.get(s)
                            if r is not None and r.sampling is not None and st.wants(r.sampling):
                                held = {"constraints": r.constraint, "grammar": r.grammar}.get(st.name)
                                st.enter(s, r.sampling, r.input_ids, reserved=held)  # held: reserved by submit
                    tok = self._sample_rows(h, emit_rows, [it[0] for it in em], [it[1] + it[2] for it in em], tok,
                                            mb=mb)
                    if self.graph_mode:  # the slot's parameters, before its first decode step
                        for (s, _, _, _) in em:
                            r = self.by_slot.get(s)
                            self.graphs[mb].set_params(s - mb * self.B, None if r is None else r.sampling)
                if self.world == 1:
                    return self._to_host(tok)
                self._send(tok.contiguous(), 0)
            else:
                self._send(h.contiguous(), self.rank + 1)
            return None
        if cmd == CMD_DECODE:
            if self.graph_mode:
                g = self.graphs[mb]
                if not self.first:
                    self.p2p.recv(g.h_in, self.rank - 1)
                g.replay()
                if self.last:
                    if self.world == 1:
                        if self.logprobs_on and g.lp is not None:
                            self._lp_out[mb] = (self._slots(mb), self._lp_to_host(g.lp))
                        return self._to_host(g.tokens)
                    out = g.tokens.clone()
                    self._send(out, 0)
                else:
                    self._send(g.out_hidden.clone(), self.rank + 1)
                return None
            # eager: only the listed rows (slot, p0) run
            slots = [it[0] for it in items]
            n = len(slots)
            if self.first:
                h = eng.embed(torch.tensor(ids, dtype=torch.int64))
            else:
                h = torch.empty((n, H), dtype=self.dtype, device=self.device)
                self.p2p.recv(h, self.rank - 1)
            pos = [it[1] for it in items]
            for s, p in zip(slots, pos):
                eng.seq_len[s] = p
            h = eng.forward(h, slots, pos)
            for s, p in zip(slots, pos):
                eng.seq_len[s] = p + 1
            if self.last:
                tok = eng.head(h).to(torch.int32)
                if self.sampling_on:
                    tok = self._sample_rows(h, list(range(n)), slots, [p + 1 for p in pos], tok, tokens_in=ids,
                                            mb=mb)
                if self.world == 1:
                    return self._to_host(tok)
                self._send(tok.contiguous(), 0)
            else:
                self._send(h.contiguous(), self.rank + 1)
            return None
        return None

    # ------------------------------------------------------------------ rank 0: requests
    def submit(self, input_ids, max_new_tokens: int = 64, eos_ids=None, on_token=None,
               reply_to: Optional[str] = None, sampling: Optional[SamplingParams] = None, *,
               cache_prefix: Optional[int] = None, _group: Optional[dict] = None) -> int:
        """Queue a request (thread-safe). ``input_ids``: list of token ids. ``cache_prefix=L``
        (a server with ``prefix_slots``): ``input_ids[:L]`` is worth keeping - it is prefilled into
        a pool slot once and forked from there by this and later requests (``L`` is clamped to
        ``len - 1``: the last prompt token is always computed). ``sampling``:
        temperature / top-k / top-p / seed, repetition / presence / frequency penalties and
        ``logprobs`` of the request, and its constraint fields (``logit_bias``, ``banned_token_ids``,
        ``min_tokens``, ``min_p``, ``allowed_token_ids``, ``choices``, ``automaton``: checked here
        against the vocabulary, and the automaton's rows of the arena are reserved here - ValueError
        when they do not fit), and ``regex`` (compiled when the parameters were built; here its
        DFA is checked against the server's ``vocab_bytes`` and its rows of the DFA arena are
        reserved - ValueError without ``vocab_bytes``, when the DFA does not fit, or when one of its
        states allows no token of the vocabulary), and ``json_object`` (ValueError when the
        configuration has no EOS id, without ``vocab_bytes``, or when the vocabulary cannot spell JSON)
        (None, or temperature 0 with every penalty off, no logprobs and no constraint: greedy); its output depends only on its own prompt, seed and penalties, not on the slot or
        batch it runs in. With ``logprobs`` the finished :class:`Request` holds ``token_logprobs``,
        ``ranks`` and (``logprobs >= 1``) ``top_logprobs``, one entry per generated token."""
        if not self.first:
            raise RuntimeError("requests are submitted on rank 0 (the ingress stage)")
        if sampling is not None and sampling.plain:
            sampling = None
        if sampling is not None and self.world > 1:
            raise ValueError("sampling (temperature > 0, a penalty or logprobs) needs a single-stage server: with more "
                             "than one pipeline stage only greedy requests are served")
        ids = [int(x) for x in input_ids]
        if not ids:
            raise ValueError("empty prompt")
        if len(ids) + max_new_tokens > self.eng.max_seq:
            raise ValueError(f"prompt ({len(ids)}) + max_new_tokens ({max_new_tokens}) exceeds max_seq "
                             f"{self.eng.max_seq}")
        if self.kv_paged and self.kv_pool.pages_for(len(ids) + max_new_tokens) > self.kv_pages - 1:
            raise ValueError(f"prompt ({len(ids)}) + max_new_tokens ({max_new_tokens}) needs "
                             f"{self.kv_pool.pages_for(len(ids) + max_new_tokens)} pages, the pool has {self.kv_pages - 1}")
        constraint = None
        if sampling is not None and sampling.constrained:
            from ..runtime.sampling import _check_full_head, compile_constraints
            _check_full_head(self.eng)
            constraint = compile_constraints(sampling, self.cfg.vocab_size, self.cfg.eos_ids)
            if constraint.automaton is not None:  # its rows of the arena, now: no room is an error now
                arena = self._allocator("_arena", self.state_rows)
                with self._lock:
                    arena.acquire(constraint.automaton)
        grammar = None if sampling is None else sampling.grammar
        if grammar is not None or (sampling is not None and sampling.json_object):
            try:
                if grammar is not None:
                    self._reserve_grammar(grammar)
                else:
                    self._check_json()
            except ValueError:
                if constraint is not None and constraint.automaton is not None:
                    self._arena.release(constraint.automaton.digest)
                raise
        with self._lock:
            rid = self._next_id
            self._next_id += 1
        eos = tuple(self.cfg.eos_ids if eos_ids is None else eos_ids)
        if cache_prefix is not None:
            cache_prefix = max(0, min(int(cache_prefix), len(ids) - 1))
        r = Request(rid, ids, int(max_new_tokens), eos, on_token=on_token, reply_to=reply_to, sampling=sampling,
                    t_submit=time.perf_counter(), cache_prefix=cache_prefix, group=_group, constraint=constraint,
                    grammar=grammar)
        self.incoming.put(r)
        return rid

    def _check_json(self) -> None:
        """A json_object request is submitted: ValueError unless this server can serve it."""
        from ..runtime.sampling import _check_full_head
        if self.vocab_bytes is None:
            raise ValueError("json_object needs the byte strings of the vocabulary: build the server with "
                             "vocab_bytes=ops.grammar.VocabBytes.from_tokenizer(...)")
        if self.vocab_bytes.V != self.cfg.vocab_size:
            raise ValueError(f"vocab_bytes covers {self.vocab_bytes.V} tokens, the configuration has "
                             f"{self.cfg.vocab_size}")
        _check_full_head(self.eng)
        err = self._json_pda()[1]
        if err is not None:
            raise ValueError(err)

    def _reserve_grammar(self, dfa) -> None:
        """A request with a regex is submitted: check its DFA against the vocabulary's bytes and
        reserve its rows of the DFA arena (ValueError on either)."""
        from ..runtime.sampling import _check_full_head, check_vocab_cache
        if self.vocab_bytes is None:
            raise ValueError("a regex needs the byte strings of the vocabulary: build the server with "
                             "vocab_bytes=ops.grammar.VocabBytes.from_tokenizer(...)")
        if self.vocab_bytes.V != self.cfg.vocab_size:
            raise ValueError(f"vocab_bytes covers {self.vocab_bytes.V} tokens, the configuration has "
                             f"{self.cfg.vocab_size}")
        _check_full_head(self.eng)
        garena = self._allocator("_garena", self.dfa_rows)
        with self._lock:
            if self._gcheck is None:
                self._gcheck = check_vocab_cache(self.vocab_bytes, self.cfg.eos_ids)
            self._gcheck(dfa)
            garena.acquire(dfa)

    def submit_n(self, input_ids, n: int, max_new_tokens: int = 64, eos_ids=None, on_token=None,
                 reply_to: Optional[str] = None, sampling: Optional[SamplingParams] = None) -> List[int]:
        """Queue ``n`` samples of one prompt that share one prefill (thread-safe): ``input_ids[:-1]``
        becomes a pool entry, pinned until the last child has forked from it, and child ``i`` is an
        ordinary request with ``seed + i`` (``seed=None``: one drawn seed plus ``i``) and
        ``cache_prefix = len - 1``. Children admitted in the same scheduling round share one
        fan-out fork. Returns the children's request ids, in seed order."""
        import dataclasses
        n = int(n)
        if n < 1:
            raise ValueError(f"submit_n: n must be >= 1, got {n}")
        if self.P < 1:
            raise ValueError("submit_n needs a prefix pool: build the server with prefix_slots >= 1")
        ids = [int(x) for x in input_ids]
        rids: List[int] = []
        group = {"n": n, "left": n, "entry": None, "rids": rids}
        for i in range(n):
            sp = None if sampling is None else dataclasses.replace(sampling, seed=(sampling.seed + i) % (1 << 64))
            rids.append(self.submit(ids, max_new_tokens, eos_ids, on_token, reply_to, sp,
                                    cache_prefix=len(ids) - 1, _group=group))
        return rids

    def unfinished(self) -> List[Request]:
        """Rank 0, after :meth:`serve` has returned: every request that will never finish here
        (queued, waiting or in flight) - the controller answers them with an error when the
        pipeline is dropped (a lost rank), instead of leaving their clients waiting."""
        self._intake()
        return [r for r in self.requests.values() if r.state != DONE]

    def _intake(self) -> None:
        while True:
            try:
                r = self.incoming.get_nowait()
            except queue.Empty:
                break
            self.requests[r.rid] = r
            self.waiting.append(r)

    def _free_slots(self, mb: int) -> list:
        return [s for s in self._slots(mb) if s not in self.by_slot]

    # ------------------------------------------------------------------ rank 0: prefix pool
    @staticmethod
    def _common(a: list, b: list, cap: int) -> int:
        """Length of the common token prefix of ``a`` and ``b``, at most ``cap``."""
        n, i = min(len(a), len(b), cap), 0
        while i < n and a[i] == b[i]:
            i += 1
        return i

    def _pool_take(self, tokens: list, filler: Request) -> Optional[_PoolEntry]:
        """A pool slot for a new entry: a free one, else the least recently used unpinned one
        (evicted). None when every slot is pinned."""
        i = next((i for i, e in enumerate(self.pool) if e is None), None)
        if i is None:
            cand = [e for e in self.pool if e.pins == 0 and e.ready]
            if not cand:
                return None
            i = min(cand, key=lambda e: e.stamp).slot - self.B * self.M
            self.prefix_stats["prefix_evictions"] += 1
        e = self.pool[i] = _PoolEntry(self.B * self.M + i, list(tokens), filler=filler)
        self.prefix_stats["prefix_fills"] += 1
        return e

    def _attach(self, r: Request) -> None:
        """Admission of ``r``: choose the pool entry it forks from (a ready one, one that is being
        filled with its declared prefix, or a new one whose fill rides with ``r``'s micro-batch)
        and pin it; without one ``r`` stays an ordinary request."""
        ids, cap, g = r.input_ids, len(r.input_ids) - 1, r.group
        if g is not None:
            g["left"] -= 1  # children still to be admitted
        e, j, pinned = None, 0, False
        if g is not None and g["entry"] is not None and not any(c is g["entry"] for c in self.pool):
            g["entry"] = None  # a re-plan dropped the registry: the siblings' entry and its K/V are gone
        if g is not None and g["entry"] is not None:  # a sibling chose the entry and pinned it for r
            e, pinned = g["entry"], True
            j = self._common(e.tokens, ids, cap)
        else:
            L = r.cache_prefix or 0
            for c in self.pool:  # the longest match; a declared prefix may also wait for its fill
                if c is None:
                    continue
                cj = self._common(c.tokens, ids, cap)
                if cj > j and (cj >= L if L and not c.ready else c.ready):
                    e, j = c, cj
            if L and j < L:  # no entry covers the declared prefix: insert it
                e = self._pool_take(ids[:L], r)
                j = L
                if e is None:
                    self.prefix_stats["prefix_bypass"] += 1
                    e, j = None, 0
                    for c in self.pool:
                        cj = self._common(c.tokens, ids, cap) if c is not None and c.ready else 0
                        if cj > j:
                            e, j = c, cj
            if e is not None and not (L and j >= L) and j < self.prefix_min_match:
                e = None
        if e is None:
            return
        if not pinned:
            e.pins += 1
        if g is not None and g["entry"] is None:
            g["entry"] = e
            e.pins += g["left"]
        self._stamp += 1
        e.stamp = self._stamp
        if e.filler is not r:
            self.prefix_stats["prefix_hits"] += 1
            self.prefix_stats["prefix_tokens_forked"] += j
        r.entry, r.fork_len, r.state = e, j, FORKING

    def _issue_forks(self, mb: int) -> None:
        """Fork the prefix of every request of ``mb`` whose entry is ready: one ``CMD_FORK`` (items
        that share a source become one fan-out job), which returns nothing; the requests then
        prefill from their fork length."""
        rs = [r for r in (self.by_slot.get(s) for s in self._slots(mb))
              if r is not None and r.state == FORKING and r.entry.ready]
        if not rs:
            return
        items = [(r.entry.slot, r.slot, r.fork_len, 0) for r in rs]
        self._bcast_header(self.hdr.pack(CMD_FORK, mb, items, []))
        entries = list({id(r.entry): r.entry for r in rs}.values())
        if self.S > 1:  # the fill ran on its own micro-batch's stream
            with self._mb_ctx(mb):
                for e in entries:
                    if e.fill_event is not None:
                        torch.cuda.current_stream(self.device).wait_event(e.fill_event)
        self._exec(CMD_FORK, mb, items, [])
        if self.S > 1:  # a refill of an evicted entry waits for the forks that read its slot
            with self._mb_ctx(mb):
                ev = torch.cuda.Event()
                ev.record()
            for e in entries:
                i = e.slot - self.B * self.M
                self._pool_reads[i] = [x for x in self._pool_reads[i] if not x.query()] + [ev]
        for r in rs:
            r.entry.pins -= 1
            r.entry, r.prefilled, r.state = None, r.fork_len, PREFILLING

    def _emit(self, r: Request, tok: int, now: float) -> None:
        if not r.output_ids:
            r.t_first = now
        r.output_ids.append(tok)
        self.tokens_generated += 1
        if r.on_token is not None:
            r.on_token(r, tok)
        if tok in r.eos_ids or len(r.output_ids) >= r.max_new_tokens:
            r.state, r.t_done = DONE, now
            for st in ordered_stages(**self._stage_kw()):
                warn = st.leave(r.slot, r.sampling) if r.sampling is not None and st.wants(r.sampling) else None
                if warn:
                    print(f"[WARN] request {r.rid}: {warn}", flush=True)
            mb = r.slot // self.B
            self.kv_held.pop(r.slot, None)
            del self.by_slot[r.slot]
            self.cur_tok.pop(r.slot, None)
            self.pending_resets[mb].append(r.slot)
            self.finished.append(r)
        else:
            self.cur_tok[r.slot] = tok

    def _collect(self, mb: int) -> None:
        """Receive/process the return of micro-batch ``mb``'s outstanding command."""
        with self._mb_ctx(mb):
            self._collect_body(mb)

    def _collect_body(self, mb: int) -> None:
        o = self.outstanding[mb]
        if o is None:
            return
        self.outstanding[mb] = None
        kind, info, local = o
        if kind == CMD_PREFILL:
            emitted = [r for r in info if r is not None]
            if not emitted:
                return
            if local is None:
                buf = torch.zeros(len(emitted), dtype=torch.int32, device=self.device)
                self.p2p.recv(buf, self.world - 1)
                toks = buf.tolist()
            else:
                toks = self._host_list(local)
            now = time.perf_counter()
            lps = self._take_logprobs(mb)
            for r, t in zip(emitted, toks):
                r.state = DECODING
                if self.graph_mode:
                    self.graphs[mb].tokens[r.slot - mb * self.B] = t
                self._record_logprobs(r, lps.get(r.slot))
                self._emit(r, int(t), now)
        elif kind == CMD_DECODE:
            if local is None:
                if self.graph_mode:
                    g = self.graphs[mb]
                    self.p2p.recv(g.tokens, self.world - 1)  # next step's input ids, in place
                    toks = g.tokens.tolist()
                else:
                    buf = torch.zeros(len(info), dtype=torch.int32, device=self.device)
                    self.p2p.recv(buf, self.world - 1)
                    toks = buf.tolist()
            else:
                toks = self._host_list(local)
            now = time.perf_counter()
            lps = self._take_logprobs(mb)
            if self.graph_mode:
                for i, s in enumerate(self._slots(mb)):
                    r = self.by_slot.get(s)
                    if r is not None and r.state == DECODING and r.rid in info:
                        self._record_logprobs(r, lps.get(s))
                        self._emit(r, int(toks[i]), now)
            else:
                for (s, rid), t in zip(info, toks):
                    r = self.by_slot.get(s)
                    if r is not None and r.rid == rid:
                        self._record_logprobs(r, lps.get(s))
                        self._emit(r, int(t), now)

    def _schedule(self, mb: int) -> bool:
        """Issue the next command for ``mb``. Returns False if it has nothing to do."""
        resets = self.pending_resets[mb]
        # admission: waiting requests into free slots (held back while a re-plan drains)
        for s in self._free_slots(mb):
            if not self.waiting or self._replan is not None:
                break
            if self.kv_paged:  # admission by reservation: the head of the queue waits for its pages, in place
                need = self.kv_pool.pages_for(len(self.waiting[0].input_ids) + self.waiting[0].max_new_tokens)
                if sum(self.kv_held.values()) + need > self.kv_pages - 1:
                    break
                self.kv_held[s] = need
            r = self.waiting.pop(0)
            if r.sampling is not None:
                want = {c.name: c.wants(r.sampling) for c in STAGE_CLASSES}
                if not self.sampling_on:
                    self._enable_sampling(logprobs=r.sampling.logprobs is not None, **want)
                for name in (n for n in STAGE_ORDER if want[n] and getattr(self, n) is None):
                    self._enable_stage(name)
                if r.sampling.logprobs is not None and not self.logprobs_on:
                    self._enable_logprobs()
            r.slot, r.state, r.prefilled = s, PREFILLING, 0
            self.by_slot[s] = r
            if s in resets and not self.kv_paged:
                # (paged: the reset always travels with this call's command, the new request's first
                # prefill item may not - the budget - and the old request's pages are released by the
                # reset alone: its reservation was dropped on rank 0 when it finished)
                resets.remove(s)
            if self.P:
                self._attach(r)
        fills = []
        if self.P:
            self._issue_forks(mb)
            # requests of mb whose pool entry is still to be filled: the fill rides with mb's prefills
            fills = [r.entry for r in (self.by_slot.get(s) for s in self._slots(mb))
                     if r is not None and r.state == FORKING and r.entry.filler is r and not r.entry.ready]
        self.peak_in_flight = max(self.peak_in_flight, len(self.by_slot))
        pre = [self.by_slot[s] for s in self._slots(mb) if s in self.by_slot and self.by_slot[s].state == PREFILLING]
        if pre or fills:
            items, ids, info, budget = [], [], [], self.budget
            filled = []
            for e in fills:  # ordinary prefill items (pool_slot, p0, n, 0), chunked by the budget
                if budget <= 0:
                    break
                n = min(e.length - e.filled, budget)
                if e.filled == 0 and self.S > 1:  # the forks that still read the evicted entry's slot
                    i = e.slot - self.B * self.M
                    with self._mb_ctx(mb):
                        for ev in self._pool_reads[i]:
                            torch.cuda.current_stream(self.device).wait_event(ev)
                    self._pool_reads[i] = []
                items.append((e.slot, e.filled, n, 0))
                ids += e.tokens[e.filled:e.filled + n]
                info.append(None)
                e.filled += n
                budget -= n
                if e.filled == e.length:
                    filled.append(e)
            for r in pre:
                if budget <= 0:
                    break
                n = min(len(r.input_ids) - r.prefilled, budget)
                emit = int(r.prefilled + n == len(r.input_ids))
                items.append((r.slot, r.prefilled, n, emit))
                ids += r.input_ids[r.prefilled:r.prefilled + n]
                info.append(r if emit else None)
                r.prefilled += n
                budget -= n
            self._issue(CMD_PREFILL, mb, items, resets, ids, info)
            for e in filled:  # every command issued from here on is ordered behind the whole fill
                e.ready, e.filler = True, None
                if self.S > 1:
                    with self._mb_ctx(mb):
                        e.fill_event = torch.cuda.Event()
                        e.fill_event.record()
            return True
        dec = [self.by_slot[s] for s in self._slots(mb) if s in self.by_slot and self.by_slot[s].state == DECODING]
        if dec:
            if self.graph_mode:
                items = [(s, 0, 1, 0) for s in self._slots(mb)]
                info = {r.rid for r in dec}
                ids = None
            else:
                items = [(r.slot, len(r.input_ids) + len(r.output_ids) - 1, 1, 1) for r in dec]
                info = [(r.slot, r.rid) for r in dec]
                ids = [self.cur_tok[r.slot] for r in dec]
            self._issue(CMD_DECODE, mb, items, resets, ids, info)
            return True
        if resets:  # nothing to run, but keep device positions tidy on every rank
            self._issue(CMD_DECODE, mb, [], resets, None, None, run=False)
        return False

    def _issue(self, cmd, mb, items, resets, ids, info, run: bool = True):
        hdr = self.hdr.pack(cmd if run else 0, mb, items, resets)
        self.pending_resets[mb] = []
        self._bcast_header(hdr)
        if not run:
            with self._mb_ctx(mb):
                self._apply_resets(resets)
            return
        local = self._exec(cmd, mb, items, resets, ids=ids)
        self.outstanding[mb] = (cmd, info, local)

    def _busy(self) -> bool:
        return bool(self.waiting or self.by_slot or any(o is not None for o in self.outstanding)
                    or not self.incoming.empty() or self._replan is not None)

    # ------------------------------------------------------------------ main loops
    def serve(self, stop_when_idle: bool = True, idle_sleep_s: float = 0.0005,
              should_stop: Optional[Callable[[], bool]] = None) -> None:
        """Rank 0: schedule until idle (or ``should_stop()``), then stop every rank.
        Other ranks: execute rank 0's commands until STOP."""
        if not self.first:
            self._follow()
            return
        self.t_start = self.t_start or time.perf_counter()
        while True:
            if self._replan is not None and not self.by_slot and all(o is None for o in self.outstanding):
                self._apply_replan()  # drained: every stage moves to the new split together
            self._intake()
            any_work = False
            for mb in range(self.M):
                self._collect(mb)
                self._intake()
                any_work |= self._schedule(mb)
            if not any_work and not self._busy():
                if stop_when_idle or (should_stop is not None and should_stop()):
                    break
                time.sleep(idle_sleep_s)
        self.stop()

    def stop(self) -> None:
        tracing.export_env(self.tl)
        if self.first:
            self._bcast_header(self.hdr.pack(CMD_STOP, 0))
            for w, _ in self._ctrl_works:
                w.wait()
            self._ctrl_works.clear()
        self._flush_sends()
        if self.gpu:
            torch.cuda.synchronize(self.device)

    def _follow(self) -> None:
        import torch.distributed as dist
        hdr = torch.zeros(self.hdr.size, dtype=torch.int32)
        while True:
            dist.recv(hdr, 0, group=self.ctrl)
            if int(hdr[0]) == CMD_REPLAN:
                b = hdr[4:4 + int(hdr[2])].tolist()
                self._reshard(b[self.rank], b[self.rank + 1])
                continue
            cmd, mb, items, resets = _Header.unpack(hdr)
            if cmd == CMD_STOP:
                break
            if cmd == 0:
                self._apply_resets(resets)
                continue
            self._exec(cmd, mb, items, resets)
        self._flush_sends()
        if self.gpu:
            torch.cuda.synchronize(self.device)
        tracing.export_env(self.tl)

    # ------------------------------------------------------------------ convenience
    def generate(self, prompts: List[List[int]], max_new_tokens: int = 32, eos_ids=()) -> List[List[int]]:
        """Rank 0: submit ``prompts``, serve until all are done, return their outputs in order.
        (Other ranks must call :meth:`serve` concurrently.)"""
        rids = [self.submit(p, max_new_tokens, eos_ids=eos_ids) for p in prompts]
        self.serve(stop_when_idle=True)
        return [self.requests[r].output_ids for r in rids]

    def stats(self) -> dict:
        done = [r for r in self.finished]
        el = time.perf_counter() - (self.t_start or time.perf_counter())
        return {
            "requests": len(done),
            "tokens": self.tokens_generated,
            "elapsed_s": el,
            "tok_s": self.tokens_generated / el if el > 0 else 0.0,
            "ttft_ms_p50": _percentile([r.ttft_ms for r in done], 0.5),
            "tpot_ms_p50": _percentile([r.tpot_ms for r in done if len(r.output_ids) > 1], 0.5),
            "tpot_ms_p90": _percentile([r.tpot_ms for r in done if len(r.output_ids) > 1], 0.9),
            "peak_in_flight": self.peak_in_flight,  # most requests holding a slot at once
            # prefix pool: requests that forked K/V computed for another request and the prefill tokens
            # that saved them, pool entries filled / evicted, declared prefixes that found every slot pinned
            **self.prefix_stats,
        }


__all__ = ["PipelineServer", "Request", "SamplingParams"]
