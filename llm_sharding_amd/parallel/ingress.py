"""Request ingress of a PipelineServer (rank 0): the reference's ``user_request`` control
messages (``utils/node_worker.send_user_request``; the reference itself never reads requests in
serve mode) turned into ``PipelineServer.submit`` calls, and finished requests
pushed back to the client's ``reply_to`` address.

Used by ``serve.py`` (its own ingress port) and by :class:`..utils.node_worker.NodeController`
in pipeline mode (the controller's config port, when the master deploys the RCCL pipeline)."""
from __future__ import annotations

import json
import threading
from typing import Callable, Optional

from ..runtime.sampling import SamplingParams
from . import protocol
from .transport import Again, PullSocket, PushSocket


class Replies:
    """on_token callback: prints each finished request and pushes ``{"request_id",
    "output_ids", "text", "ttft_ms", "tpot_ms"}`` to its ``reply_to`` address - plus a
    ``"logprobs"`` dict (``token_logprobs``, ``ranks`` and, with ``logprobs >= 1``, ``top_logprobs``:
    per token a list of ``[id, logprob]`` pairs) for a request that asked for them. The children of
    a request with ``n > 1`` are answered together, when the last one is done: the reply is child
    0's, plus a ``"choices"`` list with one such dict (and its ``"index"``) per child, in seed order.
    If some children will never finish (:meth:`error` with their ``request_id``), the finished ones
    are still sent, as soon as every child is finished or failed: the reply is then the first
    finished child's and ``"choices"`` holds the finished children only, each with the ``"index"``
    of its seed."""

    def __init__(self, tokenizer=None, verbose: bool = True, on_done: Optional[Callable] = None):
        self.tok = tokenizer
        self.verbose = verbose
        self.on_done = on_done
        self.socks: dict = {}
        # __call__ runs on the serve thread, error() on the listener thread: one lock guards the
        # socket table and the sends (one PushSocket per reply_to, never two racing creations)
        self._lock = threading.Lock()
        self._groups: dict = {}  # n > 1: groups with a finished child, waiting for their siblings

    def _group_done(self, g: dict, reply: Optional[dict], reply_to: str) -> Optional[dict]:
        """One more child of ``g`` finished (``reply``) or failed (None): the group's reply once
        every child is accounted for and at least one finished, else None."""
        with self._lock:
            if reply is not None:
                g.setdefault("replies", []).append(reply)
                self._groups[id(g)] = (g, reply_to)
            else:
                g["failed"] = g.get("failed", 0) + 1
            got = g.get("replies", [])
            if not got or len(got) + g.get("failed", 0) < g["n"]:
                return None
            self._groups.pop(id(g), None)
        rids = g.get("rids", [])
        choices = sorted(got, key=lambda c: c["request_id"])  # seed order
        return dict(choices[0], choices=[dict(c, index=rids.index(c["request_id"]) if c["request_id"] in rids else i)
                                         for i, c in enumerate(choices)])

    def _send(self, reply_to: str, payload: bytes) -> None:
        with self._lock:
            sock = self.socks.get(reply_to)
            if sock is None:
                sock = self.socks[reply_to] = PushSocket(reply_to)
            sock.send_bytes(payload)

    def __call__(self, r, t) -> None:
        if not (t in r.eos_ids or len(r.output_ids) >= r.max_new_tokens):
            return
        text = self.tok.decode(r.output_ids) if self.tok is not None else ""
        if self.verbose:
            print(f"[INFO] request {r.rid} done: {len(r.output_ids)} tokens  ttft {r.ttft_ms:.1f} ms  "
                  f"output: {text!r}", flush=True)
        if self.on_done is not None:
            self.on_done(r, text)
        if r.reply_to:
            reply = {"request_id": r.rid, "output_ids": list(r.output_ids), "text": text,
                     "ttft_ms": r.ttft_ms, "tpot_ms": r.tpot_ms}
            if getattr(r, "token_logprobs", None) is not None:
                reply["logprobs"] = {"token_logprobs": list(r.token_logprobs), "ranks": list(r.ranks)}
                if r.top_logprobs is not None:
                    reply["logprobs"]["top_logprobs"] = [[[int(i), float(v)] for i, v in t] for t in r.top_logprobs]
            g = getattr(r, "group", None)
            if g is not None and g.get("n", 1) > 1:  # a child of n samples: one reply, when the last is done
                reply = self._group_done(g, reply, r.reply_to)
                if reply is None:
                    return
            self._send(r.reply_to, protocol.encode(reply))

    def error(self, reply_to: Optional[str], reason: str, request_id=None) -> None:
        """Tell a client its request will not be served (``{"request_id", "error"}``)."""
        if self.verbose:
            print(f"[ERROR] request {request_id} not served: {reason}", flush=True)
        if not reply_to:
            return
        try:
            self._send(reply_to, protocol.encode({"request_id": request_id, "error": reason,
                                                  "output_ids": [], "text": ""}))
            with self._lock:  # a child of n samples: its finished siblings must not wait for it for ever
                hit = [(g, to) for g, to in self._groups.values() if request_id in g.get("rids", ())]
            for g, to in hit:
                reply = self._group_done(g, None, to)
                if reply is not None:
                    self._send(to, protocol.encode(reply))
        except OSError as e:
            print(f"[WARNING] error reply to {reply_to} failed: {e}", flush=True)

    def close(self) -> None:
        with self._lock:
            for s in self.socks.values():
                s.close(linger_ms=2000)
            self.socks.clear()


def decode_message(raw: bytes) -> dict:
    return json.loads(raw) if protocol.is_json_message(raw) else protocol.decode(raw)


def submit_message(srv, msg: dict, tokenizer, default_new: int, replies: Replies) -> int:
    """Submit every prompt of a ``user_request`` message (``input_ids``: one list or a batch of
    lists, else ``text`` through the tokenizer; optional ``temperature``, ``top_k``, ``top_p``,
    ``seed``: sampling instead of greedy decode, a batch's prompts each drawing their own seed
    when none is given; optional ``repetition_penalty``, ``presence_penalty``,
    ``frequency_penalty``: penalties on repeated tokens, with or without a temperature; optional
    ``logprobs`` (0..20): per-token log-probabilities, ranks and that many alternatives in the
    reply; optional ``logit_bias`` (token id, as a string or an integer, -> bias),
    ``banned_token_ids``, ``min_tokens``, ``min_p``, ``allowed_token_ids`` and ``choices`` (a list
    of token-id sequences): constrained decoding, refused with an error reply when a field is
    invalid or the automaton does not fit the server's arena; optional ``regex``: the output's bytes
    fully match the pattern (``ops.grammar``), refused with an error reply on a syntax error, a
    server without ``vocab_bytes``, a DFA that does not fit its arena or a state that allows no
    token; optional ``json_object: true`` or ``response_format: {"type": "json_object"}``: the
    output is one JSON object (``ops.pda``), refused with an error reply together with ``regex`` or
    where the server cannot serve it; optional ``cache_prefix``: the leading tokens worth keeping in the server's prefix pool;
    optional ``n > 1``: that many samples of each prompt sharing one prefill, answered with a
    ``"choices"`` list - needs a server with ``prefix_slots``). Returns the number of requests
    queued."""
    n_new = int(msg.get("max_new_tokens") or default_new)
    samples = int(msg.get("n") or 1)
    rows = msg.get("input_ids")
    if rows is None:
        if tokenizer is None:
            print("[ERROR] text request but no tokenizer", flush=True)
            return 0
        rows = [tokenizer.encode(msg.get("text", ""))]
    elif rows and not isinstance(rows[0], (list, tuple)):
        rows = [rows]
    n = 0
    for ids in rows:
        try:
            # optional temperature / top_k / top_p / seed / *_penalty / logprobs / constraint keys; absent: greedy
            # (the plain call)
            sp = SamplingParams.from_dict(msg)
            kw = {} if sp is None else {"sampling": sp}
            if samples != 1:
                n += len(srv.submit_n(ids, samples, n_new, on_token=replies, reply_to=msg.get("reply_to"), **kw))
                continue
            if msg.get("cache_prefix") is not None:
                kw["cache_prefix"] = int(msg["cache_prefix"])
            srv.submit(ids, n_new, on_token=replies, reply_to=msg.get("reply_to"), **kw)
            n += 1
        except ValueError as e:
            replies.error(msg.get("reply_to"), f"request rejected: {e}")
    return n


def run_ingress(srv, sock: PullSocket, tokenizer, stop_evt: threading.Event, default_new: int,
                replies: Replies, on_other: Optional[Callable[[dict], None]] = None,
                accepting: Optional[Callable[[], Optional[str]]] = None) -> None:
    """Read control messages from ``sock`` until ``shutdown`` (or ``stop_evt``): queue
    ``user_request`` prompts on the server; other commands go to ``on_other`` (e.g. ping).
    ``accepting()`` returning a reason string refuses new requests with an error reply (a
    pipeline being dropped after a lost rank must not swallow them)."""
    while not stop_evt.is_set():
        try:
            raw = sock.recv_bytes(timeout_ms=200)
        except Again:
            continue
        msg = decode_message(raw)
        cmd = msg.get("command") if isinstance(msg, dict) else None
        if cmd == "shutdown":
            stop_evt.set()
            break
        if cmd == "user_request":
            why = accepting() if accepting is not None else None
            if why:
                replies.error(msg.get("reply_to"), why)
                continue
            submit_message(srv, msg, tokenizer, default_new, replies)
        elif on_other is not None:
            on_other(msg)
        else:
            print(f"[WARNING] ingress: unknown message {cmd!r}", flush=True)


__all__ = ["Replies", "run_ingress", "submit_message", "decode_message"]
