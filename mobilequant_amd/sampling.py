"""Seeded device-side token selection (csrc/mq_sample.hip): SamplingParams, the packed per-row request array the
kernel reads, and the launch record both decode engines keep for their logits / position / token buffers."""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from typing import Mapping, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import (MQ_LOGPROB_MAX_TOP, MQ_LOGPROB_SCRATCH_BYTES, MQ_SAMPLE_SCRATCH_BYTES, MqLogprobTopArgs, MqSampleArgs, MqSamplePenalizedArgs,
                   MqSampleRaggedArgs, MqSampleRowsArgs)

MAX_ROWS = 8
MAX_VOCAB = 1 << 20
ROW_DTYPE = np.dtype([("temperature", "<f4"), ("top_k", "<i4"), ("top_p", "<f4"), ("min_p", "<f4"), ("seed", "<u8"), ("stream", "<u8")])
assert ROW_DTYPE.itemsize == ctypes.sizeof(_lib.MqSampleRow) == 32
PENALTY_DTYPE = np.dtype([("repetition", "<f4"), ("presence", "<f4"), ("frequency", "<f4"), ("reserved", "<i4")])
assert PENALTY_DTYPE.itemsize == ctypes.sizeof(_lib.MqSamplePenaltyRow) == 16
HISTORY_PROMPT_BIT = 1 << 31                      # a history entry: bit 31 = in the prompt, bits 0..15 = times generated (saturating)
HISTORY_DTYPES = (torch.int32, getattr(torch, "uint32", torch.int32))


def _f32(v) -> np.float32:
    with np.errstate(over="ignore"):
        return np.float32(v)


@dataclass(frozen=True)
class SamplingParams:
    """temperature >= 0 (0 = greedy), top_k >= 0 (0 = off), top_p in (0, 1] (1 = off), min_p in [0, 1) (0 = off), seed in [0, 2^64).
    Filters compose in the usual order: temperature, top-k, top-p, min-p.  With a seed, a stream (the sequence's identity) and the
    position, the drawn token is a property of the sequence: the same in any batch, in any slot, captured or not.
    In front of them (step 0 of the rule), from the sequence's own tokens: repetition_penalty > 0 (1 = off; a positive
    logit of a token of the prompt or of the generated text is divided by it, a negative one multiplied: transformers'
    RepetitionPenaltyLogitsProcessor), presence_penalty and frequency_penalty (0 = off; subtracted once, and once per occurrence, for
    tokens generated so far: the OpenAI / vLLM definition) and logit_bias {token id: added value} (-inf bans a token; stored as a sorted
    tuple of pairs, so the request stays hashable)."""
    temperature: float = 1.0
    top_k: int = 0
    top_p: float = 1.0
    min_p: float = 0.0
    seed: int = 0
    repetition_penalty: float = 1.0
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    logit_bias: Optional[Mapping[int, float]] = None

    def __post_init__(self):
        t, k, p, m, s = self.temperature, self.top_k, self.top_p, self.min_p, self.seed
        if isinstance(t, bool) or not isinstance(t, (int, float)) or not (math.isfinite(t) and t >= 0):
            raise ValueError(f"SamplingParams: temperature={t!r} must be a finite number >= 0 (0 = greedy)")
        if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k < 2 ** 31:
            raise ValueError(f"SamplingParams: top_k={k!r} must be an int in [0, 2^31) (0 = off)")
        if isinstance(p, bool) or not isinstance(p, (int, float)) or not 0 < p <= 1:
            raise ValueError(f"SamplingParams: top_p={p!r} must be in (0, 1] (1 = off)")
        if isinstance(m, bool) or not isinstance(m, (int, float)) or not 0 <= m < 1:
            raise ValueError(f"SamplingParams: min_p={m!r} must be in [0, 1) (0 = off)")
        if isinstance(s, bool) or not isinstance(s, int) or not 0 <= s < 2 ** 64:
            raise ValueError(f"SamplingParams: seed={s!r} must be an int in [0, 2^64)")
        if np.float32(p) <= 0 or np.float32(m) >= 1:
            raise ValueError("SamplingParams: top_p / min_p leave their range when rounded to fp32")
        r, a, f, lb = self.repetition_penalty, self.presence_penalty, self.frequency_penalty, self.logit_bias
        if isinstance(r, bool) or not isinstance(r, (int, float)) or not (math.isfinite(r) and r > 0) or not 0 < _f32(r) < np.inf:
            raise ValueError(f"SamplingParams: repetition_penalty={r!r} must be a finite number > 0 in fp32 (1 = off)")
        for name, v in (("presence_penalty", a), ("frequency_penalty", f)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or not np.isfinite(_f32(v)):
                raise ValueError(f"SamplingParams: {name}={v!r} must be a finite number in fp32 (0 = off)")
        if lb is not None:
            items = lb.items() if isinstance(lb, Mapping) else lb
            pairs = []
            try:
                for t, v in items:
                    if isinstance(t, bool) or not isinstance(t, (int, np.integer)) or int(t) < 0:
                        raise ValueError(f"SamplingParams: logit_bias token id {t!r} must be an int >= 0")
                    if isinstance(v, bool) or not isinstance(v, (int, float, np.floating)) or math.isnan(v) or v == math.inf:
                        raise ValueError(f"SamplingParams: logit_bias[{t}]={v!r} must be a number below +inf (-inf bans the token)")
                    pairs.append((int(t), float(v)))
            except TypeError:
                raise ValueError(f"SamplingParams: logit_bias={lb!r} must map token ids to numbers") from None
            pairs.sort()
            if any(p[0] == q[0] for p, q in zip(pairs, pairs[1:])):
                raise ValueError("SamplingParams: logit_bias names a token id twice")
            object.__setattr__(self, "logit_bias", tuple(pairs) or None)

    @property
    def penalized(self) -> bool:
        """Any of repetition_penalty, presence_penalty, frequency_penalty, logit_bias is active (step 0 of the rule runs)."""
        return np.float32(self.repetition_penalty) != 1 or np.float32(self.presence_penalty) != 0 or np.float32(self.frequency_penalty) != 0 \
            or self.logit_bias is not None


def check_stream(stream) -> int:
    if isinstance(stream, bool) or not isinstance(stream, (int, np.integer)) or not 0 <= int(stream) < 2 ** 64:
        raise ValueError(f"sampling: stream={stream!r} must be an int in [0, 2^64)")
    return int(stream)


def pack_rows(params: Sequence[SamplingParams], streams: Sequence[int]) -> np.ndarray:
    """The mq_sample_row array (host side) for these requests."""
    if len(params) != len(streams):
        raise ValueError(f"sampling: {len(params)} SamplingParams for {len(streams)} streams")
    rows = np.zeros(len(params), dtype=ROW_DTYPE)
    for r, (p, s) in enumerate(zip(params, streams)):
        if not isinstance(p, SamplingParams):
            raise TypeError(f"sampling: expected SamplingParams, got {type(p).__name__}")
        rows[r] = (p.temperature, p.top_k, p.top_p, p.min_p, p.seed, check_stream(s))
    return rows


def pack_penalty_rows(params: Sequence) -> np.ndarray:
    """The mq_sample_penalty_row array (host side): SamplingParams or (repetition, presence, frequency) per row."""
    rows = np.zeros(len(params), dtype=PENALTY_DTYPE)
    for r, p in enumerate(params):
        rows[r] = (p.repetition_penalty, p.presence_penalty, p.frequency_penalty, 0) if isinstance(p, SamplingParams) else (*p, 0)
    return rows


def _check_ids(ids, V: int) -> torch.Tensor:
    t = torch.as_tensor([int(i) for i in ids], dtype=torch.int64)
    if t.numel() and (int(t.min()) < 0 or int(t.max()) >= V):
        raise ValueError(f"sampling: a token id outside [0, {V}) in the history")
    return t


def history_prompt(history_row: torch.Tensor, ids, clear: bool = True):
    """mq_sample_history_prompt on one row's history ([V] int32 device tensor holding the uint32 entries): clear it, then mark the ids
    as prompt tokens (bit 31).  The ids are checked here, on the host: one outside [0, V) raises ValueError."""
    V = history_row.numel()
    if history_row.dtype not in HISTORY_DTYPES or not history_row.is_contiguous():
        raise RuntimeError("mobilequant_amd: a history row must be a contiguous int32 (uint32 bits) tensor")
    dev = history_row.device
    t = _check_ids(ids, V).to(dev)
    with torch.cuda.device(dev):
        _lib.call("mq_sample_history_prompt", history_row.data_ptr(), V, t.data_ptr() if t.numel() else None, t.numel(), int(bool(clear)),
                  torch.cuda.current_stream(dev).cuda_stream)


def _check_count(who: str, delta, history, history_ok: bool, history_form: str, ids, ids_name: str, ids_ok: bool, ids_form: str):
    """The checks of the two history_count functions, in their order: delta, the history (its form, then its device), the ids."""
    if isinstance(delta, bool) or delta not in (1, -1):
        raise ValueError(f"mobilequant_amd: {who} delta={delta!r} must be +1 or -1")
    if not history_ok:
        raise RuntimeError(f"mobilequant_amd: {who} history must be {history_form}")
    if not history.is_cuda:
        raise RuntimeError(f"mobilequant_amd: {who} history must be a ROCm device tensor; there is no CPU path")
    if not ids_ok:
        raise RuntimeError(f"mobilequant_amd: {who} {ids_name} must be a contiguous {ids_form}")
    if ids.device != history.device:
        raise RuntimeError(f"mobilequant_amd: {who} {ids_name} must be a ROCm device tensor on the history's device")


def _is_row(t, dtypes, V: int) -> bool:
    return isinstance(t, torch.Tensor) and t.dtype in dtypes and t.dim() == 1 and t.numel() >= V and t.is_contiguous()


def _is_ids(t, dim: int) -> bool:
    return isinstance(t, torch.Tensor) and t.dtype == torch.int64 and t.dim() == dim and t.is_contiguous()


def history_count(history_row: torch.Tensor, ids: torch.Tensor, delta: int):
    """mq_sample_history_count on one row's history ([V] int32 device tensor holding the uint32 entries): the count (bits 0..15) of every
    id in `ids` (an int64 device tensor, any number; ids repeat) moves by delta = +1 or -1, saturating at 65 535 and at 0.  Bit 31 is kept
    and an id outside [0, V) is ignored on the device: no id is read on the host.  One launch, capturable."""
    h = history_row
    _check_count("history_count", delta, h, _is_row(h, HISTORY_DTYPES, 0), "one contiguous int32 (uint32 bits) row [V]",
                 ids, "ids", _is_ids(ids, 1), "int64 [n] tensor")
    with torch.cuda.device(h.device):
        _lib.call("mq_sample_history_count", h.data_ptr(), h.numel(), ids.data_ptr() if ids.numel() else None, ids.numel(), int(delta),
                  torch.cuda.current_stream(h.device).cuda_stream)
    return history_row


def _fill_shared(a, logits: torch.Tensor, rows: int, params: torch.Tensor, tok: torch.Tensor, scratch: torch.Tensor,
                 kept: Optional[torch.Tensor] = None, logprob: Optional[torch.Tensor] = None):
    """The fields every mq_sample* argument struct shares, over the first `rows` rows of logits [>= rows, V].  Returns a."""
    V = logits.shape[1]
    a.logits, a.logits_stride, a.V, a.rows = logits.data_ptr(), logits.stride(0) if logits.shape[0] > 1 else max(V, logits.stride(0)), V, rows
    a.params, a.tok = params.data_ptr(), tok.data_ptr()
    a.kept = kept.data_ptr() if kept is not None else None
    a.logprob = logprob.data_ptr() if logprob is not None else None
    a.scratch, a.scratch_bytes = scratch.data_ptr(), MQ_SAMPLE_SCRATCH_BYTES
    return a


class SampleLaunch:
    """mq_sample over an engine's own buffers: logits [rows, V] -> tok [rows] at the positions in pos [rows].  The per-row requests
    live in a device array that set_rows() rewrites in place, so a captured launch serves any request.
    The first request with a penalty or a bias allocates the rows' histories [rows, V], penalty rows and dense bias rows; from then on,
    while any row's request is penalised, launch() is mq_sample_penalized (which also counts every drawn token in its row's history),
    and while every row is neutral it is mq_sample, as before.  `penalized` says which: a captured graph holds one of the two."""

    def __init__(self, logits: torch.Tensor, pos: torch.Tensor, tok: torch.Tensor, cache_len: int):
        lg = logits.view(-1, logits.shape[-1])
        rows, V = lg.shape
        dev = logits.device
        self.rows, self.dev = rows, dev
        self.params = torch.zeros(rows * ROW_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.scratch = torch.zeros(MQ_SAMPLE_SCRATCH_BYTES, dtype=torch.uint8, device=dev)
        self.args = a = _fill_shared(MqSampleArgs(), lg, rows, self.params, tok, self.scratch)
        a.pos, a.cache_len = pos.data_ptr(), int(cache_len)
        self._keep = (lg, pos, tok)
        self.V = V
        self.penalized = False
        self.pargs = None                                       # mq_sample_penalized's block and buffers: allocated on first need
        self.set_rows([SamplingParams(temperature=0.0)] * rows, list(range(rows)))

    def set_rows(self, params: Sequence[SamplingParams], streams: Sequence[int]):
        host = pack_rows(params, streams)
        if len(host) != self.rows:
            raise ValueError(f"sampling: {len(host)} requests for {self.rows} rows")
        self.params.copy_(torch.from_numpy(host.view(np.uint8).reshape(-1)))
        self.penalized = any(p.penalized for p in params)
        if self.penalized or self.pargs is not None:
            self._set_penalty_rows(params)

    def _allocate_penalty(self):
        rows, V, dev = self.rows, self.V, self.dev
        self.history = torch.zeros(rows, V, dtype=torch.int32, device=dev)              # uint32 entries
        self.penalty = torch.zeros(rows * PENALTY_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.bias = torch.zeros(rows, V, dtype=torch.float32, device=dev)
        self.bias_ptr = torch.zeros(rows, dtype=torch.int64, device=dev)                # per row: its bias row, or NULL
        self._bias_of = [None] * rows
        p = MqSamplePenalizedArgs()
        ctypes.memmove(ctypes.byref(p.s), ctypes.byref(self.args), ctypes.sizeof(MqSampleArgs))
        p.penalty, p.history, p.history_stride = self.penalty.data_ptr(), self.history.data_ptr(), self.history.stride(0)
        p.bias, p.observe = self.bias_ptr.data_ptr(), 1
        self.pargs = p

    def _set_penalty_rows(self, params: Sequence[SamplingParams]):
        if self.pargs is None:
            self._allocate_penalty()
        self.penalty.copy_(torch.from_numpy(pack_penalty_rows(params).view(np.uint8).reshape(-1)))
        ptrs = []
        for r, p in enumerate(params):
            lb = p.logit_bias
            if lb != self._bias_of[r]:
                self.bias[r].zero_()
                if lb is not None:
                    ids = _check_ids([t for t, _ in lb], self.V).to(self.dev)
                    self.bias[r].index_copy_(0, ids, torch.tensor([v for _, v in lb], dtype=torch.float32, device=self.dev))
                self._bias_of[r] = lb
            ptrs.append(self.bias[r].data_ptr() if lb is not None else 0)
        self.bias_ptr.copy_(torch.tensor(ptrs, dtype=torch.int64))

    def observe_prompt(self, row: int, ids, clear: bool = True):
        """Mark ids as prompt tokens of the row's sequence (clear: forget the row's history first).  Only a penalised launch reads the
        histories, so this does nothing until the first penalised request has allocated them."""
        if self.pargs is not None:
            history_prompt(self.history[row], ids, clear)

    def clear_history(self, row: int):
        self.observe_prompt(row, (), clear=True)

    def launch(self):
        """On the current stream (capturable: two kernel launches, nothing else)."""
        st = torch.cuda.current_stream(self.dev).cuda_stream
        if self.penalized:
            _lib.call("mq_sample_penalized", ctypes.byref(self.pargs), st)
        else:
            _lib.call("mq_sample", ctypes.byref(self.args), st)


class RowsLaunch:
    """mq_sample_rows over an engine's multi-token step: rows logits [R, V] of ONE sequence -> out [R], row j drawn at
    *pos + n_offset + j under the single request of `sampler` (a one-row SampleLaunch: its device request, penalty row, bias row and
    history are read in place, so a captured launch serves any request of the same kind).  proposals: the int64 device ids in front of
    rows 1 .. R - 1.  One argument block per (row count, penalised): a penalised block names the sampler's penalty row, its history and
    its dense bias row (zeros without a logit_bias: adding +0 leaves every z of the rule as it is)."""

    def __init__(self, sampler: "SampleLaunch", logits: torch.Tensor, pos: torch.Tensor, proposals: torch.Tensor, out: torch.Tensor):
        if sampler.rows != 1:
            raise ValueError("sampling: RowsLaunch serves one sequence (a one-row SampleLaunch)")
        self.sampler, self.logits, self.pos, self.proposals, self.out = sampler, logits, pos, proposals, out
        self.scratch = torch.zeros(MQ_SAMPLE_SCRATCH_BYTES, dtype=torch.uint8, device=logits.device)
        self._args = {}

    def args(self, T: int, penalized: bool) -> MqSampleRowsArgs:
        a = self._args.get((T, penalized))
        if a is None:
            s = self.sampler
            a = _fill_shared(MqSampleRowsArgs(), self.logits, T, s.params, self.out, self.scratch)
            a.n_base, a.n_offset = self.pos.data_ptr(), 1 - T
            a.proposals = self.proposals.data_ptr() if T > 1 else None
            if penalized:
                a.penalty, a.history, a.bias = s.penalty.data_ptr(), s.history[0].data_ptr(), s.bias[0].data_ptr()
            self._args[(T, penalized)] = a
        return a

    def launch(self, T: int):
        """On the current stream (capturable).  Reads the position BEHIND the T-row step: row j draws at pos - T + 1 + j."""
        a = self.args(T, self.sampler.penalized)
        _lib.call("mq_sample_rows", ctypes.byref(a), torch.cuda.current_stream(self.logits.device).cuda_stream)


class RaggedRowsLaunch:
    """mq_sample_ragged over a batched engine's ragged step: rows logits [R, V] of up to `batch` sequences -> out [R];
    the row table (row_seq, row_pos: device int32) and the rows' tokens (row_tok: device int64) are the step's own.  A live row of
    sequence s at position p is drawn at p + n_offset under request s of `sampler` (a batch SampleLaunch: its device requests, penalty
    rows, histories and bias pointers are read in place, so a captured launch serves any plan and any requests of the same kind).  One
    argument block per (row count, penalised): a penalised block names the sampler's penalty rows, histories and bias pointers."""

    def __init__(self, sampler: "SampleLaunch", logits: torch.Tensor, row_seq: torch.Tensor, row_pos: torch.Tensor, row_tok: torch.Tensor,
                 out: torch.Tensor, cache_len: int, n_offset: int = 1):
        self.sampler, self.logits, self.out = sampler, logits, out
        self.row_seq, self.row_pos, self.row_tok = row_seq, row_pos, row_tok
        self.cache_len, self.n_offset = int(cache_len), int(n_offset)
        self.scratch = torch.zeros(MQ_SAMPLE_SCRATCH_BYTES, dtype=torch.uint8, device=logits.device)
        self._args = {}

    def args(self, R: int, penalized: bool) -> MqSampleRaggedArgs:
        a = self._args.get((R, penalized))
        if a is None:
            s = self.sampler
            a = _fill_shared(MqSampleRaggedArgs(), self.logits, R, s.params, self.out, self.scratch)
            a.batch, a.cache_len, a.n_offset = s.rows, self.cache_len, self.n_offset
            a.row_seq, a.row_pos, a.row_tok = self.row_seq.data_ptr(), self.row_pos.data_ptr(), self.row_tok.data_ptr()
            if penalized:
                a.penalty, a.history, a.history_stride, a.bias = s.penalty.data_ptr(), s.history.data_ptr(), s.history.stride(0), s.bias_ptr.data_ptr()
            self._args[(R, penalized)] = a
        return a

    def launch(self, R: int):
        """On the current stream (capturable: kernel launches, nothing else)."""
        a = self.args(R, self.sampler.penalized)
        _lib.call("mq_sample_ragged", ctypes.byref(a), torch.cuda.current_stream(self.logits.device).cuda_stream)


class TokenLogprobs(NamedTuple):
    """The records of T tokens (CPU tensors; csrc/mq_logprob.hip's rule): logprob [T] fp32, the log-softmax of the RAW
    logits row (no temperature, penalty or bias) at the chosen token; rank [T] int32, its place in that row (1 = the top token);
    top_id [T, n] int32 and top_logprob [T, n] fp32, the row's first n tokens (logit descending, ties by index) and their
    log-probabilities."""
    logprob: torch.Tensor
    rank: torch.Tensor
    top_id: torch.Tensor
    top_logprob: torch.Tensor


def check_logprobs(who: str, logprobs, sampling) -> Optional[int]:
    """generate(logprobs=...): None, or an int in 0 .. 20 together with sampling= (the records are written behind the sample launch;
    the plain greedy, do_sample and generate(draft=...) paths pick their tokens with torch and stay as they are)."""
    if logprobs is None:
        return None
    if isinstance(logprobs, bool) or not isinstance(logprobs, (int, np.integer)) or not 0 <= int(logprobs) <= MQ_LOGPROB_MAX_TOP:
        raise ValueError(f"{who}: logprobs={logprobs!r} must be None or an int in 0..{MQ_LOGPROB_MAX_TOP} (the number of alternatives per token)")
    if sampling is None:
        raise ValueError(f"{who}: logprobs= needs sampling= (the records are written behind the device-side selection; for greedy "
                         f"decoding pass sampling=SamplingParams(temperature=0))")
    return int(logprobs)


class LogprobLaunch:
    """mq_logprob_top behind an engine's selection launches: the record buffers logprob / rank [batch, cache_len] and
    top_id / top_logprob [batch, cache_len, n_top], and one argument block per way the samplers address rows -- the engine's own
    logits / pos / tok (mq_sample's form), the T rows of a multi-token step (mq_sample_rows' form) and the R rows of a ragged step
    (mq_sample_ragged's form).  A live row's record goes to [its sequence][its token index], computed on the device: a captured launch
    moves on by itself, and a speculative round's rejected rows are overwritten when their index is drawn again."""

    def __init__(self, logits: torch.Tensor, pos: torch.Tensor, tok: torch.Tensor, cache_len: int, n_top: int,
                 scratch: Optional[torch.Tensor] = None):
        lg = logits.view(-1, logits.shape[-1])
        self.batch, self.cache_len, self.n_top, self.dev = lg.shape[0], int(cache_len), int(n_top), logits.device
        B, L, n, dev = self.batch, self.cache_len, self.n_top, self.dev
        self.logprob = torch.full((B, L), float("nan"), dtype=torch.float32, device=dev)
        self.rank = torch.zeros(B, L, dtype=torch.int32, device=dev)
        self.top_id = torch.full((B, L, n), -1, dtype=torch.int32, device=dev)
        self.top_logprob = torch.full((B, L, n), float("-inf"), dtype=torch.float32, device=dev)
        # (an engine's launches of every n_top run one after the other on one stream: they share its scratch)
        self.scratch = scratch if scratch is not None else torch.zeros(MQ_LOGPROB_SCRATCH_BYTES, dtype=torch.uint8, device=dev)
        self._keep = [lg, pos, tok]
        self.args = self._block(lg, B, tok, pos=pos.data_ptr())
        self._row_args = {}
        # one launch with every row idle, outside any capture: the kernels' code is loaded before a graph records them; nothing is written
        idle = torch.full((B,), self.cache_len, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _lib.call("mq_logprob_top", ctypes.byref(self._block(lg, B, tok, pos=idle.data_ptr())), torch.cuda.current_stream(dev).cuda_stream)
            torch.cuda.current_stream(dev).synchronize()

    def _block(self, lg: torch.Tensor, rows: int, tok: torch.Tensor, **index) -> MqLogprobTopArgs:
        a = MqLogprobTopArgs()
        a.logits, a.logits_stride, a.V, a.rows, a.n_top, a.tok = lg.data_ptr(), lg.stride(0), lg.shape[1], rows, self.n_top, tok.data_ptr()
        a.batch, a.cache_len, a.record_len = self.batch, self.cache_len, self.cache_len
        a.logprob, a.rank = self.logprob.data_ptr(), self.rank.data_ptr()
        if self.n_top:
            a.top_id, a.top_logprob = self.top_id.data_ptr(), self.top_logprob.data_ptr()
        a.scratch, a.scratch_bytes = self.scratch.data_ptr(), MQ_LOGPROB_SCRATCH_BYTES
        for k, v in index.items():
            setattr(a, k, v)
        return a

    def launch(self):
        """Behind mq_sample / mq_sample_penalized on the engine's logits, pos and tok; on the current stream (capturable)."""
        _lib.call("mq_logprob_top", ctypes.byref(self.args), torch.cuda.current_stream(self.dev).cuda_stream)

    def _row_block(self, sel, rows: int, make) -> MqLogprobTopArgs:
        """The argument block behind `sel` at this row count.  A block holds raw pointers into sel's buffers, and an engine that
        lowers its row chain again (refresh_grids, a stale grid) allocates new row buffers and builds a new selection launch: a block
        is therefore cached WITH the selection launch it was made for (which keeps those buffers alive) and made again for another."""
        held = self._row_args.get(rows)
        if held is None or held[0] is not sel:
            held = self._row_args[rows] = (sel, make())
        return held[1]

    def launch_rows(self, sel: "RowsLaunch", T: int):
        """Behind sel.launch(T) (mq_sample_rows): the same rows, the same base index, the tokens it drew."""
        a = self._row_block(sel, T, lambda: self._block(sel.logits, T, sel.out, n_base=sel.pos.data_ptr(), n_offset=1 - T))
        _lib.call("mq_logprob_top", ctypes.byref(a), torch.cuda.current_stream(self.dev).cuda_stream)

    def launch_ragged(self, sel: "RaggedRowsLaunch", R: int):
        """Behind sel.launch(R) (mq_sample_ragged): the same rows and row table, the tokens it drew."""
        a = self._row_block(sel, R, lambda: self._block(sel.logits, R, sel.out, row_seq=sel.row_seq.data_ptr(), row_pos=sel.row_pos.data_ptr(),
                                                        n_offset=sel.n_offset))
        _lib.call("mq_logprob_top", ctypes.byref(a), torch.cuda.current_stream(self.dev).cuda_stream)

    def records(self, seq: int, start: int, stop: int) -> TokenLogprobs:
        """The records [start, stop) of sequence seq, read back (the only host reads of this class)."""
        if not 0 <= seq < self.batch or not 0 <= start <= stop <= self.cache_len:
            raise ValueError(f"logprob records [{start}, {stop}) of sequence {seq} outside [0, {self.cache_len}] x {self.batch} sequences")
        return TokenLogprobs(self.logprob[seq, start:stop].cpu(), self.rank[seq, start:stop].cpu(), self.top_id[seq, start:stop].cpu(),
                             self.top_logprob[seq, start:stop].cpu())


def validate_generate_args(who: str, sampling, do_sample: bool, draft=None):
    if do_sample:
        raise ValueError(f"{who}: sampling= and do_sample=True are two different selection rules; pass one of them")
    if draft is not None:
        raise ValueError(f"{who}: a draft is for greedy decoding only (sampling= with a draft)")


# ---- the checks of the one-shot functions, by the caller's name ----------------------------------------------------------------------
# Every check of a value or a type runs before the first check of a device (_place): a call that is wrong in both ways reports the former.
def _check_logits(who: str, logits):
    """-> (logits [rows, V], rows, V); 1-D logits are one row."""
    if isinstance(logits, torch.Tensor) and logits.dim() == 1:
        logits = logits.view(1, -1)
    if not isinstance(logits, torch.Tensor) or logits.dim() != 2 or logits.dtype != torch.float32 or logits.stride(1) != 1:
        raise RuntimeError(f"mobilequant_amd: {who} logits must be fp32 [rows, V] with unit column stride")
    rows, V = logits.shape
    if not 1 <= rows <= MAX_ROWS:
        raise RuntimeError(f"mobilequant_amd: {who} rows={rows} outside 1..{MAX_ROWS}")
    return logits, rows, V


def _check_n_offset(who: str, n_offset) -> int:
    if isinstance(n_offset, bool) or not isinstance(n_offset, (int, np.integer)) or not -2 ** 30 <= int(n_offset) <= 2 ** 30:
        raise ValueError(f"mobilequant_amd: {who} n_offset={n_offset!r} must be an int in [-2^30, 2^30]")
    return int(n_offset)


def _check_vectors(who: str, *specs):
    """specs: (tensor or None, dtype, count, name, required) -- contiguous vectors of exactly `count` entries."""
    for t, dt, n, what, required in specs:
        if t is None:
            if required:
                raise RuntimeError(f"mobilequant_amd: {who} needs {what} ({dt} [{n}])")
        elif not isinstance(t, torch.Tensor) or t.dtype != dt or t.numel() != n or not t.is_contiguous():
            raise RuntimeError(f"mobilequant_amd: {who} {what} must be contiguous {dt} [{n}]")


def _packed(who: str, what: str, src, pack, dtype: np.dtype, count: Optional[int], noun: str = "", unit: str = "rows"):
    """`count` packed rows of `dtype` (count None: as many as src holds): src itself when it is a uint8 tensor of that size (the caller's
    device array), else the host array pack(src).  -> (tensor or array, number of rows)"""
    if not isinstance(src, torch.Tensor):
        host = pack(src)
        if count is not None and len(host) != count:
            raise RuntimeError(f"mobilequant_amd: {who} got {len(host)} {noun} for {count} {unit}")
        return host, len(host)
    if count is None:
        if src.dtype != torch.uint8 or src.numel() % dtype.itemsize or not src.is_contiguous():
            raise RuntimeError(f"mobilequant_amd: {who} {what} must be contiguous uint8 bytes, {dtype.itemsize} per sequence")
        return src, src.numel() // dtype.itemsize
    if src.dtype != torch.uint8 or src.numel() != count * dtype.itemsize or not src.is_contiguous():
        raise RuntimeError(f"mobilequant_amd: {who} {what} must be {count * dtype.itemsize} contiguous uint8 bytes")
    return src, count


def _check_history_block(who: str, history, count: int, V: int, aligned_rows: bool = False) -> int:
    """history [count, >= V] -> the row stride the C entry takes"""
    if not isinstance(history, torch.Tensor) or history.dtype not in HISTORY_DTYPES or history.dim() != 2 or history.shape[0] != count \
            or history.shape[1] < V or history.stride(1) != 1 or (aligned_rows and history.stride(0) % 4):
        raise RuntimeError(f"mobilequant_amd: {who} history must be int32 (uint32 bits) [{count}, >= {V}] with unit column stride")
    return history.stride(0) if count > 1 else max(V, history.stride(0))


def _check_bias_rows(who: str, bias, count: int, V: int, unit: str) -> list:
    brows = list(bias)
    if len(brows) != count:
        raise RuntimeError(f"mobilequant_amd: {who} got {len(brows)} bias rows for {count} {unit}")
    if not all(b is None or _is_row(b, (torch.float32,), V) for b in brows):
        raise RuntimeError(f"mobilequant_amd: a {who} bias row must be a contiguous fp32 [{V}] tensor")
    return brows


def _place(who: str, dev, **tensors) -> list:
    """The device checks, behind all others: a tensor of the caller's must be a ROCm device tensor; a host array of _packed goes to dev."""
    from .ops import _dev
    return [None if t is None else torch.from_numpy(t.view(np.uint8).reshape(-1)).to(dev) if isinstance(t, np.ndarray) else _dev(t, f"{who} {what}")
            for what, t in tensors.items()]


def _bias_table(who: str, dev, brows) -> Optional[torch.Tensor]:
    """[count] int64 on dev: each row's bias pointer, or NULL"""
    from .ops import _dev
    if brows is None:
        return None
    return torch.tensor([0 if b is None else _dev(b, who + " bias").data_ptr() for b in brows], dtype=torch.int64).to(dev)


def _ptr(t: Optional[torch.Tensor]):
    return t.data_ptr() if t is not None else None


def sample(logits: torch.Tensor, pos: torch.Tensor, params_rows, tok: torch.Tensor, *, cache_len: int = 2 ** 31 - 1,
           kept: Optional[torch.Tensor] = None, logprob: Optional[torch.Tensor] = None, penalties=None,
           history: Optional[torch.Tensor] = None, bias=None, observe: bool = False) -> torch.Tensor:
    """mq_sample: logits [rows, V] fp32 (row stride >= V), pos [rows] int32, tok [rows] int64 (written in place, returned).
    params_rows: a uint8 device tensor holding the mq_sample_row array, or (list of SamplingParams, list of streams).  A row whose
    pos is outside [0, cache_len) keeps its token.  kept [rows] int32 / logprob [rows] fp32: optional outputs.
    With any of penalties / history / bias / observe the call is mq_sample_penalized (step 0 of the rule in front): history [rows, >= V]
    int32 (the uint32 entries: bit 31 = in the prompt, bits 0..15 = times generated) is required; penalties: a uint8 device tensor
    holding the mq_sample_penalty_row array, or per row a SamplingParams or (repetition, presence, frequency) (default: the
    SamplingParams of params_rows, else neutral); bias: None, or per row None or a dense fp32 [V] device tensor; observe: count each
    drawn token in its row's history.  The logits are not written.
    Like sample_rows and sample_ragged, every shape, dtype and value is checked before any tensor's device: a call that is wrong in both
    ways (fp64 logits on the CPU, say) reports the former."""
    from .ops import _dev, _on, _stream
    who = "sample"
    logits, rows, V = _check_logits(who, logits)
    pr, _ = _packed(who, "params_rows", params_rows, lambda p: pack_rows(*p), ROW_DTYPE, rows, "requests")
    _check_vectors(who, (pos, torch.int32, rows, "pos", True), (tok, torch.int64, rows, "tok", True), (kept, torch.int32, rows, "kept", False),
                   (logprob, torch.float32, rows, "logprob", False))
    penalized = penalties is not None or history is not None or bias is not None or bool(observe)
    if penalized:
        if history is None:
            raise RuntimeError("mobilequant_amd: sample with penalties=, bias= or observe= needs history=")
        if isinstance(history, torch.Tensor) and history.dim() == 1:
            history = history.view(1, -1)
        hstride = _check_history_block(who, history, rows, V)
        if penalties is None:
            penalties = params_rows[0] if not isinstance(params_rows, torch.Tensor) else [(1.0, 0.0, 0.0)] * rows
        pen, _ = _packed(who, "penalties", penalties, lambda p: pack_penalty_rows(list(p)), PENALTY_DTYPE, rows, "penalty rows")
        brows = None if bias is None else _check_bias_rows(who, bias, rows, V, "rows")
    dev = _dev(logits, who + " logits").device
    pr, pos, tok, kept, logprob = _place(who, dev, params_rows=pr, pos=pos, tok=tok, kept=kept, logprob=logprob)
    scratch = torch.empty(MQ_SAMPLE_SCRATCH_BYTES, dtype=torch.uint8, device=dev)
    a = _fill_shared(MqSampleArgs(), logits, rows, pr, tok, scratch, kept, logprob)
    a.pos, a.cache_len = pos.data_ptr(), int(cache_len)
    if not penalized:
        with _on(logits, pos, pr, tok):
            _lib.call("mq_sample", ctypes.byref(a), _stream())
        return tok
    history, pen = _place(who, dev, history=history, penalties=pen)
    bias_ptr = _bias_table(who, dev, brows)
    p = MqSamplePenalizedArgs()
    p.s = a
    p.penalty, p.history, p.history_stride, p.bias, p.observe = pen.data_ptr(), history.data_ptr(), hstride, _ptr(bias_ptr), int(bool(observe))
    with _on(logits, pos, pr, tok):
        _lib.call("mq_sample_penalized", ctypes.byref(p), _stream())
    return tok


def sample_rows(logits: torch.Tensor, n_base: torch.Tensor, n_offset: int, params: SamplingParams, stream: int, tok: torch.Tensor, *,
                proposals: Optional[torch.Tensor] = None, history: Optional[torch.Tensor] = None, penalties=None,
                bias: Optional[torch.Tensor] = None, kept: Optional[torch.Tensor] = None, logprob: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mq_sample_rows: logits [rows, V] fp32 (row stride >= V), the rows of ONE sequence, under the single request
    (params, stream).  Row j is drawn at n_base[0] + n_offset + j (n_base: an int32 device tensor of one entry) into tok [rows] int64
    (written in place, returned); kept [rows] int32 / logprob [rows] fp32: optional outputs.  proposals: int64 device tensor of the
    rows - 1 ids in front of rows 1 .. rows - 1 (required when rows > 1).  history: None or one int32 (uint32 bits) row [>= V] shared by
    the rows; penalties: None (params' own), a SamplingParams or (repetition, presence, frequency); bias: None or a dense fp32 [>= V]
    device row.  Row j sees the history with proposals[:j] counted; nothing but the outputs is written."""
    from .ops import _dev, _on, _stream
    who = "sample_rows"
    logits, rows, V = _check_logits(who, logits)
    if not isinstance(params, SamplingParams):
        raise TypeError(f"mobilequant_amd: sample_rows expected SamplingParams, got {type(params).__name__}")
    n_offset = _check_n_offset(who, n_offset)
    pr = pack_rows([params], [stream])
    _check_vectors(who, (n_base, torch.int32, 1, "n_base", True), (tok, torch.int64, rows, "tok", True), (kept, torch.int32, rows, "kept", False),
                   (logprob, torch.float32, rows, "logprob", False), (proposals, torch.int64, rows - 1, "proposals", rows > 1))
    if history is not None and not _is_row(history, HISTORY_DTYPES, V):
        raise RuntimeError(f"mobilequant_amd: sample_rows history must be one contiguous int32 (uint32 bits) row [>= {V}]")
    if bias is not None and not _is_row(bias, (torch.float32,), V):
        raise RuntimeError(f"mobilequant_amd: sample_rows bias must be a contiguous fp32 [>= {V}] tensor")
    pen = pack_penalty_rows([params if penalties is None else penalties])
    dev = _dev(logits, who + " logits").device
    pr, n_base, tok, kept, logprob, proposals, history, bias, pen = _place(
        who, dev, params=pr, n_base=n_base, tok=tok, kept=kept, logprob=logprob, proposals=proposals, history=history, bias=bias, penalties=pen)
    scratch = torch.empty(MQ_SAMPLE_SCRATCH_BYTES, dtype=torch.uint8, device=dev)
    a = _fill_shared(MqSampleRowsArgs(), logits, rows, pr, tok, scratch, kept, logprob)
    a.n_base, a.n_offset, a.penalty, a.bias, a.history = n_base.data_ptr(), n_offset, pen.data_ptr(), _ptr(bias), _ptr(history)
    a.proposals = _ptr(proposals) if rows > 1 else None
    with _on(logits, n_base, pr, tok):
        _lib.call("mq_sample_rows", ctypes.byref(a), _stream())
    return tok


def sample_ragged(logits: torch.Tensor, row_seq: torch.Tensor, row_pos: torch.Tensor, row_tok: torch.Tensor, n_offset: int, params_rows,
                  tok: torch.Tensor, *, cache_len: int = 2 ** 31 - 1, penalties=None, history: Optional[torch.Tensor] = None, bias=None,
                  kept: Optional[torch.Tensor] = None, logprob: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mq_sample_ragged: logits [rows, V] fp32 (row stride >= V), the rows of a ragged step over `batch` sequences.
    row_seq / row_pos: int32 device tensors [rows], the table of mq_decode_attention_ragged; row_tok: int64 device tensor [rows], the
    tokens the rows were stepped with.  params_rows: a uint8 device tensor holding the mq_sample_row array of the batch, or (list of
    SamplingParams, list of streams), one per sequence: its length is the batch.  A live row of sequence s at position p is drawn at
    p + n_offset into tok [rows] int64 (written in place, returned) under request s, with the proposals of its run in front of it
    counted into the history as it reads; a row whose sequence is outside [0, batch) or whose position is outside [0, cache_len) keeps
    its tok / kept / logprob.  penalties: None (the SamplingParams of params_rows; a packed params_rows: neutral), a uint8 device tensor
    holding the mq_sample_penalty_row array, or per sequence a SamplingParams or (repetition, presence, frequency); history: None (all
    zeros) or int32 (uint32 bits) [batch, >= V]; bias: None, or per sequence None or a dense fp32 [V] device tensor.  Nothing but the
    outputs is written."""
    from .ops import _dev, _on, _stream
    who = "sample_ragged"
    logits, rows, V = _check_logits(who, logits)
    n_offset = _check_n_offset(who, n_offset)
    pr, batch = _packed(who, "params_rows", params_rows, lambda p: pack_rows(*p), ROW_DTYPE, None)
    if not 1 <= batch <= MAX_ROWS:
        raise RuntimeError(f"mobilequant_amd: sample_ragged batch={batch} outside 1..{MAX_ROWS}")
    _check_vectors(who, (row_seq, torch.int32, rows, "row_seq", True), (row_pos, torch.int32, rows, "row_pos", True),
                   (row_tok, torch.int64, rows, "row_tok", True), (tok, torch.int64, rows, "tok", True), (kept, torch.int32, rows, "kept", False),
                   (logprob, torch.float32, rows, "logprob", False))
    hstride = V if history is None else _check_history_block(who, history, batch, V, aligned_rows=True)
    if penalties is None and not isinstance(params_rows, torch.Tensor):
        penalties = params_rows[0]
    pen = None
    if penalties is not None:
        pen, _ = _packed(who, "penalties", penalties, lambda p: pack_penalty_rows(list(p)), PENALTY_DTYPE, batch, "penalty rows", "sequences")
    brows = None if bias is None else _check_bias_rows(who, bias, batch, V, "sequences")
    dev = _dev(logits, who + " logits").device
    pr, row_seq, row_pos, row_tok, tok, kept, logprob, history, pen = _place(
        who, dev, params_rows=pr, row_seq=row_seq, row_pos=row_pos, row_tok=row_tok, tok=tok, kept=kept, logprob=logprob, history=history, penalties=pen)
    bias_ptr = _bias_table(who, dev, brows)
    scratch = torch.empty(MQ_SAMPLE_SCRATCH_BYTES, dtype=torch.uint8, device=dev)
    a = _fill_shared(MqSampleRaggedArgs(), logits, rows, pr, tok, scratch, kept, logprob)
    a.batch, a.cache_len, a.n_offset = batch, int(cache_len), n_offset
    a.row_seq, a.row_pos, a.row_tok = row_seq.data_ptr(), row_pos.data_ptr(), row_tok.data_ptr()
    a.penalty, a.history, a.history_stride, a.bias = _ptr(pen), _ptr(history), hstride, _ptr(bias_ptr)
    with _on(logits, row_seq, pr, tok):
        _lib.call("mq_sample_ragged", ctypes.byref(a), _stream())
    return tok


def history_count_ragged(history: torch.Tensor, pairs: torch.Tensor, delta: int):
    """mq_sample_history_count_ragged on a block of histories ([batch, >= V] int32 device tensor holding the uint32 entries; V is its
    column count): pairs is an int64 device tensor [n, 2] of (sequence, id); the count (bits 0..15) of each pair's id in its sequence's
    history moves by delta = +1 or -1, saturating at 65 535 and at 0.  Bit 31 is kept; a pair whose sequence is outside [0, batch) or
    whose id is outside [0, V) is ignored on the device; pairs repeat.  One launch for all sequences (none for n = 0), capturable."""
    h = history
    ok = isinstance(h, torch.Tensor) and h.dtype in HISTORY_DTYPES and h.dim() == 2 and 1 <= h.shape[0] <= MAX_ROWS and h.stride(1) == 1 \
        and h.stride(0) >= h.shape[1] and h.stride(0) % 4 == 0
    _check_count("history_count_ragged", delta, h, ok, f"int32 (uint32 bits) [1..{MAX_ROWS}, V] with unit column stride",
                 pairs, "pairs", _is_ids(pairs, 2) and pairs.shape[1] == 2, "int64 [n, 2] tensor of (sequence, id)")
    n = pairs.shape[0]
    with torch.cuda.device(h.device):
        _lib.call("mq_sample_history_count_ragged", h.data_ptr(), h.stride(0), h.shape[1], h.shape[0], pairs.data_ptr() if n else None, n, int(delta),
                  torch.cuda.current_stream(h.device).cuda_stream)
    return history


def logprob_top(logits: torch.Tensor, tok: torch.Tensor, n_top: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """mq_logprob_top: logits [rows, V] fp32 (row stride >= V; the RAW rows), tok [rows] int64 device tensor of chosen
    ids, n_top in 0 .. 20.  Returns device tensors (logprob [rows] fp32, rank [rows] int32, top_id [rows, n_top] int32, top_logprob
    [rows, n_top] fp32) by the rule in csrc/mq_logprob.hip's header: a row's outputs depend on that row, its token, n_top and V only.
    A token outside [0, V) gives logprob NaN and rank 0."""
    from .ops import _dev, _on, _stream
    _dev(logits, "logprob_top logits")
    if logits.dim() == 1:
        logits = logits.view(1, -1)
    if logits.dim() != 2 or logits.dtype != torch.float32 or logits.stride(1) != 1:
        raise RuntimeError("mobilequant_amd: logprob_top logits must be fp32 [rows, V] with unit column stride")
    rows, V = logits.shape
    if not 1 <= rows <= MAX_ROWS:
        raise RuntimeError(f"mobilequant_amd: logprob_top rows={rows} outside 1..{MAX_ROWS}")
    if isinstance(n_top, bool) or not isinstance(n_top, (int, np.integer)) or not 0 <= int(n_top) <= MQ_LOGPROB_MAX_TOP:
        raise ValueError(f"mobilequant_amd: logprob_top n_top={n_top!r} must be an int in 0..{MQ_LOGPROB_MAX_TOP}")
    _dev(tok, "logprob_top tok")
    if tok.dtype != torch.int64 or tok.numel() != rows or not tok.is_contiguous():
        raise RuntimeError(f"mobilequant_amd: logprob_top tok must be contiguous int64 [{rows}]")
    n, dev = int(n_top), logits.device
    logprob = torch.empty(rows, dtype=torch.float32, device=dev)
    rank = torch.empty(rows, dtype=torch.int32, device=dev)
    top_id = torch.empty(rows, n, dtype=torch.int32, device=dev)
    top_logprob = torch.empty(rows, n, dtype=torch.float32, device=dev)
    scratch = torch.empty(MQ_LOGPROB_SCRATCH_BYTES, dtype=torch.uint8, device=dev)
    a = MqLogprobTopArgs()
    a.logits, a.logits_stride, a.V, a.rows, a.n_top = logits.data_ptr(), logits.stride(0) if rows > 1 else max(V, logits.stride(0)), V, rows, n
    a.tok, a.batch, a.cache_len, a.record_len = tok.data_ptr(), rows, 1, 1
    a.logprob, a.rank = logprob.data_ptr(), rank.data_ptr()
    if n:
        a.top_id, a.top_logprob = top_id.data_ptr(), top_logprob.data_ptr()
    a.scratch, a.scratch_bytes = scratch.data_ptr(), MQ_LOGPROB_SCRATCH_BYTES
    with _on(logits, tok):
        _lib.call("mq_logprob_top", ctypes.byref(a), _stream())
    return logprob, rank, top_id, top_logprob


def sample_uniforms(seed: int, stream: int, n: int, first: int, count: int, device) -> torch.Tensor:
    """The rule's uniforms u_i, i = first .. first + count - 1, at (seed, stream, n): the generator alone (tests)."""
    out = torch.empty(count, dtype=torch.float32, device=device)
    with torch.cuda.device(out.device):
        _lib.call("mq_sample_uniforms", int(seed), int(stream), int(n) & 0xFFFFFFFF, int(first), int(count), out.data_ptr(),
                  torch.cuda.current_stream().cuda_stream)
    return out
