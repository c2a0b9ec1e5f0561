"""Seeded device-side token selection (csrc/mq_sample.hip): SamplingParams, the packed per-row request array the
kernel reads, and the launch record both decode engines keep for their logits / position / token buffers."""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import MQ_SAMPLE_SCRATCH_BYTES, MqSampleArgs

MAX_ROWS = 8
MAX_VOCAB = 1 << 20
ROW_DTYPE = np.dtype([("temperature", "<f4"), ("top_k", "<i4"), ("top_p", "<f4"), ("min_p", "<f4"), ("seed", "<u8"), ("stream", "<u8")])
assert ROW_DTYPE.itemsize == ctypes.sizeof(_lib.MqSampleRow) == 32


@dataclass(frozen=True)
class SamplingParams:
    """temperature >= 0 (0 = greedy), top_k >= 0 (0 = off), top_p in (0, 1] (1 = off), min_p in [0, 1) (0 = off), seed in [0, 2^64).
    Filters compose in the usual order: temperature, top-k, top-p, min-p.  With a seed, a stream (the sequence's identity) and the
    position, the drawn token is a property of the sequence: the same in any batch, in any slot, captured or not."""
    temperature: float = 1.0
    top_k: int = 0
    top_p: float = 1.0
    min_p: float = 0.0
    seed: int = 0

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


class SampleLaunch:
    """mq_sample over an engine's own buffers: logits [rows, V] -> tok [rows] at the positions in pos [rows].  The per-row requests
    live in a device array that set_rows() rewrites in place, so a captured launch serves any request."""

    def __init__(self, logits: torch.Tensor, pos: torch.Tensor, tok: torch.Tensor, cache_len: int):
        lg = logits.view(-1, logits.shape[-1])
        rows, V = lg.shape
        dev = logits.device
        self.rows, self.dev = rows, dev
        self.params = torch.zeros(rows * ROW_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.scratch = torch.zeros(MQ_SAMPLE_SCRATCH_BYTES, dtype=torch.uint8, device=dev)
        a = MqSampleArgs()
        a.logits, a.logits_stride, a.V, a.rows = lg.data_ptr(), lg.stride(0), V, rows
        a.pos, a.cache_len, a.params, a.tok = pos.data_ptr(), int(cache_len), self.params.data_ptr(), tok.data_ptr()
        a.kept, a.logprob = None, None
        a.scratch, a.scratch_bytes = self.scratch.data_ptr(), MQ_SAMPLE_SCRATCH_BYTES
        self.args = a
        self._keep = (lg, pos, tok)
        self.set_rows([SamplingParams(temperature=0.0)] * rows, list(range(rows)))

    def set_rows(self, params: Sequence[SamplingParams], streams: Sequence[int]):
        host = pack_rows(params, streams)
        if len(host) != self.rows:
            raise ValueError(f"sampling: {len(host)} requests for {self.rows} rows")
        self.params.copy_(torch.from_numpy(host.view(np.uint8).reshape(-1)))

    def launch(self):
        """On the current stream (capturable: two kernel launches, nothing else)."""
        _lib.call("mq_sample", ctypes.byref(self.args), torch.cuda.current_stream(self.dev).cuda_stream)


def validate_generate_args(who: str, sampling, do_sample: bool, draft=None):
    if do_sample:
        raise ValueError(f"{who}: sampling= and do_sample=True are two different selection rules; pass one of them")
    if draft is not None:
        raise ValueError(f"{who}: a draft is for greedy decoding only (sampling= with a draft)")


def sample(logits: torch.Tensor, pos: torch.Tensor, params_rows, tok: torch.Tensor, *, cache_len: int = 2 ** 31 - 1,
           kept: Optional[torch.Tensor] = None, logprob: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mq_sample: logits [rows, V] fp32 (row stride >= V), pos [rows] int32, tok [rows] int64 (written in place, returned).
    params_rows: a uint8 device tensor holding the mq_sample_row array, or (list of SamplingParams, list of streams).  A row whose
    pos is outside [0, cache_len) keeps its token.  kept [rows] int32 / logprob [rows] fp32: optional outputs."""
    from .ops import _dev, _on, _stream
    _dev(logits, "sample logits")
    if logits.dim() == 1:
        logits = logits.view(1, -1)
    if logits.dim() != 2 or logits.dtype != torch.float32 or logits.stride(1) != 1:
        raise RuntimeError("mobilequant_amd: sample logits must be fp32 [rows, V] with unit column stride")
    rows, V = logits.shape
    if not 1 <= rows <= MAX_ROWS:
        raise RuntimeError(f"mobilequant_amd: sample rows={rows} outside 1..{MAX_ROWS}")
    if isinstance(params_rows, torch.Tensor):
        pr = _dev(params_rows, "sample params_rows")
        if pr.dtype != torch.uint8 or pr.numel() != rows * ROW_DTYPE.itemsize or not pr.is_contiguous():
            raise RuntimeError(f"mobilequant_amd: sample params_rows must be {rows * ROW_DTYPE.itemsize} contiguous uint8 bytes")
    else:
        host = pack_rows(*params_rows)
        if len(host) != rows:
            raise RuntimeError(f"mobilequant_amd: sample got {len(host)} requests for {rows} rows")
        pr = torch.from_numpy(host.view(np.uint8).reshape(-1)).to(logits.device)
    for t, dt, what in ((pos, torch.int32, "pos"), (tok, torch.int64, "tok"), (kept, torch.int32, "kept"), (logprob, torch.float32, "logprob")):
        if t is None:
            continue
        _dev(t, "sample " + what)
        if t.dtype != dt or t.numel() != rows or not t.is_contiguous():
            raise RuntimeError(f"mobilequant_amd: sample {what} must be contiguous {dt} [{rows}]")
    a = MqSampleArgs()
    scratch = torch.empty(MQ_SAMPLE_SCRATCH_BYTES, dtype=torch.uint8, device=logits.device)
    a.logits, a.logits_stride, a.V, a.rows = logits.data_ptr(), logits.stride(0) if rows > 1 else max(V, logits.stride(0)), V, rows
    a.pos, a.cache_len, a.params, a.tok = pos.data_ptr(), int(cache_len), pr.data_ptr(), tok.data_ptr()
    a.kept = kept.data_ptr() if kept is not None else None
    a.logprob = logprob.data_ptr() if logprob is not None else None
    a.scratch, a.scratch_bytes = scratch.data_ptr(), MQ_SAMPLE_SCRATCH_BYTES
    with _on(logits, pos, pr, tok):
        _lib.call("mq_sample", ctypes.byref(a), _stream())
    return tok


def sample_uniforms(seed: int, stream: int, n: int, first: int, count: int, device) -> torch.Tensor:
    """The rule's uniforms u_i, i = first .. first + count - 1, at (seed, stream, n): the generator alone (tests)."""
    out = torch.empty(count, dtype=torch.float32, device=device)
    with torch.cuda.device(out.device):
        _lib.call("mq_sample_uniforms", int(seed), int(stream), int(n) & 0xFFFFFFFF, int(first), int(count), out.data_ptr(),
                  torch.cuda.current_stream().cuda_stream)
    return out
