"""Batched decode: up to eight independent sequences ("slots") advanced by one step together, each with its own position and its own
int8 KV cache (csrc/mq_decode_batch.hip).

``DecodeEngine`` streams the whole model for one token per step.  ``BatchDecodeEngine`` lowers every decoder layer to the same five
launches (norm + q|k|v, attention, o_proj + residual, norm + w1|w3 + gate, w2 + residual) but each launch serves B activation rows:
the weights are read once per step for all slots.  The contract is per sequence: slot b of a batched step computes exactly -- bit for
bit -- what ``DecodeEngine`` computes for that sequence alone.  A phase whose linears carry per-group weight grids
(QuantConfig group_size) runs ``mq_decode_gemv_grouped``, the launch the single engine runs for it at B = 1.
The layer is lowered by the code the single engine uses (``decode._DecodeBase._lower_chain``); this engine only says where the B rows live.

Positions live in device memory (``pos [B]``), so ONE captured hipGraph serves every mix of slot positions: the attention launch
chooses each sequence's split count on the device, and a slot whose position is the ``cache_len`` sentinel is idle -- its cache and
its logits row do not change.

Ragged steps: ``step_tokens`` / ``extend`` move chosen slots by several tokens in ONE step while the others stand
still, ``rewind`` drops a slot's last positions, and ``generate(draft=...)`` is greedy speculative decoding across the batch.  Their
rows run the same weight launches over row buffers of their own and ``mq_decode_attention_ragged`` (csrc/mq_decode_rows.hip), whose
row table -- like the tokens and the position advance -- is device data: one hipGraph per total row count serves every plan.

Speculation under seeded sampling: ``sample_rows`` / ``step_sample_tokens`` draw every row of a ragged step at its own
index under its own slot's request (``mq_sample_ragged``, csrc/mq_sample.hip, over the step's row table) and ``generate_speculative``
returns, token for token, the ids of ``generate(sampling=...)``.

Forks: ``fork({src: [dst, ...]})`` makes one slot's cached sequence the start of others -- ONE ``mq_decode_cache_fork``
launch (csrc/mq_decode_fork.hip) copies the live cache bytes of all sources, in all layers, to all destinations -- and
``generate(..., n=k)`` / ``generate_speculative(..., n=k)`` draw k samples of every prompt from ONE prefill of it.

Beam search: ``generate_beam(prompts, max_new_tokens, num_beams)`` keeps W beams of every prompt in W neighbouring
slots.  Per step ONE ``mq_beam_select`` (csrc/mq_beam.hip) picks every prompt's best K continuations from the logits rows on the
device, the host reads n_groups x K records and runs the hypothesis bookkeeping, and ONE ``mq_decode_cache_reorder``
(csrc/mq_decode_reorder.hip) makes "slot d continues old slot parent[d]" true for all slots at once, in place, before the ordinary
``step()``.  A prompt's result is a function of the prompt and the arguments only.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Mapping, NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _lib, ops
from .decode import DecodeEngine, _check_draft, _DecodeBase, _eos_set, _spec_stats, _Target, plan_rows, spec_row_budget
from .sampling import (RaggedRowsLaunch, SampleLaunch, SamplingParams, TokenLogprobs, check_logprobs, check_stream, history_count_ragged,
                       validate_generate_args)

MAX_BATCH = 8


class BeamResult(NamedTuple):
    """generate_beam's return for one prompt, best hypothesis first."""
    sequences: List[List[int]]           # context + new tokens, an ending EOS included
    scores: List[float]                  # sum_logprob / L ** length_penalty, L the hypothesis' new tokens
    sum_logprobs: List[float]            # the fp32 sums of the tokens' log-probabilities


class _BeamHyps:
    """A prompt's finished hypotheses: the best W by score; adding drops the worst, and on equal scores the earlier entry stays."""

    def __init__(self, width: int):
        self.width, self.items, self.added = width, [], 0

    def add(self, ids: List[int], sum_logprob: float, score: float):
        self.items.append((score, self.added, ids, sum_logprob))
        self.added += 1
        self.items.sort(key=lambda e: (-e[0], e[1]))               # score descending, earlier-added first
        del self.items[self.width:]

    def full(self) -> bool:
        return len(self.items) >= self.width

    def worst(self) -> float:
        return self.items[-1][0]


def _count(n: int, fan: int) -> str:
    """How an error message names n slots: as prompts, or under generate(n=fan) as the samples of n / fan prompts."""
    return f"{n} prompts" if fan == 1 else f"{n} samples ({n // fan} prompts x n={fan}, one per slot)"


def _nest(res, k: int, with_records: bool):
    """generate(n=k)'s return: the flat per-slot lists as out[i][j] = slot i * k + j (and the records the same way)."""
    def fold(flat):
        return [list(flat[i:i + k]) for i in range(0, len(flat), k)]
    return (fold(res[0]), fold(res[1])) if with_records else fold(res)


class _BatchGreedy:
    """How BatchDecodeEngine._generate_speculative chooses tokens: plain generate's torch.argmax per row (ties break as they do there)."""

    def first(self, eng) -> List[int]:
        """The token behind every slot's cached sequence, from eng.logits (an idle slot's entry means nothing)."""
        return torch.argmax(eng.logits, dim=-1).tolist()

    def plain(self, eng, tokens: Sequence[int]) -> List[int]:
        """ONE step() of every active slot on `tokens` and the token behind each."""
        eng.step(tokens)
        return self.first(eng)

    def rows(self, eng, tokens: Mapping[int, Sequence[int]]) -> List[int]:
        """ONE ragged step of eng over `tokens`: the token behind every row, in row order (one read-back for all slots)."""
        eng.step_tokens(tokens)
        return torch.argmax(eng.rlogits[:sum(len(t) for t in tokens.values())], dim=-1).tolist()

    def count(self, eng, kept):
        pass


class _BatchSampled:
    """_BatchGreedy's counterpart for generate(sampling=..., streams=...): every slot under its own request and stream -- sample() and,
    behind a ragged step, mq_sample_ragged (one graph with the step after capture(), ONE read-back of the R tokens).  Under a penalised
    request start() rebuilds the slots' histories from the prompts; sample() counts what it draws itself (first, plain), mq_sample_ragged
    counts nothing: count() adds the kept tokens of a round, (slot, token) pairs, with one staging copy and one launch for all slots."""

    def __init__(self, rows, streams):
        self.requests, self.streams = list(rows), list(streams)

    def start(self, eng, prompts):
        idle = eng.batch - len(self.requests)
        eng.set_sampling(self.requests + [SamplingParams(temperature=0.0)] * idle, self.streams + [0] * idle)
        if eng._sampler.penalized:
            for i, p in enumerate(prompts):
                eng._sampler.observe_prompt(i, p)                  # slot i's history: cleared, then its prompt

    def first(self, eng) -> List[int]:
        eng.sample()
        return eng.tok.tolist()

    def plain(self, eng, tokens: Sequence[int]) -> List[int]:
        eng.step(tokens)
        return self.first(eng)

    def rows(self, eng, tokens: Mapping[int, Sequence[int]]) -> List[int]:
        return eng.step_sample_tokens(tokens).tolist()

    def count(self, eng, kept):
        if kept and eng._sampler.penalized:
            history_count_ragged(eng._sampler.history, torch.tensor(kept, dtype=torch.int64).to(eng.dev), 1)


class BatchDecodeEngine(_DecodeBase):
    """B single-token decode streams over one model.  Slots are filled with prefill(slot, ids), emptied with release(slot) and all
    active slots advance together with step()."""

    # LONG_FROM / LONG_SPLITS (the base's) apply per sequence, on the device; MAX_IMAGE_BYTES / MAX_HEAD_FLOATS bound B * K and B * hidden

    MAX_ROWS = MAX_BATCH                 # step_tokens: rows per ragged step (MQ_DECODE_MAX_BATCH), lowered by the shape (max_rows)

    def __init__(self, model, batch: int, cache_len: int = 2048, max_rows: int = 8):
        """max_rows: the rows of a ragged step (step_tokens), lowered as DecodeEngine.max_rows is: R * K int8 images in the GEMV launches'
        LDS (128 KiB), R * hidden normalised floats in the head's (32 768)."""
        from .llama import LlamaForCausalLM
        assert isinstance(model, LlamaForCausalLM)
        B = int(batch)
        if not 1 <= B <= MAX_BATCH:
            raise ValueError(f"BatchDecodeEngine: batch={batch} outside 1..{MAX_BATCH}")
        self.model, self.shape, self.batch = model, model.shape, B
        s = self.shape
        dev = next(model.parameters()).device
        self.dev, self.cache_len = dev, int(cache_len)
        if not 0 < self.cache_len <= DecodeEngine.max_cache_len(5, s.head_dim):
            raise RuntimeError(f"BatchDecodeEngine: cache_len={cache_len} is outside 1 .. {DecodeEngine.max_cache_len(5, s.head_dim)}")
        big = max(s.hidden, s.ffn, s.heads * s.head_dim)
        if B * big > self.MAX_IMAGE_BYTES or B * s.hidden > self.MAX_HEAD_FLOATS:
            raise RuntimeError(f"BatchDecodeEngine: batch {B} x K {big} exceeds the {self.MAX_IMAGE_BYTES} bytes of activation images a launch holds")
        self.cos, self.sin = model.cos.contiguous(), model.sin.contiguous()
        assert self.cos.shape[0] >= self.cache_len, "rope tables shorter than the cache"
        qkv_n = (s.heads + 2 * s.kv_heads) * s.head_dim
        self.x = torch.zeros(B, s.hidden, device=dev)
        self.qkv = torch.zeros(B, qkv_n, device=dev)
        self.attn_q = torch.zeros(B, s.heads * s.head_dim, dtype=torch.int8, device=dev)
        self.attn_part = torch.zeros(B, self.LONG_SPLITS, s.heads * s.head_dim, dtype=torch.int64, device=dev)
        self.attn_ticket = torch.zeros(B, s.heads, dtype=torch.int32, device=dev)
        self.gate_q = torch.zeros(B, s.ffn, dtype=torch.int8, device=dev)
        # (row B of the allocation, outside self.logits: where a ragged step's finish drops the rows that are no slot's last)
        self._logits_rows = torch.zeros(B + 1, s.vocab, device=dev)
        self.logits = self._logits_rows[:B]
        self.pos = torch.full((B,), self.cache_len, dtype=torch.int32, device=dev)       # every slot idle
        self.tok = torch.zeros(B, dtype=torch.int64, device=dev)
        # [B][kv_heads][cache_len][head_dim] int8 indices (index - 128) on qk_bmm.input2 / pv_bmm.input2's grids
        self.k_cache = [torch.zeros(B, s.kv_heads, self.cache_len, s.head_dim, dtype=torch.int8, device=dev) for _ in model.layers]
        self.v_cache = [torch.zeros(B, s.kv_heads, self.cache_len, s.head_dim, dtype=torch.int8, device=dev) for _ in model.layers]
        self._host_pos = [self.cache_len] * B
        self._active = [False] * B
        if isinstance(max_rows, bool) or int(max_rows) < 1:
            raise ValueError(f"BatchDecodeEngine: max_rows={max_rows} must be >= 1")
        self.max_rows = max(1, min(int(max_rows), self.MAX_ROWS, self.MAX_IMAGE_BYTES // big, self.MAX_HEAD_FLOATS // s.hidden))
        self.spec_stats = None               # what the last generate(draft=...) / generate_speculative did
        self._rows_at = None                 # (rows, positions behind it) of the last step_tokens call: what sample_rows may draw
        self.graph = None
        self.append_stats = None             # what the last prefill(slot, ids, append=True) did
        self._append_images = None           # per layer ImageCache of prefill(append=True), allocated on first use
        self._sampler = None                 # mq_sample over logits / pos / tok (sample(), generate(sampling=...))
        self._sample_graphs = {}             # penalised -> the captured sample + step graph, recorded on first use after capture()
        self._lp = None                      # mq_logprob_top behind every selection launch (set_logprobs), or None
        self._lp_launches = {}               # n_top -> its LogprobLaunch (record buffers [batch, cache_len]), allocated on first request
        self._fork_caches = self.k_cache + self.v_cache
        self._fork_table = ops.decode_cache_table(self._fork_caches)     # fork(): built once, the caches are never reallocated
        self._fork_parent = torch.arange(B, dtype=torch.int32, device=dev)
        self.fork_stats = None               # what the last fork() did
        self._beam = None                    # generate_beam's device buffers, allocated on first use
        self.beam_stats = None               # what the last generate_beam() did
        self._lower()

    def _lower(self):
        """Launch records from the model as it is now (_lower_model): per layer the five-launch chain over the B rows of the slot buffers,
        a sequence per row."""
        self._rows = None         # row phases of step_tokens: lowered on first use, from the layers' images (_lower_rows)
        self._row_graphs = {}     # total row count -> the captured ragged step, recorded on first use after capture()
        self._lower_model()
        t = _Target(self.x, self.qkv, self.attn_q, self.attn_part, self.attn_ticket, self.gate_q, self.k_cache, self.v_cache, nsplit=self.LONG_SPLITS,
                    rows=self.batch, attn="batch")
        with torch.no_grad():
            for li, layer in enumerate(self.model.layers):
                self.phases += self._lower_chain(li, self._layer_images(layer), t)
        self.head = self._head_batch(self.x, self.logits, self.batch, pos=self.pos)

    # -- running -------------------------------------------------------------------------------------------------------------
    _ENTRY = {"gemv": "mq_decode_gemv_batch", "gemv_grouped": "mq_decode_gemv_grouped", "attn": "mq_decode_attention_batch"}

    def _launch(self):
        """embedding gather + 5 launches per layer + norm / lm_head for all slots, on the current stream; reads self.tok / self.pos."""
        st = torch.cuda.current_stream(self.dev).cuda_stream
        torch.index_select(self.embed, 0, self.tok, out=self.x)
        for kind, a in self.phases:
            _lib.call(self._ENTRY[kind], ctypes.byref(a), st)
        _lib.call("mq_decode_head_batch", ctypes.byref(self.head), st)

    def _advance(self):
        self.pos.add_((self.pos < self.cache_len).to(torch.int32))         # active slots only (idle ones hold the sentinel)

    def capture(self):
        """Record one step for all slots (incl. the position advance) as ONE hipGraph on one stream; step() replays it.  Every mix of
        slot positions replays the same graph: the attention launch picks each sequence's split count from its position."""
        self._sync_grids()
        pos0 = self.pos.clone()
        self.pos.fill_(self.cache_len)            # the warm-up below runs with every slot idle: no cache or logits row changes
        self.attn_ticket.zero_()
        self.graph = self._record(self._launch, self._advance)
        self.pos.copy_(pos0)
        self._sample_graphs = {}
        self._row_graphs = {}                     # (ragged steps: one graph per total row count, recorded on first use)
        self._row_sample_graphs = {}              # (with the selection behind them: one per (total row count, penalised))
        return self

    # -- ragged steps: several tokens per slot (csrc/mq_decode_rows.hip) ----------------------------------------
    def _lower_rows(self):
        """The launch records of a ragged step (_lower_row_chain): mq_decode_attention_ragged over the engine's own caches.  The plan
        of a step -- tokens, row table, where each row's logits go, the slots' position advance -- is ONE packed int32 buffer (rplan),
        written by one host -> device copy; rtok / row_dst (int64) and row_seq / row_pos / radv (int32) are views of it."""
        R, B = self.max_rows, self.batch
        self.rplan = torch.zeros(6 * R + B, dtype=torch.int32, device=self.dev)
        self.rtok, self.row_dst = self.rplan[:2 * R].view(torch.int64), self.rplan[2 * R:4 * R].view(torch.int64)
        self.row_seq, self.row_pos, self.radv = self.rplan[4 * R:5 * R], self.rplan[5 * R:6 * R], self.rplan[6 * R:]
        self._upload_plan(None)
        self.rsel = torch.zeros(R, dtype=torch.int64, device=self.dev)                   # sample_rows: row r's drawn token
        self._row_sel, self._row_sample_graphs = None, {}
        self._lower_row_chain(head_pos=self.row_pos, attn="ragged", batch=B, row_seq=self.row_seq, row_pos=self.row_pos)

    def _upload_plan(self, plan):
        """A plan_rows plan (None: every row idle, no slot advances) into rplan: one host -> device copy.  An idle row names
        sequence -1 at the cache_len sentinel; a row that is not its slot's last sends its logits to the spare row behind self.logits."""
        R, B = self.max_rows, self.batch
        h = np.zeros(6 * R + B, dtype=np.int32)
        tok, dst = h[:2 * R].view(np.int64), h[2 * R:4 * R].view(np.int64)
        dst[:] = B
        h[4 * R:5 * R], h[5 * R:6 * R] = -1, self.cache_len
        if plan is not None:
            n = len(plan.row_tok)
            tok[:n], h[4 * R:4 * R + n], h[5 * R:5 * R + n] = plan.row_tok, plan.row_seq, plan.row_pos
            for slot, (r0, cnt) in plan.spans.items():
                dst[r0 + cnt - 1] = slot
                h[6 * R + slot] = cnt
        self.rplan.copy_(torch.from_numpy(h), non_blocking=False)

    def _finish_rows(self, R: int):
        """logits[slot] <- the slot's last row (the others, idle ones included, land in the spare row) and the slots' position advance:
        fixed-shape device ops over the plan, so any assignment of R rows to slots replays the same graph."""
        self._logits_rows.index_copy_(0, self.row_dst[:R], self.rlogits[:R])
        self.pos.add_(self.radv)

    def _capture_rows(self, R: int, plan, sel: Optional[RaggedRowsLaunch] = None):
        """Record the R-row ragged step (incl. the logits rows and the position advance) as a hipGraph; with sel, mq_sample_ragged over
        the rows behind it, in the same graph.  The warm-up launch outside the capture runs with every row idle: no cache byte, logits
        row or position changes (the selection's own warm-up draws nothing: an idle row keeps its token)."""
        self._set_rows(R)
        self._upload_plan(None)
        self.rticket.zero_()
        if sel is None:
            g = self._row_graphs[R] = self._record(lambda: self._launch_rows(R), lambda: self._finish_rows(R))
        else:
            with torch.cuda.device(self.dev):
                sel.launch(R)                                  # outside the capture: the select kernel's LDS ceiling

            def finish():
                self._finish_rows(R)
                sel.launch(R)
                if self._lp is not None:
                    self._lp.launch_ragged(sel, R)
            g = self._row_sample_graphs[self._lp_key(R, self._sampler.penalized)] = self._record(lambda: self._launch_rows(R), finish)
        self._upload_plan(plan)
        return g

    @torch.no_grad()
    def step_tokens(self, tokens: Mapping[int, Sequence[int]]) -> Dict[int, torch.Tensor]:
        """A ragged step: every named slot (active, at least one token) appends its tokens at its own position, all in ONE step of at
        most max_rows rows in total (rows in ascending slot order, a slot's rows contiguous).  Returns slot -> logits [T_slot, vocab],
        views of the row buffer that the next call overwrites: row j is, bit for bit, what DecodeEngine.step(tokens[j]) returns for
        that sequence alone after the earlier tokens, and the slot's caches end as those steps leave them.  Its position advances by
        T_slot and self.logits[slot] holds its last row: sample() and generate continue from there.  Slots NOT named do not move
        (unlike step(), which advances every active slot): their caches, positions and logits rows keep their bytes.
        ValueError: total rows outside 1..max_rows, an empty token list, a slot out of range; RuntimeError: an idle slot, tokens
        that would overflow the slot's cache.  After capture(): one hipGraph per TOTAL row count, recorded on first use; the row
        table, the tokens, the position advance and the logits[slot] update are device data and device ops inside it."""
        plan = self._step_rows(tokens, False, "step_tokens")
        return {slot: self.rlogits[r0:r0 + cnt] for slot, (r0, cnt) in plan.spans.items()}

    def _step_rows(self, tokens: Mapping[int, Sequence[int]], select: bool, who: str):
        """The ragged step of step_tokens (select: with mq_sample_ragged over its rows behind it, step_sample_tokens).  Returns the plan."""
        plan = plan_rows(tokens, [p if a else None for p, a in zip(self._host_pos, self._active)], self.max_rows, self.cache_len,
                         "BatchDecodeEngine." + who)
        R = len(plan.row_tok)
        if self._rows is None:
            self._lower_rows()
        sel = self._row_launch() if select else None
        if self.graph is not None:
            g = self._row_sample_graphs.get(self._lp_key(R, self._sampler.penalized)) if select else self._row_graphs.get(R)
            if g is None:
                g = self._capture_rows(R, plan, sel)
            else:
                self._upload_plan(plan)
            g.replay()
        else:
            self._upload_plan(plan)
            self._set_rows(R)
            with torch.cuda.device(self.dev):
                self._launch_rows(R)
                self._finish_rows(R)
                if select:
                    sel.launch(R)
                    if self._lp is not None:
                        self._lp.launch_ragged(sel, R)
        for slot, (_, cnt) in plan.spans.items():
            self._host_pos[slot] += cnt
        self._rows_at = (R, list(self._host_pos))
        return plan

    def _row_launch(self) -> RaggedRowsLaunch:
        if self._sampler is None:
            self.set_sampling(SamplingParams(temperature=0.0))
        if self._rows is None:
            self._lower_rows()
        if self._row_sel is None:
            self._row_sel = RaggedRowsLaunch(self._sampler, self.rlogits, self.row_seq, self.row_pos, self.rtok, self.rsel, self.cache_len, n_offset=1)
        return self._row_sel

    @torch.no_grad()
    def sample_rows(self, R: int) -> torch.Tensor:
        """mq_sample_ragged on the R rows of the last step_tokens call, each under its own slot's request of
        set_sampling (greedy until one is set): returns a device tensor [R] (overwritten by the next call; no host read), rows in the
        step's order (ascending slots, a slot's rows contiguous).  The row cached at position p predicts token index p + 1 -- the index
        sample() would draw at after a plain step -- so a slot's row j is the token plain sampling draws behind tokens[slot][:j + 1]:
        what DecodeEngine.sample_rows draws for that sequence alone.  Under a penalised request the row sees its slot's history plus
        tokens[slot][1:j + 1], the proposals in front of it (read from the step's own token buffer); no history is written: count what
        is kept with sampling.history_count_ragged.  R must be that call's total row count, with every position still behind it."""
        R = int(R)
        if self._rows_at != (R, self._host_pos):
            raise RuntimeError(f"BatchDecodeEngine.sample_rows: R={R} is not the row count of a step_tokens call that the slots' positions "
                               f"({self._host_pos}) still stand behind")
        with torch.cuda.device(self.dev):
            sel = self._row_launch()
            sel.launch(R)
            if self._lp is not None:
                self._lp.launch_ragged(sel, R)
        return self.rsel[:R]

    @torch.no_grad()
    def step_sample_tokens(self, tokens: Mapping[int, Sequence[int]]) -> torch.Tensor:
        """step_tokens(tokens) and sample_rows(total rows): returns the drawn tokens [R] (device), rows in ascending slot order.  After
        capture() the ragged step and the selection are ONE graph per (total rows, penalised), recorded on first use with every row
        idle; any assignment of rows to slots and any requests replay it.  The uncaptured launches give the same bits.  step_tokens'
        logits rows are in self.rlogits[:R]."""
        self._step_rows(tokens, True, "step_sample_tokens")
        return self.rsel[:self._rows_at[0]]

    @torch.no_grad()
    def extend(self, tokens: Mapping[int, Sequence[int]]) -> torch.Tensor:
        """Append any number of tokens per named slot (active; no reset), packed into step_tokens calls of at most max_rows rows:
        the logits and caches of that many single steps per slot.  Returns self.logits (each named slot's row: its last token's)."""
        rest = {int(slot): [int(v) for v in t] for slot, t in tokens.items()}
        plan_rows({b: t[:1] for b, t in rest.items()}, [p if a else None for p, a in zip(self._host_pos, self._active)], max(self.max_rows, len(rest)),
                  self.cache_len, "BatchDecodeEngine.extend")                # slots in range, active, no empty list
        for b, t in rest.items():
            if self._host_pos[b] + len(t) > self.cache_len:
                raise RuntimeError(f"BatchDecodeEngine.extend: {len(t)} tokens at position {self._host_pos[b]} overflow slot {b}'s KV cache "
                                   f"({self.cache_len} positions)")
        while rest:
            room, call = self.max_rows, {}
            for b in sorted(rest):
                if room == 0:
                    break
                call[b], rest[b] = rest[b][:room], rest[b][room:]
                room -= len(call[b])
                if not rest[b]:
                    del rest[b]
            self.step_tokens(call)
        return self.logits

    def rewind(self, slot: int, n: int):
        """Drop the slot's positions >= n (n <= position(slot)): its later steps compute what an engine that never saw them computes.
        Only the slot's position moves, on host and device: no batched launch reads a cached byte at or past a slot's position (the
        attention launches mask the keys, the values and the split blocks by it), so the dropped bytes are never read before they are
        overwritten.  The other slots and self.logits are untouched.  The sampler's token history of the slot is left STALE, as in
        DecodeEngine.rewind: call observe_history(slot, ids) with the tokens the sequence now holds before a penalised draw."""
        self._check_slot(slot)
        n = int(n)
        if not self._active[slot]:
            raise RuntimeError(f"BatchDecodeEngine.rewind: slot {slot} is idle")
        if not 0 <= n <= self._host_pos[slot]:
            raise ValueError(f"BatchDecodeEngine.rewind: n={n} outside 0..{self._host_pos[slot]} (slot {slot}'s position)")
        self.pos[slot] = n
        self._host_pos[slot] = n
        return self

    # -- seeded token selection on the device (csrc/mq_sample.hip) ---------------------------------------------
    def set_sampling(self, sampling, streams: Optional[Sequence[int]] = None):
        """Per-slot requests for sample(): one SamplingParams for every slot or one per slot; streams (the sequences' identities)
        default to the slot numbers.  Rewritten in device memory: the captured graphs stay valid.  Penalised and neutral requests
        may mix; a penalised slot reads its own token history (observe_history(slot, ids); generate() keeps it itself)."""
        rows = [sampling] * self.batch if isinstance(sampling, SamplingParams) else list(sampling)
        st = list(range(self.batch)) if streams is None else [check_stream(v) for v in streams]
        if len(rows) != self.batch or len(st) != self.batch:
            raise ValueError(f"BatchDecodeEngine.set_sampling: {len(rows)} requests / {len(st)} streams for {self.batch} slots")
        if self._sampler is None:
            self._sampler = SampleLaunch(self.logits, self.pos, self.tok, self.cache_len)
        self._sampler.set_rows(rows, st)
        return self

    def observe_history(self, slot: int, ids):
        """DecodeEngine.observe_history for one slot: its history is cleared and `ids` are marked as its prompt tokens.  release(slot)
        clears it; set_position(slot, ...) leaves it as it is."""
        self._check_slot(slot)
        if self._sampler is None:
            self.set_sampling(SamplingParams(temperature=0.0))
        self._sampler.observe_prompt(slot, ids, clear=True)
        return self

    @torch.no_grad()
    def sample(self) -> torch.Tensor:
        """mq_sample on the logits rows into tok [B] (device; no host read).  An idle slot keeps its token.  Slot b's token is what
        DecodeEngine.sample draws for that sequence alone under the same request and stream."""
        if self._sampler is None:
            self.set_sampling(SamplingParams(temperature=0.0))
        with torch.cuda.device(self.dev):
            self._select()
        return self.tok

    def logprob_records(self, slot: int, start: int, stop: int) -> TokenLogprobs:
        """The records of slot's tokens at sequence indices [start, stop) (CPU tensors, read back here): index n is the token drawn
        for the slot at position(slot) == n.  Only indices drawn since set_logprobs(n_top) hold records; release() clears nothing."""
        self._check_slot(slot)
        return self._records(slot, start, stop)

    def _capture_sample_step(self):
        """mq_sample + the step for all slots + the position advance as one graph (BatchDecodeEngine.capture's recipe: the launch
        outside the capture runs with every slot idle)."""
        pos0 = self.pos.clone()
        self.pos.fill_(self.cache_len)

        def step():
            self._launch()
            self._advance()
        g = self._sample_graphs[self._lp_key(self._sampler.penalized)] = self._record(self._select, step, before_capture=lambda: self.pos.copy_(pos0))
        return g

    @torch.no_grad()
    def sample_step(self) -> torch.Tensor:
        """sample() and step() on the drawn tokens; after capture() ONE graph replay (recorded on first use)."""
        if self._sampler is None:
            self.set_sampling(SamplingParams(temperature=0.0))
        if self.graph is None:
            self.sample()
            return self.step()
        for b in range(self.batch):
            if self._active[b] and self._host_pos[b] >= self.cache_len:
                raise RuntimeError(f"BatchDecodeEngine.sample_step: slot {b}'s KV cache is full ({self.cache_len} positions); release() it first")
        (self._sample_graphs.get(self._lp_key(self._sampler.penalized)) or self._capture_sample_step()).replay()
        for b in range(self.batch):
            if self._active[b]:
                self._host_pos[b] += 1
        return self.logits

    def position(self, slot: int) -> int:
        """Cached positions of the slot's sequence (what the next step appends at); cache_len for an idle slot."""
        return self._host_pos[slot]

    def active(self, slot: int) -> bool:
        return self._active[slot]

    def cached_keys(self, slot: int, li: int, n: Optional[int] = None) -> torch.Tensor:
        """Layer li's cached keys of the slot: [kv_heads, n positions, head_dim] int8 indices (index - 128)."""
        n = self.position(slot) if n is None else int(n)
        return self.k_cache[li][slot, :, :n]

    def cached_values(self, slot: int, li: int, n: Optional[int] = None) -> torch.Tensor:
        """Layer li's cached values of the slot: [kv_heads, n positions, head_dim] int8 indices (index - 128)."""
        n = self.position(slot) if n is None else int(n)
        return self.v_cache[li][slot, :, :n]

    def _check_slot(self, slot: int):
        if not 0 <= int(slot) < self.batch:
            raise IndexError(f"BatchDecodeEngine: slot {slot} outside 0..{self.batch - 1}")

    def set_position(self, slot: int, pos: int):
        """Make the slot active with `pos` cached positions (benchmarks and prefill())."""
        self._check_slot(slot)
        assert 0 <= int(pos) <= self.cache_len
        self.pos[slot] = int(pos)
        self._host_pos[slot] = int(pos)
        self._active[slot] = True

    def release(self, slot: int):
        """The slot goes idle: its position becomes the cache_len sentinel, its cache and logits row stop changing."""
        self._check_slot(slot)
        self.pos[slot] = self.cache_len
        self._host_pos[slot] = self.cache_len
        self._active[slot] = False
        if self._sampler is not None:
            self._sampler.clear_history(slot)                  # (a no-op until a penalised request has allocated the histories)

    @torch.no_grad()
    def fork(self, forks: Mapping[int, Sequence[int]]):
        """Make source slots' sequences the start of other slots: forks is {source slot: destination slots}.  After the call every
        destination is an active slot that holds its source's sequence, indistinguishable from a slot that prefilled (and stepped) the
        same tokens itself: its caches below position(source) are the source's bytes -- ONE mq_decode_cache_fork launch for all
        sources, destinations and layers -- and its position, pending token (tok), logits row and, once a penalised
        request has allocated the histories, sampler history row are the source's.  A destination may be idle or active; an active
        one is overwritten (bytes at or past the source's position keep their old values and are never read).  The sources and every
        other slot are untouched.
        NOT copied: a slot's sampling request and stream (different streams are the point: set_sampling), and the log-probability
        records below the fork position, which stay with the source -- generate reads only indices from the prompt's end on.
        The captured graphs stay valid (no buffer moves); fork itself runs eagerly, between replays: one small host -> device copy of
        the fork table, the launch, and four index copies of the per-slot state on the same stream.  sample_rows() needs a new
        step_tokens() afterwards.  self.fork_stats = {"sources", "destinations", "positions" (cached positions copied, summed over
        the destinations), "bytes" (cache bytes written)}.
        ValueError / IndexError / RuntimeError with "BatchDecodeEngine.fork: " in front, before anything is launched: a slot out of
        range, an idle source, a source whose cache is full (position cache_len), a destination equal to its source, a destination named twice (by one source or by two), a source that is
        also a destination, an empty mapping or an empty destination list."""
        who = "BatchDecodeEngine.fork: "
        plan = {}
        try:
            plan = {int(src): [int(d) for d in dsts] for src, dsts in forks.items()}
        except (AttributeError, TypeError, ValueError):
            raise ValueError(who + "forks must be a mapping {source slot: sequence of destination slots}") from None
        if not plan:
            raise ValueError(who + "an empty mapping (nothing to fork)")
        parent = list(range(self.batch))
        taken = {}
        for src, dsts in plan.items():
            if not 0 <= src < self.batch:
                raise IndexError(who + f"source slot {src} outside 0..{self.batch - 1}")
            if not self._active[src]:
                raise RuntimeError(who + f"source slot {src} is idle (prefill() or start() it first)")
            if self._host_pos[src] >= self.cache_len:                  # (on the device a full cache reads as the idle sentinel: nothing would be copied)
                raise RuntimeError(who + f"source slot {src}'s KV cache is full ({self.cache_len} positions): its position is the idle "
                                   "sentinel on the device, rewind() it first")
            if not dsts:
                raise ValueError(who + f"source slot {src} has an empty destination list")
            for d in dsts:
                if not 0 <= d < self.batch:
                    raise IndexError(who + f"destination slot {d} outside 0..{self.batch - 1}")
                if d == src:
                    raise ValueError(who + f"slot {src} is its own destination")
                if d in taken:
                    raise ValueError(who + f"destination slot {d} is named twice (by source {taken[d]} and by source {src})")
                taken[d] = src
                parent[d] = src
        both = sorted(set(plan) & set(taken))
        if both:
            raise ValueError(who + f"slot {both[0]} is a source and a destination (no chains: fork from the first source)")
        dst = sorted(taken)
        idx = torch.tensor([dst, [taken[d] for d in dst]], dtype=torch.int64).to(self.dev)
        self._fork_parent.copy_(torch.tensor(parent, dtype=torch.int32), non_blocking=False)
        ops.decode_cache_fork(self._fork_caches, self.pos, self._fork_parent, table=self._fork_table)
        state = [self.pos, self.tok, self.logits]
        if self._sampler is not None and self._sampler.pargs is not None:
            state.append(self._sampler.history)
        for t in state:                                            # (behind the launch, which reads the SOURCES' positions only)
            t.index_copy_(0, idx[0], t.index_select(0, idx[1]))
        for d, src in taken.items():
            self._host_pos[d], self._active[d] = self._host_pos[src], True
        self._rows_at = None
        s = self.shape
        positions = sum(self._host_pos[d] for d in dst)
        self.fork_stats = {"sources": len(plan), "destinations": len(dst), "positions": positions,
                           "bytes": positions * s.head_dim * s.kv_heads * len(self._fork_caches)}
        return self

    def fill_cache_random(self, slot: int, n: int, seed: int = 0):
        """Benchmark helper: n positions of random cached indices in one slot, which becomes active at position n."""
        g = torch.Generator(device=self.dev).manual_seed(seed)
        s = self.shape
        for c in self.k_cache + self.v_cache:
            c[slot, :, :n] = torch.randint(-128, 128, (s.kv_heads, n, s.head_dim), generator=g, device=self.dev, dtype=torch.int8)
        self.set_position(slot, n)

    @torch.no_grad()
    def _step_seq(self, tokens: Sequence[int], slot: int):
        """step() for ONE slot, token by token: the other active slots are parked at the cache_len sentinel for the duration (an idle
        slot's cache and logits row do not change) and get their positions back afterwards."""
        others = [b for b in range(self.batch) if b != slot and self._active[b]]
        saved = self.pos.clone()
        try:
            for b in others:
                self._active[b] = False
                self.pos[b] = self.cache_len
            for tok in tokens:
                self.tok[slot] = int(tok)
                self.step()
        finally:
            for b in others:
                self._active[b] = True
                self.pos[b] = saved[b]

    # a slot's sequence as _DecodeBase's prefill and speculative bodies see it
    def _seq_caches(self, li: int, slot: int):
        return self.k_cache[li][slot], self.v_cache[li][slot]

    def _store_values(self, li: int, values: torch.Tensor, slot: int):
        self.v_cache[li][slot, :, :values.shape[1]] = values

    def _logits_row(self, slot: int) -> torch.Tensor:
        return self.logits[slot]

    @torch.no_grad()
    def prefill(self, slot: int, context_ids, append: bool = False) -> torch.Tensor:
        """DecodeEngine.prefill for one slot: one module-graph forward over the context, its keys / values on their QMatMul input
        grids into the slot's caches, the slot's position behind the context.  The other slots are untouched.  Returns the logits row
        of the last context position.
        append=True: DecodeEngine.prefill(append=True) on this slot's live sequence (same split, same contract, self.append_stats);
        the slot's caches are imported and written in place through their head strides.  The stepped tokens run as single-slot steps
        with the other slots parked; their caches, positions and logits rows do not change."""
        self._check_slot(slot)
        if not append:
            return self._prefill_fill(context_ids, True, slot)
        if not self._active[slot]:
            raise RuntimeError(f"BatchDecodeEngine.prefill: slot {slot} is idle: append continues a live sequence (prefill() or start() it first)")
        return self._prefill_append(context_ids, slot)

    def start(self, slot: int):
        """Make the slot active at position 0 with an empty cache (a sequence fed token by token through step())."""
        self._check_slot(slot)
        for c in self.k_cache + self.v_cache:
            c[slot].zero_()
        self.set_position(slot, 0)

    @torch.no_grad()
    def step(self, tokens: Optional[Sequence[int]] = None) -> torch.Tensor:
        """One step for every active slot: tokens (length B; entries of idle slots are ignored) or None to use the device-side tok [B].
        Returns logits [B, vocab] (device tensor, overwritten by the next step); active slots advance by one position."""
        for b in range(self.batch):
            if self._active[b] and self._host_pos[b] >= self.cache_len:
                raise RuntimeError(f"BatchDecodeEngine.step: slot {b}'s KV cache is full ({self.cache_len} positions); release() it first")
        if tokens is not None:
            t = [int(v) for v in tokens]
            if len(t) != self.batch:
                raise ValueError(f"BatchDecodeEngine.step: {len(t)} tokens for {self.batch} slots")
            self.tok.copy_(torch.tensor(t, dtype=torch.int64), non_blocking=False)
        if self.graph is not None:
            self.graph.replay()
        else:
            with torch.cuda.device(self.dev):
                self._launch()
            self._advance()
        for b in range(self.batch):
            if self._active[b]:
                self._host_pos[b] += 1
        return self.logits

    @torch.no_grad()
    def generate(self, prompts: Sequence[Sequence[int]], max_new_tokens: int, eos_token_id=None, do_sample: bool = False,
                 temperature: float = 0.5, generator: Optional[torch.Generator] = None, sampling=None,
                 streams: Optional[Sequence[int]] = None, draft=None, num_draft: int = 4, logprobs: Optional[int] = None,
                 n: Optional[int] = None):
        """DecodeEngine.generate for up to `batch` prompts at once, each in its own slot: prompt i's list is what DecodeEngine.generate
        returns for it alone (context + new tokens).  Per step the next tokens are chosen on the device (argmax, or multinomial of
        softmax(logits / temperature) per row); the host reads the B token ids.  A sequence stops at its own EOS, after max_new_tokens
        or at the cache end, and its slot is released.
        sampling (one SamplingParams, or one per prompt) with streams (default: the prompt's index in `prompts`): seeded selection by
        mq_sample's rule.  Prompt i's list is then what DecodeEngine.generate(prompts[i], sampling=..., stream=
        streams[i]) returns, bit for bit, whatever the batch, the slot and the other prompts are.  After capture() a step costs one
        graph replay (sample + step) and one read-back of the B tokens.
        draft (greedy only; a callable draft(ids, k) -> at most k proposals such as prompt_lookup_draft(), or one callable per prompt):
        greedy speculative decoding for every prompt at once (_generate_speculative).  Prompt i's list equals the plain greedy one
        token for token; self.spec_stats counts the rounds.
        logprobs (with sampling= only; 0 .. 20): returns (list of ids, list of TokenLogprobs) -- prompt i's records are those of
        DecodeEngine.generate(prompts[i], ..., logprobs=logprobs), bit for bit: one per new token, written on the device behind every
        sample launch and read back once at the end.  None returns what it always did, through the launches and
        graphs without mq_logprob_top.
        n (with sampling= only; k >= 1): k samples of every prompt from ONE encoding of it: each prompt is cached once
        (prefill, or the step path for a one-token prompt) and forked into k - 1 more slots (fork()); sample j of prompt i lives in slot
        i * k + j, so len(prompts) * k <= batch.  sampling is one SamplingParams or one per prompt (it serves that prompt's k samples);
        streams has len(prompts) * k entries in slot order (default: the slot index).  The return nests: out[i][j] is an id list --
        token for token what DecodeEngine.generate(prompts[i], sampling=rows[i], stream=streams[i * k + j]) returns, and so what this
        call returns with the prompt repeated k times -- and with logprobs= the TokenLogprobs nest the same way, bit for bit.  n with a
        greedy draft= is a ValueError (generate_speculative takes n); None runs today's call, launches, graphs and return shape."""
        n_top = check_logprobs("BatchDecodeEngine.generate", logprobs, sampling)
        fan = None
        if n is not None:
            if draft is not None:
                raise ValueError("BatchDecodeEngine.generate: n= draws samples; a draft here is for greedy decoding only (generate_speculative takes n=)")
            prompts, sampling, fan = self._fan_out("BatchDecodeEngine.generate", prompts, sampling, n)
        res = self._generate_checked(prompts, max_new_tokens, eos_token_id, do_sample, temperature, generator, sampling, streams, draft, num_draft,
                                     n_top, fan or 1)
        return res if fan is None else _nest(res, fan, n_top is not None)

    def _fan_out(self, who: str, prompts, sampling, n):
        """generate(n=k)'s arguments in slot order: every prompt and its request k times in a row.  Returns (prompts, requests, k)."""
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
            raise ValueError(f"{who}: n={n!r} must be an integer >= 1 (or None)")
        k, count = int(n), len(prompts)
        if sampling is None:
            raise ValueError(f"{who}: n={k} draws samples and needs sampling= (SamplingParams, one or one per prompt)")
        if count < 1 or count * k > self.batch:
            raise ValueError(f"{who}: {count} prompts x n={k} samples for {self.batch} slots")
        if not isinstance(sampling, SamplingParams):
            if not isinstance(sampling, (list, tuple)) or any(not isinstance(r, SamplingParams) for r in sampling):
                raise TypeError(f"{who}: sampling must be SamplingParams or a sequence of them")
            if len(sampling) != count:
                raise ValueError(f"{who}: {len(sampling)} SamplingParams for {count} prompts (with n= a request serves its prompt's {k} samples)")
            sampling = [r for r in sampling for _ in range(k)]
        return [p for p in prompts for _ in range(k)], sampling, k

    def _generate_checked(self, prompts, max_new_tokens, eos_token_id, do_sample, temperature, generator, sampling, streams, draft, num_draft,
                          n_top, fan: int):
        """generate behind n=: the checks of its other arguments and its body (fan: slots i * fan .. i * fan + fan - 1 hold one prompt)."""
        n = len(prompts)
        if not 0 < n <= self.batch:
            raise ValueError(f"BatchDecodeEngine.generate: {n} prompts for {self.batch} slots")
        drafts = None
        if draft is not None:
            if sampling is not None:
                validate_generate_args("BatchDecodeEngine.generate", sampling, do_sample, draft)
            if do_sample:
                raise ValueError("BatchDecodeEngine.generate: a draft is for greedy decoding only (do_sample=True with a draft)")
            drafts = self._check_drafts("BatchDecodeEngine.generate", draft, num_draft, n)
        if sampling is not None:
            validate_generate_args("BatchDecodeEngine.generate", sampling, do_sample)
            rows = [sampling] * n if isinstance(sampling, SamplingParams) else list(sampling)
            st = list(range(n)) if streams is None else [check_stream(v) for v in streams]
            if len(rows) != n or len(st) != n:
                raise ValueError(f"BatchDecodeEngine.generate: {len(rows)} SamplingParams / {len(st)} streams for {_count(n, fan)}")
            if any(not isinstance(r, SamplingParams) for r in rows):
                raise TypeError("BatchDecodeEngine.generate: sampling must be SamplingParams or a sequence of them")
            if any(len(p) + max_new_tokens > self.cache_len for p in prompts):
                raise ValueError(f"BatchDecodeEngine.generate: a prompt plus {max_new_tokens} new tokens exceeds the cache ({self.cache_len} positions)")
        elif streams is not None:
            raise ValueError("BatchDecodeEngine.generate: streams= belongs to sampling=")
        prompts = [[int(t) for t in p] for p in prompts]
        assert all(len(p) > 0 for p in prompts)
        eos = _eos_set(eos_token_id)
        with self._logprobs_for(n_top):
            return self._generate(prompts, max_new_tokens, eos, do_sample, temperature, generator, (rows, st) if sampling is not None else None, drafts,
                                  num_draft, n_top, fan)

    def _generate(self, prompts, max_new_tokens: int, eos: set, do_sample: bool, temperature: float, generator, sampling, drafts, num_draft: int,
                  n_top: Optional[int], fan: int = 1):
        """generate's body behind its argument checks (sampling: None or (requests, streams) per prompt)."""
        n = len(prompts)
        if max_new_tokens <= 0:
            return prompts if n_top is None else (prompts, [self.logprob_records(i, 0, 0) for i in range(n)])
        self._start_prompts(prompts, fan)
        outs = [list(p) for p in prompts]
        made = [0] * n
        live = list(range(n))
        if drafts is not None:
            return self._generate_speculative(outs, max_new_tokens, eos, drafts, int(num_draft), _BatchGreedy())
        if sampling is not None:
            rows, st = sampling
            idle = SamplingParams(temperature=0.0)
            self.set_sampling(rows + [idle] * (self.batch - n), st + [0] * (self.batch - n))
            if self._sampler.penalized:
                for i, p in enumerate(prompts):
                    self._sampler.observe_prompt(i, p)             # slot i's history: cleared, then its prompt
            while live:
                if all(made[i] + 1 >= max_new_tokens for i in live):
                    self.sample()                                  # the last tokens need no step
                else:
                    self.sample_step()
                nxt = self.tok.tolist()
                for i in list(live):
                    outs[i].append(nxt[i])
                    made[i] += 1
                    if nxt[i] in eos or made[i] >= max_new_tokens:
                        self.release(i)
                        live.remove(i)
            return outs if n_top is None else (outs, [self.logprob_records(i, len(prompts[i]), len(outs[i])) for i in range(n)])
        while live:
            if do_sample:
                probs = torch.softmax(self.logits / temperature, dim=-1)
                self.tok.copy_(torch.multinomial(probs, num_samples=1, generator=generator).view(-1))
            else:
                torch.argmax(self.logits, dim=-1, out=self.tok)
            nxt = self.tok.tolist()
            for i in list(live):
                outs[i].append(nxt[i])
                made[i] += 1
                if nxt[i] in eos or made[i] >= max_new_tokens or self._host_pos[i] >= self.cache_len:
                    self.release(i)
                    live.remove(i)
            if live:
                self.step()
        return outs

    # -- beam search (csrc/mq_beam.hip, csrc/mq_decode_reorder.hip) -----------------------------------------------
    def _beam_buffers(self, G: int, K: int):
        """generate_beam's device buffers: `pack` (ONE host -> device copy per step: tok int64 [B], then parent, group int32 [B] and cum
        fp32 [B]) and `rec` (ONE read-back per step: score, row, token, logprob [G][K], then row_lse [B]); both int32, viewed."""
        B = self.batch
        if self._beam is None:
            pack = torch.zeros(5 * B, dtype=torch.int32, device=self.dev)
            self._beam = {"pack": pack, "tok": pack[:2 * B].view(torch.int64), "parent": pack[2 * B:3 * B], "group": pack[3 * B:4 * B],
                          "cum": pack[4 * B:].view(torch.float32), "rec": torch.zeros(4 * MAX_BATCH * _lib.MQ_LOGPROB_MAX_TOP + B, dtype=torch.int32, device=self.dev),
                          "scratch": torch.empty(_lib.MQ_BEAM_SCRATCH_BYTES, dtype=torch.uint8, device=self.dev)}
        b, n = self._beam, G * K
        rec = b["rec"]
        b["out"] = (rec[:n].view(torch.float32).view(G, K), rec[n:2 * n].view(G, K), rec[2 * n:3 * n].view(G, K),
                    rec[3 * n:4 * n].view(torch.float32).view(G, K), rec[4 * n:4 * n + B].view(torch.float32))
        return b

    def _beam_upload(self, tok, parent, group, cum):
        B = self.batch
        h = np.zeros(5 * B, dtype=np.int32)
        h[:2 * B].view(np.int64)[:] = tok
        h[2 * B:3 * B], h[3 * B:4 * B] = parent, group
        h[4 * B:].view(np.float32)[:] = cum
        self._beam["pack"].copy_(torch.from_numpy(h), non_blocking=False)

    @torch.no_grad()
    def generate_beam(self, prompts: Sequence[Sequence[int]], max_new_tokens: int, num_beams: int, *, eos_token_id=None,
                      length_penalty: float = 1.0, early_stopping: bool = True, num_return_sequences: int = 1) -> List[BeamResult]:
        """Beam search for up to batch // num_beams prompts at once: W = num_beams beams per prompt, prompt g's in
        slots g W .. g W + W - 1.  Returns one BeamResult per prompt: the best num_return_sequences hypotheses (sequences: context +
        new tokens, an ending EOS included; scores; sum_logprobs), best first.  No sampling and no penalties are involved: the sampler
        histories and the logprobs= records stay untouched.  Each prompt is encoded ONCE (slot g W); then per step: mq_beam_select over
        self.logits (K = max(2, 1 + |eos|) W candidates per prompt), one read-back of the n_groups x K records, the host rule, one
        packed upload of parent / token / cum, mq_decode_cache_reorder (skipped when the table is the identity), the per-slot state
        from a gathered temporary, and the ordinary step() (a graph replay after capture()).  A finished prompt's slots are released
        and the others go on.  self.beam_stats = {"steps", "selects", "reorders", "positions", "bytes"} (step() calls, select and
        re-order launches, cached positions moved, cache bytes written).
        THE HOST RULE (after transformers' BeamSearchScorer).  L = the new tokens of a hypothesis once the current token is appended.
        The K candidates are walked in order: an EOS at j >= W is skipped; an EOS at j < W adds (ids of the row + EOS, s) to the
        prompt's finished list with score s / L ** length_penalty; any other candidate becomes the next beam (row, token, s) until W
        are taken.  The finished list keeps the best W: adding drops the worst, and on equal scores the earlier entry stays.  After
        the walk the prompt is done iff it has W finished hypotheses and early_stopping is true or the worst finished score is >=
        cand_score[0] / L ** length_penalty.  At max_new_tokens every live beam of a prompt that is not done is added in beam order
        with cum / L ** length_penalty.  Returned: score descending, earlier-added first on ties.  Scores are Python floats (the
        fp32 sum divided in double precision).
        CONTRACT.  Prompt g's result is a function of the prompt and the arguments only: bit for bit the same alone or beside other
        prompts, in any group position, captured or eager.
        ValueError / IndexError with "BatchDecodeEngine.generate_beam: " in front, before anything is launched: num_beams outside
        1 .. 8, no prompt or len(prompts) * num_beams > batch, an empty prompt, a token outside the vocabulary (IndexError),
        max_new_tokens < 1, num_return_sequences outside 1 .. num_beams, K > 20 or above the vocabulary, a prompt plus max_new_tokens
        past the cache, a length_penalty that is not a finite number, an early_stopping that is not a bool."""
        who = "BatchDecodeEngine.generate_beam: "

        def integer(v):
            return isinstance(v, (int, np.integer)) and not isinstance(v, bool)
        if not integer(num_beams) or not 1 <= num_beams <= MAX_BATCH:
            raise ValueError(who + f"num_beams={num_beams!r} must be an integer in 1..{MAX_BATCH}")
        W = int(num_beams)
        try:
            prompts = [[int(t) for t in p] for p in prompts]
        except (TypeError, ValueError):
            raise ValueError(who + "prompts must be a sequence of token id sequences") from None
        G = len(prompts)
        if G < 1 or G * W > self.batch:
            raise ValueError(who + f"{G} prompts x num_beams={W} for {self.batch} slots")
        for g, p in enumerate(prompts):
            if not p:
                raise ValueError(who + f"prompt {g} is empty")
            for t in p:
                if not 0 <= t < self.shape.vocab:
                    raise IndexError(who + f"token {t} of prompt {g} outside the vocabulary (0..{self.shape.vocab - 1})")
        if not integer(max_new_tokens) or max_new_tokens < 1:
            raise ValueError(who + f"max_new_tokens={max_new_tokens!r} must be an integer >= 1")
        T = int(max_new_tokens)
        if not integer(num_return_sequences) or not 1 <= num_return_sequences <= W:
            raise ValueError(who + f"num_return_sequences={num_return_sequences!r} must be an integer in 1..num_beams ({W})")
        if not (eos_token_id is None or integer(eos_token_id) or (isinstance(eos_token_id, (list, tuple, set, frozenset)) and all(integer(t) for t in eos_token_id))):
            raise ValueError(who + f"eos_token_id={eos_token_id!r} must be None, a token id or a collection of token ids")
        eos = {int(t) for t in _eos_set(int(eos_token_id) if integer(eos_token_id) else eos_token_id)}
        K = max(2, 1 + len(eos)) * W
        if K > _lib.MQ_LOGPROB_MAX_TOP:
            raise ValueError(who + f"max(2, 1 + {len(eos)} EOS ids) x num_beams={W} = {K} candidates per step, above {_lib.MQ_LOGPROB_MAX_TOP}")
        if K > self.shape.vocab:
            raise ValueError(who + f"{K} candidates per step, above the vocabulary ({self.shape.vocab})")
        if any(len(p) + T > self.cache_len for p in prompts):
            raise ValueError(who + f"a prompt plus {T} new tokens exceeds the cache ({self.cache_len} positions)")
        if isinstance(length_penalty, bool) or not isinstance(length_penalty, (int, float, np.integer, np.floating)) or not np.isfinite(length_penalty):
            raise ValueError(who + f"length_penalty={length_penalty!r} must be a finite number")
        if not isinstance(early_stopping, (bool, np.bool_)):
            raise ValueError(who + f"early_stopping={early_stopping!r} must be True or False")
        lp_exp = float(length_penalty)

        # every prompt encoded once, in its group's first slot (generate's own start: one-token prompts through the step kernels)
        B = self.batch
        for b in range(B):
            self.release(b)
        first = [g * W for g in range(G)]
        short = [g for g in range(G) if len(prompts[g]) == 1]
        if short:
            for g in short:
                self.start(first[g])
            toks = [0] * B
            for g in short:
                toks[first[g]] = prompts[g][0]
            self.step(toks)
        for g in range(G):
            if len(prompts[g]) > 1:
                self.prefill(first[g], prompts[g])
        self._rows_at = None

        buf = self._beam_buffers(G, K)
        s = self.shape
        pos_bytes = s.head_dim * s.kv_heads * len(self._fork_caches)
        stats = self.beam_stats = {"steps": 0, "selects": 0, "reorders": 0, "positions": 0, "bytes": 0}
        beams = [[([], np.float32(0.0))] for _ in range(G)]        # per prompt: (new ids, cum) of the live beams, beam b in slot g W + b
        hyps = [_BeamHyps(W) for _ in range(G)]
        live = list(range(G))
        group = [-1] * B
        cum = [0.0] * B
        for g in live:
            group[first[g]] = g
        self._beam_upload([0] * B, list(range(B)), group, cum)
        for step in range(T):
            L = step + 1
            norm = float(L) ** lp_exp
            ops.beam_select(self.logits, buf["cum"], buf["group"], G, K, out=buf["out"], scratch=buf["scratch"])
            stats["selects"] += 1
            rec = buf["rec"][:4 * G * K].cpu().numpy()             # ONE read-back: the n_groups x K records
            score, row = rec[:G * K].view(np.float32).reshape(G, K), rec[G * K:2 * G * K].reshape(G, K)
            token, parent = rec[2 * G * K:3 * G * K].reshape(G, K), list(range(B))
            tok = [0] * B
            for g in list(live):
                nxt = []
                for j in range(K):
                    r, t, sc = int(row[g, j]), int(token[g, j]), score[g, j]
                    if r < 0:
                        break                                      # (padding: the group has no more candidates)
                    ids = beams[g][r - first[g]][0]
                    if t in eos:
                        if j < W:
                            hyps[g].add(ids + [t], float(sc), float(sc) / norm)
                        continue
                    nxt.append((r, t, sc))
                    if len(nxt) == W:
                        break
                done = hyps[g].full() and (bool(early_stopping) or hyps[g].worst() >= float(score[g, 0]) / norm)
                if not done and len(nxt) < W:
                    raise RuntimeError(who + f"prompt {g} has {len(nxt)} continuations for {W} beams at step {step}")
                if not done and L == T:                            # the end: the live beams, in beam order
                    for r, t, sc in nxt:
                        hyps[g].add(beams[g][r - first[g]][0] + [t], float(sc), float(sc) / norm)
                    done = True
                if done:
                    live.remove(g)
                    for b in range(first[g], first[g] + W):
                        self.release(b)
                        group[b] = -1
                    continue
                beams[g] = [(beams[g][r - first[g]][0] + [t], sc) for r, t, sc in nxt]
                for b, (r, t, sc) in enumerate(nxt):
                    d = first[g] + b
                    parent[d], tok[d], group[d], cum[d] = r, t, g, float(sc)
            if not live:
                break
            self._beam_upload(tok, parent, group, cum)
            moved = sum(self._host_pos[p] for d, p in enumerate(parent) if p != d)
            if moved:                                              # (the identity writes nothing: no launch)
                ops.decode_cache_reorder(self._fork_caches, self.pos, buf["parent"], table=self._fork_table)
                stats["reorders"] += 1
                stats["positions"] += moved
                stats["bytes"] += moved * pos_bytes
                self.pos.copy_(self.pos.index_select(0, buf["parent"]))      # (behind the launch, which reads the old positions)
                hp, act = list(self._host_pos), list(self._active)
                for d, p in enumerate(parent):
                    self._host_pos[d], self._active[d] = hp[p], act[p]
            self.tok.copy_(buf["tok"])
            self.step()
            stats["steps"] += 1
        out = []
        for g in range(G):
            best = hyps[g].items[:int(num_return_sequences)]
            out.append(BeamResult([prompts[g] + ids for _, _, ids, _ in best], [sc for sc, _, _, _ in best], [sl for _, _, _, sl in best]))
        return out

    def _check_drafts(self, who: str, draft, num_draft, n: int, fan: int = 1) -> list:
        """The drafts of a batched speculative generation, one per prompt: a callable (for every prompt) or a sequence of n callables."""
        drafts = list(draft) if isinstance(draft, (list, tuple)) else [draft] * n
        if any(isinstance(d, _DecodeBase) for d in drafts):
            raise TypeError(f"{who}: an engine cannot draft for a batch: pass callable drafts, draft(ids, k) -> list of "
                            "token ids (one for all prompts or one per prompt)")
        for d in drafts:
            _check_draft(who, self, d, num_draft, (), "a callable draft(ids, k) -> list of token ids, or a sequence "
                         "of such callable drafts, one per prompt")
        if len(drafts) != n:
            raise ValueError(f"{who}: {len(drafts)} drafts for {_count(n, fan)}" + (f": one draft, one per prompt ({n // fan}) or one per sample" if fan > 1 else ""))
        return drafts

    def _start_prompts(self, prompts: Sequence[Sequence[int]], fan: int = 1):
        """Every slot released, then prompt i cached in slot i: one-token prompts go through the step kernels (as DecodeEngine.generate),
        alone; longer ones through the prefill forward.  fan > 1 (generate(n=fan): prompts holds every prompt fan times in a row): only
        the first slot of each run caches its prompt, and ONE fork() gives it to the run's other slots."""
        for b in range(self.batch):
            self.release(b)
        first = range(0, len(prompts), fan)
        short = [i for i in first if len(prompts[i]) == 1]
        if short:
            for i in short:
                self.start(i)
            self.step([prompts[i][0] if i in short else 0 for i in range(self.batch)])
        for i in first:
            if len(prompts[i]) > 1:
                self.prefill(i, prompts[i])
        if fan > 1:
            self.fork({i: range(i + 1, i + fan) for i in first})

    @torch.no_grad()
    def generate_speculative(self, prompts: Sequence[Sequence[int]], max_new_tokens: int, draft, *, sampling, streams: Optional[Sequence[int]] = None,
                             num_draft: int = 4, eos_token_id=None, logprobs: Optional[int] = None, n: Optional[int] = None):
        """Speculative decoding under seeded sampling for up to `batch` prompts at once: prompt i's list is, token for
        token, what generate(prompts, max_new_tokens, sampling=sampling, streams=streams)[i] and DecodeEngine.generate(prompts[i],
        sampling=rows[i], stream=streams[i]) return, whatever the drafts propose and whatever else is in the batch.  Token n of a
        sequence is a function of its logits, its request, its stream and n alone, so there is no rejection scheme: every prompt's
        first token comes from sample(); then per round (_generate_speculative) ONE step_sample_tokens runs [t_i, d1 .. dk_i] for all
        live slots with mq_sample_ragged drawing every row at its own index under its own slot's request (one graph after capture()),
        one read-back brings the R tokens, spec_accept keeps plain sampling's next tokens per slot and rewind drops the rest; while any
        request is penalised the kept tokens of all slots are then counted into the histories by one history_count_ragged launch.
        sampling: one SamplingParams or one per prompt; streams: default, the prompt's index.  draft: a callable draft(ids, k) -> at
        most k proposals, or one callable per prompt; an engine cannot draft for a batch (TypeError).  The stops are the sampled
        generate's: a sequence ends at its own EOS or after max_new_tokens.  self.spec_stats counts the rounds.
        logprobs (0 .. 20): returns (list of ids, list of TokenLogprobs), the records of generate(..., logprobs=logprobs).  Every row of
        a round writes its record at its own (slot, token index): a rejected row's record is overwritten when that index is drawn
        again, and nothing behind the returned ids is read, so no bookkeeping is needed.
        n: generate's n= through the same prompt start (one encoding per prompt, then fork()): out[i][j], nested, is generate(...,
        n=n)'s.  A callable draft serves every sample; a sequence holds one draft per prompt, or one per sample (len(prompts) * n, in
        slot order)."""
        who = "BatchDecodeEngine.generate_speculative"
        n_top = check_logprobs(who, logprobs, sampling)
        fan = 1
        if n is not None:
            count = len(prompts)
            prompts, sampling, fan = self._fan_out(who, prompts, sampling, n)
            if isinstance(draft, (list, tuple)) and len(draft) == count:
                draft = [d for d in draft for _ in range(fan)]
        res = self._speculative_checked(who, prompts, max_new_tokens, draft, sampling, streams, num_draft, eos_token_id, n_top, fan)
        return res if n is None else _nest(res, fan, n_top is not None)

    def _speculative_checked(self, who, prompts, max_new_tokens, draft, sampling, streams, num_draft, eos_token_id, n_top, fan: int):
        """generate_speculative behind n=: the checks of its other arguments and its body."""
        n = len(prompts)
        if not 0 < n <= self.batch:
            raise ValueError(f"{who}: {n} prompts for {self.batch} slots")
        drafts = self._check_drafts(who, draft, num_draft, n, fan)
        if isinstance(sampling, SamplingParams):
            rows = [sampling] * n
        elif isinstance(sampling, (list, tuple)) and all(isinstance(r, SamplingParams) for r in sampling):
            rows = list(sampling)
        else:
            raise TypeError(f"{who}: sampling must be SamplingParams or a sequence of them, got {type(sampling).__name__}")
        st = list(range(n)) if streams is None else [check_stream(v) for v in streams]
        if len(rows) != n or len(st) != n:
            raise ValueError(f"{who}: {len(rows)} SamplingParams / {len(st)} streams for {_count(n, fan)}")
        if any(len(p) + max_new_tokens > self.cache_len for p in prompts):
            raise ValueError(f"{who}: a prompt plus {max_new_tokens} new tokens exceeds the cache ({self.cache_len} positions)")
        prompts = [[int(t) for t in p] for p in prompts]
        assert all(len(p) > 0 for p in prompts)
        with self._logprobs_for(n_top):
            if max_new_tokens <= 0:
                return prompts if n_top is None else (prompts, [self.logprob_records(i, 0, 0) for i in range(n)])
            self._start_prompts(prompts, fan)
            select = _BatchSampled(rows, st)
            select.start(self, prompts)
            outs = self._generate_speculative([list(p) for p in prompts], max_new_tokens, _eos_set(eos_token_id), drafts, int(num_draft), select)
            return outs if n_top is None else (outs, [self.logprob_records(i, len(prompts[i]), len(outs[i])) for i in range(n)])

    def _generate_speculative(self, outs: List[List[int]], max_new_tokens: int, eos: set, drafts, num_draft: int, select) -> List[List[int]]:
        """Speculative decoding across the batch, for generate(draft=...) (select: _BatchGreedy) and generate_speculative (_BatchSampled);
        slot i holds outs[i] (its prompt, cached).  The first new token of every prompt is chosen from its context's logits.  Then per
        round, with t_i slot i's last token (not yet cached) and P_i its position: the live slots share the step's rows
        (spec_row_budget), slot i's draft proposes k_i tokens, ONE ragged step runs [t_i, d1 .. dk_i] for every live slot with `select`
        choosing the token behind every row, one read-back brings them, and per slot spec_accept keeps the plain loop's next tokens and
        rewind(slot, P_i + kept) drops the rest (_spec_keep); select.count then sees the kept tokens of all slots at once.  Every kept
        token is the plain loop's: a slot's row j holds the logits after t, d1 .. dj, bit for bit, and a token depends on its row
        (greedy) or on its row, its slot's request and its index (sampling) alone.  The stops are plain generate's: EOS,
        max_new_tokens, the cache end.  More live slots than max_rows (an engine whose shape lowered max_rows below its batch) take a
        plain step() instead, whose own selection counts what it draws."""
        n = len(outs)
        stats = self.spec_stats = _spec_stats()
        made, live = [0] * n, []
        first = select.first(self)
        for i in range(n):
            outs[i].append(first[i])
            made[i] = 1
            if first[i] in eos or made[i] >= max_new_tokens or self._host_pos[i] >= self.cache_len:
                self.release(i)
            else:
                live.append(i)
        while live:
            P = {i: self._host_pos[i] for i in live}
            stats["rounds"] += 1
            stats["target_steps"] += 1
            if len(live) > self.max_rows:
                drawn = select.plain(self, [outs[i][-1] if i in P else 0 for i in range(self.batch)])
                props = {i: [] for i in live}
                rows = {i: [drawn[i]] for i in live}
                views = {}
            else:
                ks = spec_row_budget(num_draft, self.max_rows, [max_new_tokens - made[i] for i in live], [self.cache_len - P[i] for i in live])
                props = {i: ([int(v) for v in drafts[i](list(outs[i]), k)][:k] if k > 0 else []) for i, k in zip(live, ks)}
                drawn = select.rows(self, {i: [outs[i][-1]] + props[i] for i in live})       # ONE read-back for all slots
                rows, views, r0 = {}, {}, 0
                for i in live:                                     # (ascending slots: the rows' order)
                    rows[i], views[i] = drawn[r0:r0 + 1 + len(props[i])], self.rlogits[r0:r0 + 1 + len(props[i])]
                    r0 += 1 + len(props[i])
            kept, stopped = [], []
            for i in live:
                new, _, stop = self._spec_keep(rows[i], props[i], eos, max_new_tokens - made[i], views.get(i), i)
                outs[i] += new
                made[i] += len(new)
                if views:
                    kept += [(i, t) for t in new]
                if stop:
                    stopped.append(i)
            select.count(self, kept)                               # (before a stopped slot's release forgets its history)
            for i in stopped:
                self.release(i)
                live.remove(i)
        return outs
