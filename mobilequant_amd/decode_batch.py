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
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence

import torch

from . import _lib
from .decode import DecodeEngine, _DecodeBase, _eos_set, _Target
from .sampling import SampleLaunch, SamplingParams, check_stream, validate_generate_args

MAX_BATCH = 8


class BatchDecodeEngine(_DecodeBase):
    """B single-token decode streams over one model.  Slots are filled with prefill(slot, ids), emptied with release(slot) and all
    active slots advance together with step()."""

    # LONG_FROM / LONG_SPLITS (the base's) apply per sequence, on the device; MAX_IMAGE_BYTES / MAX_HEAD_FLOATS bound B * K and B * hidden

    def __init__(self, model, batch: int, cache_len: int = 2048):
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
        self.logits = torch.zeros(B, s.vocab, device=dev)
        self.pos = torch.full((B,), self.cache_len, dtype=torch.int32, device=dev)       # every slot idle
        self.tok = torch.zeros(B, dtype=torch.int64, device=dev)
        # [B][kv_heads][cache_len][head_dim] int8 indices (index - 128) on qk_bmm.input2 / pv_bmm.input2's grids
        self.k_cache = [torch.zeros(B, s.kv_heads, self.cache_len, s.head_dim, dtype=torch.int8, device=dev) for _ in model.layers]
        self.v_cache = [torch.zeros(B, s.kv_heads, self.cache_len, s.head_dim, dtype=torch.int8, device=dev) for _ in model.layers]
        self._host_pos = [self.cache_len] * B
        self._active = [False] * B
        self.graph = None
        self.append_stats = None             # what the last prefill(slot, ids, append=True) did
        self._append_images = None           # per layer ImageCache of prefill(append=True), allocated on first use
        self._sampler = None                 # mq_sample over logits / pos / tok (sample(), generate(sampling=...))
        self._sample_graphs = {}             # penalised -> the captured sample + step graph, recorded on first use after capture()
        self._lower()

    def _lower(self):
        """Launch records from the model as it is now (_lower_model): per layer the five-launch chain over the B rows of the slot buffers,
        a sequence per row."""
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
            self._sampler.launch()
        return self.tok

    def _capture_sample_step(self):
        """mq_sample + the step for all slots + the position advance as one graph (BatchDecodeEngine.capture's recipe: the launch
        outside the capture runs with every slot idle)."""
        pos0 = self.pos.clone()
        self.pos.fill_(self.cache_len)

        def step():
            self._launch()
            self._advance()
        g = self._sample_graphs[self._sampler.penalized] = self._record(self._sampler.launch, step, before_capture=lambda: self.pos.copy_(pos0))
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
        (self._sample_graphs.get(self._sampler.penalized) or self._capture_sample_step()).replay()
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

    def fill_cache_random(self, slot: int, n: int, seed: int = 0):
        """Benchmark helper: n positions of random cached indices in one slot, which becomes active at position n."""
        g = torch.Generator(device=self.dev).manual_seed(seed)
        s = self.shape
        for c in self.k_cache + self.v_cache:
            c[slot, :, :n] = torch.randint(-128, 128, (s.kv_heads, n, s.head_dim), generator=g, device=self.dev, dtype=torch.int8)
        self.set_position(slot, n)

    @torch.no_grad()
    def _step_slot(self, slot: int, tokens: Sequence[int]):
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

    @torch.no_grad()
    def _prefill_append(self, slot: int, context_ids) -> torch.Tensor:
        t = [int(v) for v in context_ids]
        if not self._active[slot]:
            raise RuntimeError(f"BatchDecodeEngine.prefill: slot {slot} is idle: append continues a live sequence (prefill() or start() it first)")
        P = self._host_pos[slot]
        if not t:
            raise ValueError("BatchDecodeEngine.prefill: no tokens to append")
        if P + len(t) > self.cache_len:
            raise RuntimeError(f"BatchDecodeEngine.prefill: {len(t)} tokens appended at position {P} overflow slot {slot}'s KV cache "
                               f"({self.cache_len} positions)")
        if P == 0:
            self.append_stats = {"stepped": 0, "prefilled": len(t), "reason": None}
            return self.prefill(slot, t)
        self._sync_grids()
        head, reason = self._append_split(P, len(t))
        if head:
            self._step_slot(slot, t[:head])
        if head < len(t):
            row = self._append_chunk(t[head:], P + head, lambda li: (self.k_cache[li][slot], self.v_cache[li][slot]), False)
            if row is None:
                reason = "the model's attention refused the image cache"
                self._step_slot(slot, t[head:])
                head = len(t)
            else:
                self.set_position(slot, P + len(t))
                self.logits[slot].copy_(row)
        self.append_stats = {"stepped": head, "prefilled": len(t) - head, "reason": reason}
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
        if append:
            return self._prefill_append(slot, context_ids)
        ids = torch.as_tensor([int(t) for t in context_ids], dtype=torch.long, device=self.dev).view(1, -1)
        S = ids.shape[1]
        assert 0 < S <= self.cache_len
        self._sync_grids()
        raw = self.model.new_cache(1, S, device=self.dev)
        logits = self.model(ids, cache=raw, last_logits_only=True)
        for li, layer in enumerate(self.model.layers):
            att = layer.self_attn
            self.k_cache[li][slot].zero_()
            self.v_cache[li][slot].zero_()
            self.k_cache[li][slot, :, :S] = att.qk_bmm.input2_quantizer.quantize_to_int(raw[li][0][0].contiguous())[0]
            self.v_cache[li][slot, :, :S] = att.pv_bmm.input2_quantizer.quantize_to_int(raw[li][1][0].contiguous())[0]
        self.set_position(slot, S)
        self.logits[slot].copy_(logits[0, -1])
        return self.logits[slot]

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
                 streams: Optional[Sequence[int]] = None) -> List[List[int]]:
        """DecodeEngine.generate for up to `batch` prompts at once, each in its own slot: prompt i's list is what DecodeEngine.generate
        returns for it alone (context + new tokens).  Per step the next tokens are chosen on the device (argmax, or multinomial of
        softmax(logits / temperature) per row); the host reads the B token ids.  A sequence stops at its own EOS, after max_new_tokens
        or at the cache end, and its slot is released.
        sampling (one SamplingParams, or one per prompt) with streams (default: the prompt's index in `prompts`): seeded selection by
        mq_sample's rule.  Prompt i's list is then what DecodeEngine.generate(prompts[i], sampling=..., stream=
        streams[i]) returns, bit for bit, whatever the batch, the slot and the other prompts are.  After capture() a step costs one
        graph replay (sample + step) and one read-back of the B tokens."""
        n = len(prompts)
        if not 0 < n <= self.batch:
            raise ValueError(f"BatchDecodeEngine.generate: {n} prompts for {self.batch} slots")
        if sampling is not None:
            validate_generate_args("BatchDecodeEngine.generate", sampling, do_sample)
            rows = [sampling] * n if isinstance(sampling, SamplingParams) else list(sampling)
            st = list(range(n)) if streams is None else [check_stream(v) for v in streams]
            if len(rows) != n or len(st) != n:
                raise ValueError(f"BatchDecodeEngine.generate: {len(rows)} SamplingParams / {len(st)} streams for {n} prompts")
            if any(not isinstance(r, SamplingParams) for r in rows):
                raise TypeError("BatchDecodeEngine.generate: sampling must be SamplingParams or a sequence of them")
            if any(len(p) + max_new_tokens > self.cache_len for p in prompts):
                raise ValueError(f"BatchDecodeEngine.generate: a prompt plus {max_new_tokens} new tokens exceeds the cache ({self.cache_len} positions)")
        elif streams is not None:
            raise ValueError("BatchDecodeEngine.generate: streams= belongs to sampling=")
        prompts = [[int(t) for t in p] for p in prompts]
        assert all(len(p) > 0 for p in prompts)
        eos = _eos_set(eos_token_id)
        if max_new_tokens <= 0:
            return prompts
        for b in range(self.batch):
            self.release(b)
        # one-token prompts go through the step kernels (as DecodeEngine.generate), alone; longer ones through the prefill forward
        short = [i for i, p in enumerate(prompts) if len(p) == 1]
        if short:
            for i in short:
                self.start(i)
            self.step([prompts[i][0] if i in short else 0 for i in range(self.batch)])
        for i, p in enumerate(prompts):
            if len(p) > 1:
                self.prefill(i, p)
        outs = [list(p) for p in prompts]
        made = [0] * n
        live = list(range(n))
        if sampling is not None:
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
            return outs
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
