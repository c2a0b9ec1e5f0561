"""Single-token decode with a static KV cache: MI355X-native counterpart of the per-token body of ``SimModel.generate``
(mobilellm/model/sim_model.py:160-221) for a simulated-quant llama-style model.

``DecodeEngine`` takes a ``mobilequant_amd.llama.LlamaForCausalLM`` that went through the reference's surgery
(``create_sim_qmodel`` -> ``update_qcfg`` / mixed-precision rules -> ``set_scale_and_offset``) and lowers every decoder layer to the
five fused launches of ``csrc/mq_decode.hip``:

    input_layernorm + q|k|v stream  ->  RoPE / cache append / qk_bmm / softmax / pv_bmm  ->  o_proj stream + residual
    ->  post_attention_layernorm + interleaved w1|w3 stream + QSiLU * (.) + w2's input quantizer  ->  w2 stream + residual

plus final norm + lm_head (floating point, as the surgery leaves them: qmodule.py:843).  Integer weights, epilogue vectors and
quantizer grids are taken from the Q-modules themselves (the same caches the prefill path uses), so a decode step computes what
the module graph computes for that position: each logit within the tolerance the prefill kernels state.  The token
id and the position live in device memory: ``capture()`` records ONE hipGraph that serves every step of a generation.
W8A8 (8-bit weights); 8-bit unsigned activation grids; 16-bit grids where the recipe puts them (norm inputs, o_proj / w2 outputs,
qk_bmm output, pv_bmm input).

The layer is lowered in one place, ``_DecodeBase``: ``_layer_images`` validates a layer and builds its norms and weight images once,
``_lower_chain`` (five launches) and ``DecodeEngine._lower_chain4`` (four) turn them into launch records through the same per-launch
helpers.  An engine asks for a chain with a ``_Target``: the buffers, the row count and how the attention record is wrapped.  The
single-row chain, the T-row chain of ``step_tokens`` and ``BatchDecodeEngine``'s B-row chain are three such calls; every hipGraph is
recorded by ``_DecodeBase._record``.
"""
from __future__ import annotations

import contextlib
import ctypes
from typing import Callable, Dict, List, Mapping, NamedTuple, Optional, Sequence, Tuple, Union

import torch

from . import _lib, ops
from ._lib import (MQ_U8, MqDecodeAttentionArgs, MqDecodeAttentionBatchArgs, MqDecodeAttentionMultiArgs, MqDecodeAttentionOprojArgs, MqDecodeAttentionRaggedArgs, MqDecodeGemvArgs, MqDecodeGemvBatchArgs,
                   MqDecodeGemvGroupedArgs, MqDecodeHeadBatchArgs, MqGrid)
from .quantization import qmodule as Q
from .sampling import (LogprobLaunch, RowsLaunch, SampleLaunch, SamplingParams, TokenLogprobs, check_logprobs, check_stream, history_count,
                       validate_generate_args)


def _grid(q: Optional[Q.Quantizer], keep: list) -> MqGrid:
    """Device view of a static per-tensor quantizer (absent / bypassed -> the null grid)."""
    if q is None or q.bypassed():
        return MqGrid(None, None, 0.0, 0.0)
    if not Q._static_per_tensor(q, 16):
        raise RuntimeError("DecodeEngine needs static per-tensor activation grids (set_scale_and_offset first)")
    s, o = q.scale.detach().float().contiguous(), q.offset.detach().float().contiguous()
    keep += [s, o]
    if isinstance(keep, _Keep):
        keep.sources.append((q, q.grid_token()))
    return MqGrid(s.data_ptr(), o.data_ptr(), float(q.qmin), float(q.qmax))


class _Keep(list):
    """Tensors the launch records point into, plus what they were derived from: (quantizer, grid_token) for every grid packed into a
    constants line and (weight, version) for every weight image, so that the engine can tell when the model moved under it."""

    def __init__(self):
        super().__init__()
        self.sources, self.weights = [], []

    def stale(self) -> bool:
        return any(q.grid_token() != t for q, t in self.sources) or any(Q._ver(w) != v for w, v in self.weights)


class _Linear:
    """Integer image of one or several QLinears that read the same activation grid: weights [N, K] int8 (index - 128) and the
    per-row epilogue vectors for that grid, concatenated (q|k|v) or row-interleaved (w1|w3)."""

    @staticmethod
    def _check(lin: Q.QLinear):
        """The conditions QLinear._int8_ready / the gated-MLP pass put on a linear before its integer path may stand in for the
        module: what they reject, the engine must not silently compute differently (qmodule.py:341-358 is the contract)."""
        wq, name = lin.weight_quantizer, type(lin).__name__
        if lin.int8_mode == "off":
            raise RuntimeError(f"DecodeEngine: {name}.int8_mode == 'off' asks for the simulated path")
        if wq is None or wq.bypassed() or wq.qcfg.bitwidth > 8 or wq.qcfg.is_dynamic or wq.lwc:
            raise RuntimeError("DecodeEngine: weight quantizers must be static, <= 8 bit and not in LWC mode (run the PTQ to its end first)")
        if lin.use_temporary_parameter or getattr(lin, "temp_weight", None) is not None:
            raise RuntimeError("DecodeEngine: fold the LET parameters first (smooth_lm_inplace): temp_weight / use_temporary_parameter is set")
        if lin.input_chan_scale is not None:
            raise RuntimeError("DecodeEngine: fold the run-time SmoothQuant channel scale into the weights first (smoothquant.smooth_lm)")
        for role in ("input_quantizer", "output_quantizer"):
            q = getattr(lin, role)
            if q is not None and not q.bypassed() and not Q._static_per_tensor(q, 16):
                raise RuntimeError(f"DecodeEngine: {role} must be a static per-tensor grid of at most 16 bits")

    def __init__(self, linears: List[Q.QLinear], a_grid: Q.Quantizer, interleave: bool = False):
        ws, alphas, zps, cts, biases = [], [], [], [], []
        for lin in linears:
            self._check(lin)
        bits = {lin.weight_quantizer.qcfg.bitwidth for lin in linears}
        if len(bits) != 1 or not bits <= {4, 8}:
            raise RuntimeError("DecodeEngine: the linears of one phase need the same 8- or 4-bit weight quantizer width")
        self.w4 = bits == {4}
        kinds = {_Linear.is_grouped(lin) for lin in linears}
        if len(kinds) != 1:
            raise RuntimeError("DecodeEngine: the linears of one phase mix per-group and per-channel weight grids (one launch contracts them "
                               "alike)")
        self.grouped = kinds == {True}
        self.group_size = None
        cat = (lambda ts: torch.stack(ts, dim=1).reshape(-1, *ts[0].shape[1:])) if interleave else (lambda ts: torch.cat(ts, dim=0))
        if self.grouped:
            self._init_grouped(linears, a_grid, cat)
            return
        for lin in linears:
            K = lin.weight.shape[1]
            if self.w4 and K % 64:
                raise RuntimeError("DecodeEngine: packed 4-bit weights need K % 64 == 0")
            plan = lin._epilogue_vectors(lin._weight_plan(lin.weight), a_grid, 128, K)
            ws.append(Q.QLinear._decode_weights(plan)[0]); alphas.append(plan["alpha"].clone()); zps.append(plan["w_zp"].clone()); cts.append(plan["col_term"].clone())
            biases.append(lin.bias.detach().float() if lin.bias is not None else None)
            plan["epi_key"] = None                      # the prefill path re-derives its vectors for its own grid object
        self.w = cat(ws).contiguous()
        self.alpha, self.w_zp, self.col_term = cat(alphas).contiguous(), cat(zps).contiguous(), cat(cts).contiguous()
        self._finish(linears, biases, cat)

    @staticmethod
    def is_grouped(lin: Q.QLinear) -> bool:
        qc = lin.weight_quantizer.qcfg
        return bool(qc.is_per_channel and qc.group_size != -1)

    def _init_grouped(self, linears: List[Q.QLinear], a_grid: Q.Quantizer, cat):
        """Per-group weight grids (mq_decode_gemv_grouped): the weight stream and the [G, N] vectors alpha / cw / t of the bracket
        P_g + cw A_g + t, from the quantities QLinear._grouped_plan and _forward_int8_grouped use at prefill (the same stored
        weights, cw = sh_w - o_w, t from the activation grid's c_a, alpha = s_a s_w).  Packed 4-bit rows carry unsigned nibbles
        (index - qmin), so their cw and t are taken in that domain.  Refuses where the prefill path would leave the integer kernel."""
        sizes = {int(lin.weight_quantizer.qcfg.group_size) for lin in linears}
        if len(sizes) != 1:
            raise RuntimeError(f"DecodeEngine: the linears of one phase mix group sizes {sorted(sizes)} (one launch folds one group size)")
        gs = sizes.pop()
        if not Q._static_per_tensor(a_grid, 8) or a_grid.qmin != 0 or a_grid.qmax != 255:
            raise RuntimeError("DecodeEngine: per-group weight grid: the input needs a static 8-bit unsigned per-tensor grid")
        s_a = a_grid.scale.detach().reshape(()).float()
        c_a = (128 - a_grid.offset.detach().reshape(())).round().to(torch.int64)
        ws, alphas, cws, ts, biases = [], [], [], [], []
        for lin in linears:
            N, K = lin.weight.shape
            if gs < 64 or gs & (gs - 1) or K % gs:
                raise RuntimeError(f"DecodeEngine: per-group weight grid: group_size {gs} with K {K} is outside the grouped decode launch "
                                   f"(a power of two >= 64 that divides K)")
            plan = lin._grouped_plan(lin.weight)
            if not plan["fold_ok"]:
                raise RuntimeError("DecodeEngine: per-group weight grid: a group's offset exceeds the kernel's 24-bit fold (narrow range far "
                                   "from zero)")
            wq, G = lin.weight_quantizer, plan["G"]
            q = plan["w"].view(N, K)                                   # stored weights: index - shift
            shift = 128 if wq.qmax > 127 else 0
            if self.w4:
                nib = (q.to(torch.int32) + (shift - int(wq.qmin))).to(torch.uint8)         # the unsigned nibble, 0 .. 15
                ws.append(ops.pack_w4(nib))
                wsum = nib.view(N, G, gs).sum(-1, dtype=torch.int64)
                cw = (int(wq.qmin) - wq.offset.detach().reshape(N, G)).round().to(torch.int64)
            else:
                ws.append(q)
                wsum = plan["wsum_t"].t().to(torch.int64)
                cw = plan["cw_t"].t().to(torch.int64)
            t64 = c_a * wsum + (gs * c_a) * cw
            cw_max = int(cw.abs().max())
            # the int32 bracket: |P_g| <= 128 * 128 gs, |cw A_g| <= cw_max 128 gs, |t|; the 24-bit multiply needs |cw| < 2^23.  One
            # host read per lowering (static grids): where it does not fit the prefill path's alpha turns NaN, here the engine refuses
            if cw_max >= 2 ** 23 or int(t64.abs().max()) + (cw_max + 128) * 128 * gs >= 2 ** 31:
                raise RuntimeError("DecodeEngine: per-group weight grid: the int32 bracket of the fold does not fit for this activation grid "
                                   "(an input grid far from zero)")
            ws[-1] = ws[-1].view(torch.int8)
            cws.append(cw.to(torch.int32))
            ts.append(t64.to(torch.int32))
            alphas.append(s_a * wq.scale.detach().reshape(N, G).float())
            biases.append(lin.bias.detach().float() if lin.bias is not None else None)
        self.group_size = gs
        self.w = cat(ws).contiguous()
        self.alpha = self.w_zp = self.col_term = None
        # [G, N] group-major, columns concatenated (q|k|v) or interleaved (w1|w3) as the rows of the stream
        self.g_alpha, self.g_cw, self.g_t = (cat(v).t().contiguous() for v in (alphas, cws, ts))
        self._finish(linears, biases, cat)

    def _finish(self, linears, biases, cat):
        self.bias = None
        if any(b is not None for b in biases):
            self.bias = cat([b if b is not None else torch.zeros(l.weight.shape[0], device=l.weight.device)
                             for b, l in zip(biases, linears)]).contiguous()
        self.N, self.K = self.w.shape[0], linears[0].weight.shape[1]
        self.rows = [l.weight.shape[0] for l in linears]
        self.sources = [(l.weight_quantizer, l.weight_quantizer.grid_token()) for l in linears]
        self.weights = [(l.weight, Q._ver(l.weight)) for l in linears]
        self._lins = list(linears)

    def byte_rows(self) -> torch.Tensor:
        """[N, K] int8, ONE byte per weight whatever the stream format: index - 128 of an 8-bit weight, the unsigned nibble of a 4-bit one
        (the numbers the packed kernels unpack: the same epilogue vectors apply)."""
        outs = []
        for lin in self._lins:
            plan = lin._weight_plan(lin.weight)
            if plan["bits4"] and plan["w4"]:                     # packed-only module (QLinear.w4_prefill = 'packed'): rebuild the nibbles
                wq = lin.weight_quantizer
                q, _ = ops.quantize(lin.weight.detach().float(), wq.scale.detach(), wq.offset.detach(), wq.qmin, wq.qmax, q_dtype=MQ_U8,
                                    shift=wq.qmin, rows=lin.weight.shape[0], want_row_sum=True)
                outs.append(q.view(torch.int8))
            else:
                outs.append(plan["w"].view(torch.int8).reshape(lin.weight.shape))
        return torch.cat(outs, dim=0).contiguous()


def _grouped_args(lin: _Linear, a: MqDecodeGemvArgs, batch: int, x_stride: int, y_stride: int, gate_stride: int) -> MqDecodeGemvGroupedArgs:
    """mq_decode_gemv_grouped's argument block: the batched launch's block around `a` plus the group size and the [G, N] vectors."""
    b = MqDecodeGemvBatchArgs()
    b.g, b.batch, b.x_stride, b.y_stride, b.gate_stride = a, batch, x_stride, y_stride, gate_stride
    ga = MqDecodeGemvGroupedArgs()
    ga.b, ga.group_size = b, lin.group_size
    ga.alpha, ga.cw, ga.t = lin.g_alpha.data_ptr(), lin.g_cw.data_ptr(), lin.g_t.data_ptr()
    ga._mq_bytes = a._mq_bytes + 12 * lin.g_alpha.numel()          # + alpha / cw / t, 4 bytes each per group and row
    return ga


def spec_accept(argmax_rows: Sequence[int], proposals: Sequence[int], eos=(), budget: Optional[int] = None,
                room: Optional[int] = None) -> Tuple[List[int], int, bool]:
    """Bookkeeping of one greedy speculative round (DecodeEngine.generate with a draft), host only.  The target ran the rows
    [t, d1 .. dk] (t: the last token, not yet cached; d: the proposals); argmax_rows[i] is row i's greedy token, i.e. plain greedy's token
    after t, d1 .. di.  Tokens are taken in order: row i's token is kept; it continues the round only while it equals d(i+1) (accepted).
    The first disagreeing row or the bonus row k ends the round with its own token.  The round also ends at an EOS token, once `budget`
    tokens are kept (new tokens still allowed) or once `room` are (cache positions left behind the last cached one: the position plain
    generate would stop at).  Returns (kept tokens, accepted proposals among them, stop).  The kept tokens are plain greedy's next
    tokens, and the target's cache is valid for exactly len(kept) positions from t's on."""
    eos = set(eos or ())
    k = len(proposals)
    if len(argmax_rows) < k + 1:
        raise ValueError(f"spec_accept: {len(argmax_rows)} rows for {k} proposals (needs k + 1)")
    out, acc = [], 0
    for i, g in enumerate(argmax_rows[:k + 1]):
        g = int(g)
        out.append(g)
        hit = i < k and g == int(proposals[i])
        acc += int(hit)
        if g in eos or (budget is not None and len(out) >= budget) or (room is not None and len(out) >= room):
            return out, acc, True
        if not hit:
            break
    return out, acc, False


def prompt_lookup_draft(ngram: int = 3) -> Callable[[List[int], int], List[int]]:
    """A draft without a model (prompt lookup): draft(ids, k) proposes up to k tokens that followed the latest EARLIER occurrence of
    the last `ngram` tokens of ids, or none."""
    n = int(ngram)
    if n < 1:
        raise ValueError(f"prompt_lookup_draft: ngram={ngram} must be >= 1")

    def draft(ids: List[int], k: int) -> List[int]:
        if k <= 0 or len(ids) <= n:
            return []
        tail = list(ids[-n:])
        for i in range(len(ids) - n - 1, -1, -1):
            if list(ids[i:i + n]) == tail:
                return [int(t) for t in ids[i + n:i + n + k]]
        return []
    return draft


class RowPlan(NamedTuple):
    """A ragged step as the launches read it (plan_rows): row r is token row_tok[r] of slot row_seq[r] at position row_pos[r]; spans[slot]
    = (first row, row count) of the slot's run."""
    row_seq: List[int]
    row_pos: List[int]
    row_tok: List[int]
    spans: Dict[int, Tuple[int, int]]


def plan_rows(tokens: Mapping[int, Sequence[int]], positions: Sequence[Optional[int]], max_rows: int, cache_len: int,
              who: str = "BatchDecodeEngine.step_tokens") -> RowPlan:
    """The row table of one ragged step (BatchDecodeEngine.step_tokens), host only.  tokens: slot -> its tokens; positions[slot]: the
    slot's cached positions, None for an idle slot.  Rows are laid out in ascending slot order, a slot's rows contiguous at consecutive
    positions from its own: each slot is ONE run of mq_decode_attention_ragged, which is what that launch asks of its caller.
    ValueError: a slot outside 0 .. len(positions) - 1, an empty token list, a total outside 1 .. max_rows.  RuntimeError: an idle
    slot, or tokens that would overflow the slot's cache."""
    B = len(positions)
    plan = {}
    for slot, toks in tokens.items():
        if isinstance(slot, bool) or int(slot) != slot or not 0 <= int(slot) < B:
            raise ValueError(f"{who}: slot {slot!r} outside 0..{B - 1}")
        if int(slot) in plan:
            raise ValueError(f"{who}: slot {int(slot)} is named twice")
        plan[int(slot)] = [int(v) for v in toks]
        if not plan[int(slot)]:
            raise ValueError(f"{who}: slot {int(slot)} has no tokens (leave a slot that does not move out of the mapping)")
    total = sum(len(t) for t in plan.values())
    if not 1 <= total <= max_rows:
        raise ValueError(f"{who}: {total} rows outside 1..{max_rows} (max_rows)")
    out = RowPlan([], [], [], {})
    for slot in sorted(plan):
        t, P = plan[slot], positions[slot]
        if P is None:
            raise RuntimeError(f"{who}: slot {slot} is idle (prefill() or start() it first)")
        if P + len(t) > cache_len:
            raise RuntimeError(f"{who}: {len(t)} tokens at position {P} overflow slot {slot}'s KV cache ({cache_len} positions)")
        out.spans[slot] = (len(out.row_tok), len(t))
        out.row_seq.extend([slot] * len(t))
        out.row_pos.extend(range(P, P + len(t)))
        out.row_tok.extend(t)
    return out


def spec_row_budget(num_draft: int, max_rows: int, allowed: Sequence[int], room: Sequence[int]) -> List[int]:
    """Proposals per live slot of one batched speculative round (BatchDecodeEngine.generate with a draft), host only.  The L = len(allowed)
    live slots share the step's max_rows rows evenly, one of each share being the slot's last token: k_i = min(num_draft, max_rows // L
    - 1, allowed[i] - 1, room[i] - 1), at least 0, where allowed[i] is the new tokens slot i may still return and room[i] the cache
    positions behind its last cached one (spec_accept's budget and room).  With max_rows // L <= 1 (eight live slots of eight rows)
    every k_i is 0: plain steps.  While L <= max_rows the rows L + sum(k) never exceed max_rows."""
    L = len(allowed)
    if len(room) != L:
        raise ValueError(f"spec_row_budget: {L} budgets for {len(room)} cache rooms")
    if int(num_draft) < 0:
        raise ValueError(f"spec_row_budget: num_draft={num_draft} must be >= 0")
    return [max(0, min(int(num_draft), int(max_rows) // L - 1, int(a) - 1, int(r) - 1)) for a, r in zip(allowed, room)]


def _spec_stats() -> Dict[str, int]:
    """self.spec_stats of a speculative generation: rows steps of the target (rounds, target_steps), tokens proposed and accepted."""
    return {"rounds": 0, "proposed": 0, "accepted": 0, "target_steps": 0}


def _eos_set(eos_token_id) -> set:
    """generate's eos_token_id (None, one id or several) as a set."""
    return set([eos_token_id] if isinstance(eos_token_id, int) else (eos_token_id or []))


def _check_draft(who: str, target, draft, num_draft, engine: tuple, what: str = "a DecodeEngine or a callable draft(ids, k) -> list of token ids"):
    """The refusals every speculative entry point shares, before anything runs: the draft is another engine (an instance of the
    classes `engine`; none: no engine may draft) of the target's vocabulary size or a callable, and num_draft >= 0.  Returns the
    draft engine, or None for a callable."""
    d_eng = draft if isinstance(draft, engine) else None
    if d_eng is target:
        raise ValueError(f"{who}: the draft must be another engine (it keeps its own cache)")
    if d_eng is None and not callable(draft):
        raise TypeError(f"{who}: draft must be {what}")
    if isinstance(num_draft, bool) or int(num_draft) < 0:
        raise ValueError(f"{who}: num_draft={num_draft} must be >= 0")
    if d_eng is not None and d_eng.shape.vocab != target.shape.vocab:
        raise ValueError(f"{who}: draft vocabulary {d_eng.shape.vocab} != target vocabulary {target.shape.vocab}")
    return d_eng


class _Greedy:
    """How DecodeEngine._speculate chooses tokens, on the target and on an engine draft alike.  This one is plain generate's
    torch.argmax (ties break as they do there)."""
    draft_room = 1                       # an engine draft reads its last proposal from its logits: kd <= cache_len - len(out) + 1

    def start(self, eng, ids, prefill):
        eng._start_sequence(ids, prefill)

    def first(self, eng) -> int:
        """The token behind eng's cached sequence, from eng.logits."""
        return int(torch.argmax(eng.logits))

    def chain(self, eng, n: int) -> List[int]:
        """n tokens behind eng's cached sequence, each stepped before the next is chosen; the last one is not cached."""
        toks = [self.first(eng)]
        for _ in range(n - 1):
            eng.step(toks[-1])
            toks.append(self.first(eng))
        return toks

    def rows(self, eng, tokens) -> List[int]:
        """ONE rows step of eng over `tokens`: the token behind every row."""
        return torch.argmax(eng.step_tokens(tokens), dim=-1).tolist()

    def recount(self, eng, dropped, kept):
        pass


class _Sampled:
    """_Greedy's counterpart for generate(sampling=...): the selection under one request and stream: sample() / sample_step() and, behind a rows step,
    mq_sample_rows (one graph after capture(), ONE read-back of the T tokens).  An engine draft shares the noise with the target.
    Under a penalised request start() rebuilds eng's history from the context and every launch counts what it draws; recount() brings
    the history back to the sequence's truth: -1 for drawn tokens that were dropped, +1 for kept ones no launch has counted."""
    draft_room = 0                       # (its last draw, at index len(out) + kd - 1, must not be an idle row)

    def __init__(self, sampling, stream):
        self.request = (sampling, stream)

    def start(self, eng, ids, prefill):
        eng.set_sampling(*self.request)
        eng._start_sequence(ids, prefill)
        if eng._sampler.penalized:
            eng._sampler.observe_prompt(0, ids)                    # the history is rebuilt for every sequence

    def first(self, eng) -> int:
        eng.sample()
        return int(eng.tok.item())

    def chain(self, eng, n: int) -> List[int]:
        buf = torch.empty(n, dtype=torch.int64, device=eng.tok.device)
        for i in range(n):                                         # token i at index position() + i, counted in eng's own history
            (eng.sample_step if i < n - 1 else eng.sample)()
            buf[i:i + 1].copy_(eng.tok)
        return buf.tolist()

    def rows(self, eng, tokens) -> List[int]:
        return eng.step_sample_tokens(tokens).tolist()

    def recount(self, eng, dropped, kept):
        if eng._sampler.penalized:
            for ids, delta in ((dropped, -1), (kept, 1)):
                if ids:
                    history_count(eng._sampler.history[0], torch.tensor(ids, dtype=torch.int64, device=eng.dev), delta)


class _CallableDraft:
    """A draft of DecodeEngine._speculate: propose(out, k) -> at most k tokens to follow out; settle(out, new, acc, props) once the
    target kept `new` behind out, `acc` of them from `props`.  This one is draft(ids, k), which keeps nothing."""

    def __init__(self, fn):
        self.fn = fn

    def start(self, ids, prefill):
        pass

    def propose(self, out, k):
        return [int(v) for v in self.fn(list(out), k)][:k]

    def settle(self, out, new, acc, props):
        pass


class _EngineDraft:
    """Another DecodeEngine drafting by the target's own selection.  Its cache holds out[:pos]: propose catches up on the kept tokens
    with extend, settle drops the rejected proposals with rewind (and from a penalised history)."""

    def __init__(self, eng, select):
        self.eng, self.select, self.pos = eng, select, 0

    def start(self, ids, prefill):
        self.select.start(self.eng, ids, prefill)
        self.pos = len(ids)

    def propose(self, out, k):
        kd = min(k, self.eng.cache_len - len(out) + self.select.draft_room)
        if kd <= 0:
            return []
        self.eng.extend(out[self.pos:])                            # its logits: behind out, the row token len(out) is chosen from
        self.pos = len(out) + kd - 1                               # out + props[:-1]
        return self.select.chain(self.eng, kd)

    def settle(self, out, new, acc, props):
        self.select.recount(self.eng, props[acc:], new[acc:])
        if self.pos > len(out):                                    # the draft keeps out + the accepted proposals it had cached
            self.pos = min(self.pos, len(out) + acc)
            self.eng.rewind(self.pos)


class _Images(NamedTuple):
    """One decoder layer as every chain over it reads it: the record fields of its two fused norms (_norm_args), o_proj's input grid and
    the weight images (o_w: o_proj once more, sliced by head for the four-launch attention launch, else None).  Built and validated once
    per layer and lowering (_layer_images)."""
    layer: torch.nn.Module
    norm1: dict
    qkv: _Linear
    g_o: Q.Quantizer
    op: _Linear
    o_w: Optional[torch.Tensor]
    norm2: dict
    w13: _Linear
    w2: _Linear


class _Target(NamedTuple):
    """Where a layer's chain reads and writes: data, not the engine that asks.  rows None: one row, bare records; else every record is
    wrapped for `rows` rows of these buffers (mq_decode_gemv_batch / _grouped).  attn: how the attention record is wrapped -- None
    (bare), "batch" (a sequence per row, mq_decode_attention_batch), "multi" (consecutive positions of one sequence,
    mq_decode_attention_multi; v_chunked: the four-launch value layout) or "ragged" (row r the position row_pos[r] of sequence
    row_seq[r] of the `batch` sequences in the caches, mq_decode_attention_ragged)."""
    x: torch.Tensor
    qkv: torch.Tensor
    attn_q: torch.Tensor
    attn_part: torch.Tensor
    attn_ticket: torch.Tensor
    gate_q: torch.Tensor
    k_cache: List[torch.Tensor]
    v_cache: List[torch.Tensor]
    nsplit: int
    rows: Optional[int] = None
    attn: Optional[str] = None
    v_chunked: bool = False
    batch: Optional[int] = None
    row_seq: Optional[torch.Tensor] = None
    row_pos: Optional[torch.Tensor] = None


class _Chain(NamedTuple):
    """One layer's (kind, record) launches by role, in launch order; o_proj is None where the attention launch contracts it (four launches)."""
    qkv: tuple
    attn: tuple
    o_proj: Optional[tuple]
    gate: tuple
    w2: tuple


class _DecodeBase:
    """What DecodeEngine and BatchDecodeEngine both are: snapshots of one model (_lower_model), the lowering of a decoder layer to launch
    records on a _Target (_lower_chain and its per-launch helpers), the hipGraph recorder (_record), the rows step behind step_tokens
    (_lower_row_chain, _set_rows, _launch_rows) and, written over ONE sequence, prefill (_prefill_fill, _prefill_append) and a
    sequence's share of a speculative round (_spec_keep).  The engine supplies model / shape / dev / cache_len / cos / sin / pos / graph
    / max_rows, _lower() and capture(), its _lower_rows / _finish_rows / _capture_rows and, for the code over one sequence, position /
    set_position / rewind plus _seq_caches / _store_values / _step_seq / _logits_row.  Those take the sequence as trailing arguments
    `*seq`: nothing in DecodeEngine, the slot in BatchDecodeEngine."""

    LONG_FROM, LONG_SPLITS = 768, 4      # five launches: the split attention launch from LONG_FROM cached positions on
    # mq_decode_gemv_batch / mq_decode_head_batch limits: rows * K int8 images in the GEMV launches' LDS, rows * hidden normalised floats in the head's
    MAX_IMAGE_BYTES, MAX_HEAD_FLOATS = 128 * 1024, 32768

    def _lower_model(self):
        """What every lowering starts from, built from the model as it is now: weight images, epilogue vectors and one constants line per
        launch (_pack) are SNAPSHOTS of the quantizers -- the kernels do not read through the module's scale / offset tensors."""
        model, s = self.model, self.shape
        self._keep = _Keep()
        self.phases = []          # (kind, ctypes struct) in launch order
        # embedding table, final norm and lm_head (fp32, unquantised: qmodule.py:843) are snapshots like every weight image: re-derived
        # here and tracked for grids_stale()
        self.embed = model.embed_tokens.weight.detach()
        if s.embed_scale:                                    # normalize_embed (Gemma; hf_model.py:1555-1556): x = embed * hidden ** 0.5
            self.embed = self.embed * (s.hidden ** 0.5)      # the same fp32 product the module graph forms per token
        self.norm_ln = isinstance(model.norm, torch.nn.LayerNorm)
        self.norm_w = model.norm.weight.detach().float().contiguous()
        self.norm_b = model.norm.bias.detach().float().contiguous() if getattr(model.norm, "bias", None) is not None else None
        self.lm_w = model.lm_head.weight.detach().float().contiguous()
        self.lm_b = model.lm_head.bias.detach().float().contiguous() if model.lm_head.bias is not None else None
        for w in (model.embed_tokens.weight, model.norm.weight, getattr(model.norm, "bias", None), model.lm_head.weight, model.lm_head.bias):
            if w is not None:
                self._keep.weights.append((w, Q._ver(w)))
        for q in model.modules():                 # grids set from act_dict.json sit on the host until a forward moves them
            if isinstance(q, Q.Quantizer) and q._has_grid() and q.scale.device != self.dev:
                q.scale.data, q.offset.data = q.scale.to(self.dev), q.offset.to(self.dev)
        self._images = []         # per layer, filled as the engine lowers it (_layer_images); the T-row chain reuses them (_lower_rows)

    @property
    def weight_bytes(self) -> int:
        return sum(p[1]._mq_bytes for p in self.phases if hasattr(p[1], "_mq_bytes"))

    @property
    def head_bytes(self) -> int:
        return self.lm_w.numel() * 4

    def grids_stale(self) -> bool:
        """True when a quantizer grid or a weight the engine snapshotted has been changed since (in place or replaced)."""
        return self._keep.stale()

    def refresh_grids(self):
        """Re-derive every weight image, epilogue vector and constants line from the model's current quantizers and re-record the
        graph(s) if there were any.  The cached keys / values stay as they are: they are indices on the OLD qk_bmm / pv_bmm input
        grids, so after a recalibration start the sequence again (reset() / prefill())."""
        had_graph = self.graph is not None
        self.graph = None
        self._lower()
        if had_graph:
            self.capture()
        return self

    def _sync_grids(self):
        # checked where a sequence starts (capture / reset / prefill), not per step(): a token is 0.65 ms, the walk over ~500 grids
        # is about as long.  A grid changed in the middle of a sequence is the caller's to announce with refresh_grids().
        if self._keep.stale():
            self.refresh_grids()

    # -- continuing a live sequence with a prefill forward over its cache -----------------------------------------
    # prefill(append=True) steps fewer tokens than this behind the 64-boundary instead of importing the cache for them.  NOT MEASURED
    # yet: 16 is a placeholder until tools/bench_append.py has been run on the device (the crossover against extend(), rounded up to
    # a multiple of 8, belongs here).
    APPEND_MIN_TOKENS = 16

    def _append_split(self, P: int, n: int) -> Tuple[int, Optional[str]]:
        """How an append of n tokens at position P is served: (tokens to step first, reason).  The first (-P) % 64 tokens are stepped
        to the next multiple of 64 -- the only positions the chunk-continuing attention starts at -- and the rest goes through the
        model's chunked forward, unless too few remain or the model's attention cannot continue an image cache: then every token is
        stepped and `reason` says why."""
        from .llama import image_cache_unsupported
        head = min((-P) % 64, n)
        rest = n - head
        if rest < max(2, self.APPEND_MIN_TOKENS):
            return n, (None if rest == 0 else f"{rest} token(s) behind position {P + head}: fewer than APPEND_MIN_TOKENS = {max(2, self.APPEND_MIN_TOKENS)}")
        why = image_cache_unsupported(self.model)
        if why is not None:
            return n, why
        return head, None

    def _append_chunk(self, chunk: Sequence[int], P1: int, caches, v_chunked: bool) -> Optional[torch.Tensor]:
        """The fused part of an append: per layer import positions [0, P1) of caches(li) = (k, v) into that layer's ImageCache
        (allocated on first use and kept: cache_len rounded up to 64 rows), run the model's chunked forward at pos = P1 and export
        rows [P1, P1 + len(chunk)) back.  Returns the logits row of the last token, or None when the model refused the image cache
        after all (nothing of the engine has been written then)."""
        from . import ops
        from .llama import _f16_scores_ok
        if getattr(self, "_append_images", None) is None:
            self._append_images = self.model.new_image_cache(1, self.cache_len, device=self.dev)
        images = self._append_images
        for li, layer in enumerate(self.model.layers):
            qk = layer.self_attn.qk_bmm
            grids = {name: (q.scale.detach(), q.offset.detach(), q.qmin, q.qmax) for name, q in (("qk_a", qk.input_quantizer), ("qk_b", qk.input2_quantizer))}
            k, v = caches(li)
            ops.attention_cache_import(images[li].per_sequence[0], k, v, P1, grids, v_chunked=v_chunked, k_f16_exact=_f16_scores_ok(qk.input2_quantizer))
            images[li].filled = P1
        ids = torch.as_tensor([int(t) for t in chunk], dtype=torch.long, device=self.dev).view(1, -1)
        try:
            logits = self.model(ids, cache=images, pos=P1, last_logits_only=True)
        except RuntimeError as e:
            if "image cache" not in str(e):
                raise
            return None
        for li in range(len(self.model.layers)):
            k, v = caches(li)
            ops.attention_cache_export(images[li].per_sequence[0], k, v, P1, len(chunk), v_chunked=v_chunked)
        return logits[0, -1]

    v_transposed = False                 # the value layout _append_chunk finds in _seq_caches (DecodeEngine's four-launch chain: chunked)

    @torch.no_grad()
    def _prefill_append(self, context_ids, *seq) -> torch.Tensor:
        """prefill(append=True) for the sequence `seq` (DecodeEngine.prefill has the contract)."""
        me, t = type(self).__name__, [int(v) for v in context_ids]
        P = self.position(*seq)
        if not t:
            raise ValueError(f"{me}.prefill: no tokens to append")
        if P + len(t) > self.cache_len:
            where = f"slot {seq[0]}'s KV cache" if seq else "the KV cache"
            raise RuntimeError(f"{me}.prefill: {len(t)} tokens appended at position {P} overflow {where} ({self.cache_len} positions)")
        if P == 0:
            self.append_stats = {"stepped": 0, "prefilled": len(t), "reason": None}
            return self.prefill(*seq, t)
        self._sync_grids()
        head, reason = self._append_split(P, len(t))
        if head:
            self._step_seq(t[:head], *seq)
        if head < len(t):
            row = self._append_chunk(t[head:], P + head, lambda li: self._seq_caches(li, *seq), self.v_transposed)
            if row is None:
                reason = "the model's attention refused the image cache"
                self._step_seq(t[head:], *seq)
                head = len(t)
            else:
                self.set_position(*seq, P + len(t))
                self._logits_row(*seq).copy_(row)
        self.append_stats = {"stepped": head, "prefilled": len(t) - head, "reason": reason}
        return self._logits_row(*seq)

    @torch.no_grad()
    def _prefill_fill(self, context_ids, zero: bool, *seq) -> torch.Tensor:
        """Context encoding for the sequence `seq` in ONE forward of the module graph with a KV cache attached: the cached keys /
        values go on their QMatMul input grids into the sequence's caches (zero: cleared first), its position behind the context, the
        last position's logits into its row."""
        ids = torch.as_tensor([int(t) for t in context_ids], dtype=torch.long, device=self.dev).view(1, -1)
        S = ids.shape[1]
        assert 0 < S <= self.cache_len
        self._sync_grids()
        raw = self.model.new_cache(1, S, device=self.dev)
        logits = self.model(ids, cache=raw, last_logits_only=True)      # [1, 1, vocab]: only the last position feeds the first new token
        for li, layer in enumerate(self.model.layers):
            att, (k, v) = layer.self_attn, self._seq_caches(li, *seq)
            if zero:
                k.zero_()
                v.zero_()
            k[:, :S] = att.qk_bmm.input2_quantizer.quantize_to_int(raw[li][0][0].contiguous())[0]
            self._store_values(li, att.pv_bmm.input2_quantizer.quantize_to_int(raw[li][1][0].contiguous())[0], *seq)
        self.set_position(*seq, S)
        return self._logits_row(*seq).copy_(logits[0, -1])

    # -- per-token log-probabilities behind the selection launches (csrc/mq_logprob.hip) --------------------------
    _lp = None                           # the LogprobLaunch behind every selection launch while the switch is on (set_logprobs)

    def set_logprobs(self, n_top: Optional[int]):
        """The switch: from now on every selection launch -- sample(), sample_step(), sample_rows(), step_sample_tokens() -- is followed
        on the same stream by mq_logprob_top over the same RAW logits and the token just written, before the step that overwrites
        the logits; after capture() inside the same graph (a graph with the launch is recorded on first use beside the one without,
        which is kept).  n_top in 0 .. 20: that many alternatives per token; None: off, today's launches and graphs.  The record
        buffers [sequences, cache_len] are allocated on the first request of each n_top and kept (a few bytes per position and
        alternative; the launches' scratch is one buffer for all of them).  generate(..., logprobs=n) sets the switch for its own run
        and puts it back as it found it; generate without logprobs= leaves it alone.  A record is written at its own
        (sequence, token index): a speculative round's rejected rows are overwritten when their index is drawn again, and
        release() / reset() need not clear anything -- read only the indices that were drawn (logprob_records)."""
        n = check_logprobs(type(self).__name__ + ".set_logprobs", n_top, True)
        if n is None:
            self._lp = None
        else:
            lp = self._lp_launches.get(n)
            if lp is None:
                shared = next(iter(self._lp_launches.values())).scratch if self._lp_launches else None
                lp = self._lp_launches[n] = LogprobLaunch(self.logits, self.pos, self.tok, self.cache_len, n, scratch=shared)
            self._lp = lp
        return self

    @contextlib.contextmanager
    def _logprobs_for(self, n_top: Optional[int]):
        """generate(logprobs=n_top): the switch set for this run and put back afterwards; None leaves it as it is."""
        before = self._lp
        if n_top is not None:
            self.set_logprobs(n_top)
        try:
            yield
        finally:
            self._lp = before

    def _lp_key(self, *key):
        """A sample graph's key: with the switch on, one more component (n_top); off, the key as it always was."""
        return key + (self._lp.n_top,) if self._lp is not None else (key if len(key) > 1 else key[0])

    def _select(self):
        """The selection launch of sample(): mq_sample / mq_sample_penalized and, with the switch on, mq_logprob_top behind it."""
        self._sampler.launch()
        if self._lp is not None:
            self._lp.launch()

    def _records(self, seq: int, start: int, stop: int) -> TokenLogprobs:
        if self._lp is None:
            raise RuntimeError(f"{type(self).__name__}.logprob_records: no records are kept (set_logprobs(n_top) first)")
        return self._lp.records(seq, int(start), int(stop))

    def _record(self, launch, append, before_capture=None):
        """launch() followed by append() as ONE hipGraph on one stream.  launch() first runs once on a side stream outside the capture:
        it sets the launches' LDS ceilings, which must not happen while capturing.  What that warm-up may touch (pos parked at the
        cache_len sentinel or not, tickets, tok) and what is restored afterwards is the caller's; before_capture() runs between the
        warm-up and the capture."""
        with torch.cuda.device(self.dev):
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                launch()
            torch.cuda.current_stream().wait_stream(side)
            if before_capture is not None:
                before_capture()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                launch()
                append()
        return g

    # -- lowering ----------------------------------------------------------------------------------------------------------
    def _norm_args(self, norm) -> Tuple[dict, Q.Quantizer]:
        """QRMSNorm (qmodule.py:469-530) or QLayerNorm (qmodule.py:579-640; StableLM-2) fused in front of a weight stream: the GEMV record's
        norm fields and the grid the stream's input sits on."""
        me = type(self).__name__
        ln = isinstance(norm, Q.QLayerNorm)
        if ln:
            if norm.use_temporary_parameter or norm.weight is None:
                raise RuntimeError(f"{me}: QLayerNorm needs its affine weight and no temporary (LET) parameters")
        elif not isinstance(norm, Q.QRMSNorm) or norm.l2norm_as_rmsnorm or norm.bias is not None:
            raise RuntimeError(f"{me}: QRMSNorm (plain RMS form, no bias) or QLayerNorm layers only")
        wfq = Q._apply(norm.weight_quantizer, norm.weight.detach()).float().contiguous()
        self._keep.append(wfq)
        self._keep.weights.append((norm.weight, Q._ver(norm.weight)))
        if norm.weight_quantizer is not None and norm.weight_quantizer._has_grid():
            self._keep.sources.append((norm.weight_quantizer, norm.weight_quantizer.grid_token()))
        f = dict(norm_w=wfq.data_ptr(), norm_in=_grid(norm.input_quantizer, self._keep), eps=float(norm.eps), layernorm=int(ln))
        if ln and norm.bias is not None:
            nb = norm.bias.detach().float().contiguous()
            self._keep.append(nb)
            f["norm_bias"] = nb.data_ptr()
        f["a_grid"] = _grid(norm.output_quantizer, self._keep)
        if norm.output_quantizer is None or norm.output_quantizer.qmax != 255:
            raise RuntimeError(f"{me}: the norm feeding a linear needs an 8-bit unsigned output grid")
        return f, norm.output_quantizer

    def _layer_images(self, layer, head_sliced: bool = False) -> _Images:
        """The layer's norms and weight images, with every check the chains rely on; appended to self._images."""
        me, s = type(self).__name__, self.shape
        attn, mlp = layer.self_attn, layer.mlp
        for m in (attn.q_proj, attn.k_proj, attn.v_proj, attn.o_proj, mlp.w1, mlp.w2, mlp.w3):
            if not isinstance(m, Q.QLinear):
                raise RuntimeError(f"{me}: run create_sim_qmodel first")
        norm1, g_in = self._norm_args(layer.input_layernorm)
        qkv = _Linear([attn.q_proj, attn.k_proj, attn.v_proj], g_in)
        # o_proj's input sits on pv_bmm's output grid (the live producer), else on its declared / own grid: the attention launch
        # writes pv_bmm's output straight as o_proj's int8 image on that grid
        pv_out = attn.pv_bmm.output_quantizer
        g_o = attn.o_proj.input_quantizer if attn.o_proj.input_quantizer is not None else (
            pv_out if Q._static_per_tensor(pv_out, 8) else attn.o_proj._input_grid)
        if g_o is None or g_o.qmax != 255:
            raise RuntimeError(f"{me}: o_proj needs an 8-bit unsigned input grid (pv_bmm output)")
        op = _Linear([attn.o_proj], g_o)
        if op.K != s.heads * s.head_dim or op.N != s.hidden:
            raise RuntimeError(f"{me}: o_proj must map heads * head_dim -> hidden")
        # [heads][N][D]: a head's K-slice of every row, one byte per weight whatever the stream format
        o_w = op.byte_rows().view(op.N, s.heads, s.head_dim).permute(1, 0, 2).contiguous() if head_sliced else None
        norm2, g_ffn = self._norm_args(layer.post_attention_layernorm)
        w13 = _Linear([mlp.w1, mlp.w3], g_ffn, interleave=True)
        act = mlp.act_fn
        if not isinstance(act, (Q.QSiLU, Q.QGELU)) or (act.input_quantizer is not None and not act.input_quantizer.bypassed()):
            raise RuntimeError(f"{me}: act_fn must be QSiLU / QGELU without an input quantizer (the reference's surgery)")
        iq2 = mlp.w2.input_quantizer
        if iq2 is None or iq2.qmax != 255:
            raise RuntimeError(f"{me}: w2 needs its own 8-bit unsigned input quantizer")
        self._images.append(_Images(layer, norm1, qkv, g_o, op, o_w, norm2, w13, _Linear([mlp.w2], iq2)))
        return self._images[-1]

    def _gemv(self, lin: _Linear, **fields) -> MqDecodeGemvArgs:
        a = MqDecodeGemvArgs()
        a.K, a.N = lin.K, lin.N
        a.w = lin.w.data_ptr()
        if not lin.grouped:                                  # (grouped: the [G, N] vectors travel in _grouped_args' block)
            a.alpha, a.w_zp, a.col_term = lin.alpha.data_ptr(), lin.w_zp.data_ptr(), lin.col_term.data_ptr()
        a.bias = lin.bias.data_ptr() if lin.bias is not None else None
        a.seg_end[0] = a.seg_end[1] = lin.N
        for k, v in fields.items():
            setattr(a, k, v)
        a.w4 = int(lin.w4)
        a._mq_bytes = lin.N * lin.K // (2 if lin.w4 else 1)
        self._keep.append(lin)
        self._keep.sources += lin.sources
        self._keep.weights += lin.weights
        return a

    def _pack(self, grids) -> int:
        """mq_decode_pack_grids: the launch's static grids -> one constants line on the device (no host read-back)."""
        arr = (MqGrid * len(grids))(*grids)
        out = torch.zeros(64, device=self.dev)                 # one 256-byte line: every wave reads all 64 floats
        _lib.call("mq_decode_pack_grids", arr, len(grids), out.data_ptr(), torch.cuda.current_stream(self.dev).cuda_stream)
        self._keep.append(out)
        return out.data_ptr()

    def _finish_gemv(self, t: _Target, lin: _Linear, a: MqDecodeGemvArgs, x_stride: int, y_stride: int, gate_stride: int = 0):
        """Pack the record's constants line and wrap it for the target: (kind, launch record).  One row: mq_decode_gemv, or
        mq_decode_gemv_grouped at batch 1 for per-group weight grids; t.rows rows: mq_decode_gemv_batch / _grouped with the row strides."""
        a.consts = self._pack([a.norm_in, a.a_grid, a.out_grid[0], a.out_grid[1], a.out_grid[2], a.gate_mid, a.gate_actout, a.gate_out, a.o_out])
        if lin.grouped:
            return "gemv_grouped", (_grouped_args(lin, a, 1, 0, 0, 0) if t.rows is None else
                                    _grouped_args(lin, a, t.rows, x_stride, y_stride, gate_stride))
        if t.rows is None:
            return "gemv", a
        b = MqDecodeGemvBatchArgs()
        b.g, b.batch, b.x_stride, b.y_stride, b.gate_stride = a, t.rows, x_stride, y_stride, gate_stride
        b._mq_bytes = a._mq_bytes
        return "gemv", b

    def _attention_grids(self, attn, at, g_o):
        keep = self._keep
        qk, pv = attn.qk_bmm, attn.pv_bmm
        at.qk_a, at.qk_b, at.qk_out = (_grid(q, keep) for q in (qk.input_quantizer, qk.input2_quantizer, qk.output_quantizer))
        at.pv_a, at.pv_b, at.pv_out = (_grid(q, keep) for q in (pv.input_quantizer, pv.input2_quantizer, pv.output_quantizer))
        at.o_in = _grid(g_o, keep)
        at.consts = self._pack([at.qk_a, at.qk_b, at.qk_out, at.pv_a, at.pv_b, at.pv_out, at.o_in])

    def _qkv_launch(self, im: _Images, t: _Target, **extra):
        """input_layernorm + q|k|v stream."""
        attn = im.layer.self_attn
        p = self._gemv(im.qkv, **im.norm1, x=t.x.data_ptr(), y=t.qkv.data_ptr(), **extra)
        p.seg_end[0], p.seg_end[1] = im.qkv.rows[0], im.qkv.rows[0] + im.qkv.rows[1]
        for k, lin in enumerate((attn.q_proj, attn.k_proj, attn.v_proj)):
            p.out_grid[k] = _grid(lin.output_quantizer, self._keep)
        return self._finish_gemv(t, im.qkv, p, self.shape.hidden, t.qkv.shape[-1])

    def _attn_launches(self, li: int, im: _Images, t: _Target):
        """RoPE / cache append / attention core into o_proj's int8 image, then o_proj + residual from that image."""
        s, attn, qkv_n = self.shape, im.layer.self_attn, t.qkv.shape[-1]
        at = MqDecodeAttentionArgs()
        at.qkv, at.k_cache, at.v_cache = t.qkv.data_ptr(), t.k_cache[li].data_ptr(), t.v_cache[li].data_ptr()
        at.cos, at.sin, at.pos = self.cos.data_ptr(), self.sin.data_ptr(), self.pos.data_ptr()
        at.heads, at.kv_heads, at.head_dim, at.cache_len = s.heads, s.kv_heads, s.head_dim, self.cache_len
        at.rot_dim, at.nsplit = self.cos.shape[1], t.nsplit
        self._attention_grids(attn, at, im.g_o)
        at.out_q, at.part, at.ticket = t.attn_q.data_ptr(), t.attn_part.data_ptr(), t.attn_ticket.data_ptr()
        if t.attn == "batch":
            w = MqDecodeAttentionBatchArgs()
            w.a, w.batch, w.split_from, w.qkv_stride = at, t.rows, self.LONG_FROM, qkv_n
        elif t.attn == "multi":
            w = MqDecodeAttentionMultiArgs()
            w.a, w.rows, w.split_from, w.qkv_stride, w.v_chunked = at, t.rows, self.LONG_FROM, qkv_n, int(t.v_chunked)
        elif t.attn == "ragged":
            w = MqDecodeAttentionRaggedArgs()
            w.a, w.rows, w.batch, w.split_from, w.qkv_stride = at, t.rows, t.batch, self.LONG_FROM, qkv_n
            w.row_seq, w.row_pos = t.row_seq.data_ptr(), t.row_pos.data_ptr()
        else:
            w = at
        p = self._gemv(im.op, xq=t.attn_q.data_ptr(), a_grid=_grid(im.g_o, self._keep), resid=t.x.data_ptr(), y=t.x.data_ptr())
        p.out_grid[0] = _grid(attn.o_proj.output_quantizer, self._keep)
        return ({"multi": "attn_multi", "ragged": "attn_ragged"}.get(t.attn, "attn"), w), self._finish_gemv(t, im.op, p, s.heads * s.head_dim, s.hidden)

    def _ffn_launches(self, im: _Images, t: _Target, resid: torch.Tensor, **extra):
        """post_attention_layernorm + interleaved w1|w3 stream + gated activation + w2's input quantizer, then w2 from that int8 image +
        the residual `resid`.  extra: more fields of the w1|w3 record (four launches: o_proj's epilogue in front of the norm)."""
        s, keep, mlp = self.shape, self._keep, im.layer.mlp
        act, iq2 = mlp.act_fn, mlp.w2.input_quantizer
        p = self._gemv(im.w13, **im.norm2, x=t.x.data_ptr(), gate_q=t.gate_q.data_ptr(), gate_act=0 if isinstance(act, Q.QSiLU) else 1,
                       gate_mid=_grid(act.input2_quantizer if isinstance(act, Q.QSiLU) else None, keep),
                       gate_actout=_grid(act.output_quantizer, keep), gate_out=_grid(iq2, keep), **extra)
        p.out_grid[0], p.out_grid[1] = _grid(mlp.w1.output_quantizer, keep), _grid(mlp.w3.output_quantizer, keep)
        gate = self._finish_gemv(t, im.w13, p, s.hidden, 0, s.ffn)
        p = self._gemv(im.w2, xq=t.gate_q.data_ptr(), a_grid=_grid(iq2, keep), resid=resid.data_ptr(), y=t.x.data_ptr())
        p.out_grid[0] = _grid(mlp.w2.output_quantizer, keep)
        return gate, self._finish_gemv(t, im.w2, p, s.ffn, s.hidden)

    def _lower_chain(self, li: int, im: _Images, t: _Target) -> _Chain:
        """Layer li as the five-launch chain on target t."""
        qkv = self._qkv_launch(im, t)
        at, o_proj = self._attn_launches(li, im, t)
        return _Chain(qkv, at, o_proj, *self._ffn_launches(im, t, t.x))

    def _head_batch(self, x: torch.Tensor, logits: torch.Tensor, rows: int, pos: Optional[torch.Tensor] = None) -> MqDecodeHeadBatchArgs:
        """mq_decode_head_batch's record: final norm + lm_head over `rows` rows of x into logits.  pos (one per row): a row whose
        position is the cache_len sentinel keeps its logits."""
        s, hb = self.shape, MqDecodeHeadBatchArgs()
        hb.x, hb.x_stride = x.data_ptr(), s.hidden
        hb.norm_weight, hb.norm_bias = self.norm_w.data_ptr(), (self.norm_b.data_ptr() if self.norm_b is not None else None)
        hb.layernorm, hb.eps = int(self.norm_ln), float(self.model.norm.eps)
        hb.w, hb.bias = self.lm_w.data_ptr(), (self.lm_b.data_ptr() if self.lm_b is not None else None)
        hb.K, hb.V, hb.batch = s.hidden, s.vocab, rows
        hb.logits, hb.logits_stride = logits.data_ptr(), s.vocab
        if pos is not None:
            hb.pos, hb.cache_len = pos.data_ptr(), self.cache_len
        return hb

    # -- the rows step (step_tokens) ------------------------------------------------------------------------------------------
    _ENTRY_ROWS = {"gemv": "mq_decode_gemv_batch", "gemv_grouped": "mq_decode_gemv_grouped", "attn_multi": "mq_decode_attention_multi",
                   "attn_ragged": "mq_decode_attention_ragged"}

    def _lower_row_chain(self, head_pos: Optional[torch.Tensor] = None, **attn):
        """The launch records of a rows step, self._rows = (phases, head): per layer the five-launch chain over max_rows rows
        (mq_decode_gemv_batch / _grouped and the attention launch that `attn`, the _Target's attention fields, names) over the
        engine's own caches, on the norms and weight images the engine's chain already holds (self._images: no weight is stored
        twice), plus mq_decode_head_batch (head_pos: its per-row positions).  Row buffers of their own; the row count is set per
        launch (_set_rows)."""
        s, dev, R = self.shape, self.dev, self.max_rows
        H, D = s.heads, s.head_dim
        self.rx = torch.zeros(R, s.hidden, device=dev)
        self.rqkv = torch.zeros(R, self.qkv.shape[-1], device=dev)
        self.rattn_q = torch.zeros(R, H * D, dtype=torch.int8, device=dev)
        self.rpart = torch.zeros(R, self.LONG_SPLITS, H * D, dtype=torch.int64, device=dev)
        self.rticket = torch.zeros(R, H, dtype=torch.int32, device=dev)
        self.rgate = torch.zeros(R, s.ffn, dtype=torch.int8, device=dev)
        self.rlogits = torch.zeros(R, s.vocab, device=dev)
        t = _Target(self.rx, self.rqkv, self.rattn_q, self.rpart, self.rticket, self.rgate, self.k_cache, self.v_cache, nsplit=self.LONG_SPLITS,
                    rows=R, **attn)
        with torch.no_grad():
            phases = [p for li, im in enumerate(self._images) for p in self._lower_chain(li, im, t)]
        self._rows = (phases, self._head_batch(self.rx, self.rlogits, R, pos=head_pos))
        self._row_graphs = {}

    def _set_rows(self, T: int):
        phases, hb = self._rows
        for kind, a in phases:
            if kind == "gemv":
                a.batch = T
            elif kind == "gemv_grouped":
                a.b.batch = T
            else:
                a.rows = T
        hb.batch = T

    def _launch_rows(self, T: int):
        """Embedding rows + 5 launches per layer over T rows + norm / lm_head for T rows, on the current stream (reads rtok and the
        positions the attention records point at)."""
        st = torch.cuda.current_stream(self.dev).cuda_stream
        phases, hb = self._rows
        torch.index_select(self.embed, 0, self.rtok[:T], out=self.rx[:T])
        for kind, a in phases:
            _lib.call(self._ENTRY_ROWS[kind], ctypes.byref(a), st)
        _lib.call("mq_decode_head_batch", ctypes.byref(hb), st)

    def _spec_keep(self, drawn: Sequence[int], props: Sequence[int], eos: set, budget: int, rows: Optional[torch.Tensor], *seq):
        """The sequence `seq`'s share of a speculative round, behind the step that ran [t, d1 .. dk] for it: spec_accept on the tokens
        `drawn` from its rows, the round's counts in self.spec_stats, and -- rows: its logits rows of that step; None after a plain
        step, which leaves nothing to drop -- rewind to the kept tokens (t and the accepted proposals stay cached) with the last kept
        row as the sequence's logits.  Returns spec_accept's (kept tokens, accepted, stop)."""
        P = self.position(*seq) - len(drawn)
        new, acc, stop = spec_accept(drawn, props, eos, budget=budget, room=self.cache_len - P)
        self.spec_stats["proposed"] += len(props)
        self.spec_stats["accepted"] += acc
        if rows is not None:
            self.rewind(*seq, P + len(new))
            self._logits_row(*seq).copy_(rows[len(new) - 1])
        return new, acc, stop


class DecodeEngine(_DecodeBase):
    MAX_ROWS = 8                         # step_tokens: tokens per multi-token step (MQ_DECODE_MAX_BATCH), lowered by the shape (max_rows)
    LONG4_FROM = 1024                    # four launches: the 1024-thread attention + o_proj launch from here on (mq_decode_attention_oproj_args.threads):
                                         # 256 / 1024 threads at 256 | 512 | 1024 | 2048 positions: 1768 | 1701 | 1555 | 1331 against 1669 | 1646 | 1595 | 1482 tok/s
    # The largest cache_len each attention launch serves (csrc/mq_decode.hip, ao_max_cache / kAttnMaxCache): 160 KiB of LDS per workgroup
    # holds the kernel's static LDS plus 4 (five launches) or 7 (four launches) bytes per cached position.  Static LDS from hipcc
    # -Rpass-analysis=kernel-resource-usage, head_dim -> bytes: five launches 8336 / 8432 / 8624 / 9008 (4 x 32768 fits: the C entry's
    # 32768 binds); four launches 2240 / 2368 / 2624 / 3136 at 256 threads, 8528 / 8656 / 8912 / 9424 at 1024 threads.
    LDS_BYTES = 160 * 1024
    ATTN_MAX_CACHE = 32768
    ROW_IMAGE_BYTES, ROW_HEAD_FLOATS = _DecodeBase.MAX_IMAGE_BYTES, _DecodeBase.MAX_HEAD_FLOATS      # (the same limits, for the T rows of step_tokens)
    AO_STATIC_LDS = {256: {32: 2240, 64: 2368, 128: 2624, 256: 3136}, 1024: {32: 8528, 64: 8656, 128: 8912, 256: 9424}}

    @classmethod
    def max_cache_len(cls, launches: int, head_dim: int, threads: Optional[int] = None) -> int:
        """Largest cache_len the attention launch of the `launches` chain admits at this head_dim.  Four launches: threads 256 / 1024 for
        one variant, None for what an engine needs (it replays both, the 1024-thread one from long_from on)."""
        if launches == 5:
            return cls.ATTN_MAX_CACHE
        if threads is None:
            return min(cls.max_cache_len(4, head_dim, t) for t in cls.AO_STATIC_LDS)
        return (cls.LDS_BYTES - cls.AO_STATIC_LDS[threads][head_dim]) // 7 // 16 * 16

    def __init__(self, model, cache_len: int = 2048, attn_splits: Optional[int] = None, prefetch: float = 0.5, prefetch_delay_us: Optional[float] = None,
                 launches: int = 4, long_from: Optional[int] = None):
        """launches: 4 (round 6, default) = per layer {norm + q|k|v, RoPE / cache append / attention + o_proj's contraction, o_proj's
        epilogue + norm + w1|w3 + gate, w2}; 5 = round 2-5's chain with o_proj as a launch of its own.  A geometry the 4-launch kernels
        do not serve -- incl. a cache_len above max_cache_len(4, head_dim) and a model with per-group weight grids (QuantConfig
        group_size: mq_decode_gemv_grouped) -- falls back to 5 (self.launches says which); a cache_len
        above max_cache_len(5, head_dim) raises RuntimeError.  The 4-launch chain keeps the VALUE cache transposed in 16-position chunks
        ([kv_heads, cache_len / 16, head_dim, 16]: its p.v sweep is v_dot4 work on coalesced KiB requests); use cached_values() / load_cached_values() to read / write it in
        the logical [kv_heads, positions, head_dim] layout."""
        from .llama import LlamaForCausalLM
        assert isinstance(model, LlamaForCausalLM)
        assert launches in (4, 5)
        self.model, self.shape = model, model.shape
        s = self.shape
        dev = next(model.parameters()).device
        self.dev, self.cache_len = dev, int(cache_len)
        self._prefetch = (prefetch, prefetch_delay_us)           # (delay None: by chain, once self.launches is known)
        self.cos, self.sin = model.cos.contiguous(), model.sin.contiguous()
        # per-group weight grids: the five-launch chain (o_proj's contraction inside the four-launch attention launch has no per-group fold)
        self.grouped = any(isinstance(m, Q.QLinear) and m.weight_quantizer is not None and _Linear.is_grouped(m) for m in model.modules())
        self.oproj_geom = self._chain_geometry(s, self.cos.shape[1], self.cache_len, 5 if self.grouped else launches)
        self.launches = 4 if self.oproj_geom is not None else 5
        self.v_transposed = self.launches == 4
        self.long_from = self.LONG4_FROM if long_from is None else int(long_from)      # (four launches) first position of the long-cache graph
        if prefetch_delay_us is None:
            # when the prefetch rows of the attention launch start streaming w1|w3 into the L2s: behind the attention's own dependent
            # requests.  Five launches: 1.5 us (round 3).  Four launches: 2.5 us -- 0.8 / 1.5 / 2.5 -> 1 748 / 1 743 / 1 756-1 766 tok/s
            # (the attention + o_proj launch is longer and requests o_proj's weights behind its scores: profiles/r06/decode_prefetch_ab.log)
            self._prefetch = (prefetch, 2.5 if self.launches == 4 else 1.5)
        if self.launches == 4:
            self.o_acc = torch.zeros(s.hidden, dtype=torch.int32, device=dev)              # o_proj's integer sums (split-K over the heads)
            self.x_mid = torch.zeros(s.hidden, device=dev)                                 # residual stream behind the attention block
            self.rope_row = torch.zeros(2 * self.cos.shape[1], device=dev)                 # {cos[pos], sin[pos]}, staged once per token
        self.x = torch.zeros(s.hidden, device=dev)
        self.qkv = torch.zeros((s.heads + 2 * s.kv_heads) * s.head_dim, device=dev)
        self.attn_q = torch.zeros(s.heads * s.head_dim, dtype=torch.int8, device=dev)     # pv_bmm's output as o_proj's int8 image
        # workgroups per head in the attention launch (64-position blocks interleaved over them).  None = by position: one workgroup
        # per head while the cache is short (the ticket-ordered combine of a split launch costs ~3 us), LONG_SPLITS of them from
        # LONG_FROM cached positions on, where the sweeps over the cache outweigh it (measured crossover)
        self.auto_splits = attn_splits is None
        self.attn_splits = int(attn_splits) if attn_splits else 1
        assert 1 <= self.attn_splits <= 16
        self.attn_part = torch.zeros(max(self.attn_splits, self.LONG_SPLITS), s.heads * s.head_dim, dtype=torch.int64, device=dev)
        self.attn_ticket = torch.zeros(s.heads, dtype=torch.int32, device=dev)
        self.gate_q = torch.zeros(s.ffn, dtype=torch.int8, device=dev)
        self.logits = torch.zeros(s.vocab, device=dev)
        self.pos = torch.zeros(1, dtype=torch.int32, device=dev)
        self.tok = torch.zeros(1, dtype=torch.int64, device=dev)
        # keys / values as int8 indices (index - 128) on qk_bmm.input2 / pv_bmm.input2's grids
        self.k_cache = [torch.zeros(s.kv_heads, self.cache_len, s.head_dim, dtype=torch.int8, device=dev) for _ in model.layers]
        # four launches: [kv_heads, cache_len / 16, head_dim, 16] -- 16-position chunks of all dimensions, each dimension's 16 positions
        # contiguous (the p.v sweep reads a chunk as one coalesced KiB and contracts it with v_dot4); five launches: [kv_heads, cache_len, head_dim]
        vshape = (s.kv_heads, self.cache_len // 16, s.head_dim, 16) if self.v_transposed else (s.kv_heads, self.cache_len, s.head_dim)
        self.v_cache = [torch.zeros(vshape, dtype=torch.int8, device=dev) for _ in model.layers]
        self._host_pos = 0                                   # mirror of self.pos for the cache-overflow guard (no device read-back)
        assert self.cos.shape[0] >= self.cache_len, "rope tables shorter than the cache"
        # step_tokens: rows per multi-token step -- T * K int8 images in the batched GEMV launches' LDS, T * hidden floats in the head's
        big = max(s.hidden, s.ffn, s.heads * s.head_dim)
        self.max_rows = max(1, min(self.MAX_ROWS, self.ROW_IMAGE_BYTES // big, self.ROW_HEAD_FLOATS // s.hidden))
        self.spec_stats = None
        self.append_stats = None                             # what the last prefill(append=True) did
        self._append_images = None                           # per layer ImageCache of prefill(append=True), allocated on first use
        self.graph = None
        self.graph_long = None
        self._sampler = None                                 # mq_sample over logits / pos / tok (sample(), generate(sampling=...))
        self._sample_graphs = {}                             # (step variant, penalised) -> the captured sample + step graph, recorded on first use
        self._lp = None                                      # mq_logprob_top behind every selection launch (set_logprobs), or None
        self._lp_launches = {}                               # n_top -> its LogprobLaunch (record buffers), allocated on first request
        self._rows_at = None                                 # (T, position behind it) of the last step_tokens call: what sample_rows may draw
        self._lower()

    @classmethod
    def _chain_geometry(cls, s, rot_dim, cache_len, launches):
        """_oproj_geometry when the four-launch chain is asked for and serves this shape AND cache_len, else None (five launches);
        RuntimeError when the five-launch attention cannot hold cache_len either."""
        if not 0 < cache_len <= cls.max_cache_len(5, s.head_dim):
            raise RuntimeError(f"DecodeEngine: cache_len={cache_len} is outside 1 .. {cls.max_cache_len(5, s.head_dim)}, the cached positions "
                               f"the attention launch holds in LDS")
        if launches != 4 or cache_len % 16 or s.head_dim not in cls.AO_STATIC_LDS[256] or cache_len > cls.max_cache_len(4, s.head_dim):
            return None
        return cls._oproj_geometry(s, rot_dim)

    @staticmethod
    def _oproj_geometry(s, rot_dim):
        """(slices, threads per row) of mq_decode_attention_oproj for this shape, or None when the 4-launch kernels do not serve it:
        heads x slices workgroups ~ one per CU; a workgroup's 256 threads hold hidden / slices rows x head_dim bytes of o_proj."""
        D, H, N = s.head_dim, s.heads, s.hidden
        if D not in (32, 64, 128, 256) or rot_dim % 2 or rot_dim > min(D, 256) or N > 4096 or N % 4:
            return None
        chunks = D // 16
        for slices in range(max(256 // H, 1), 0, -1):
            if N % slices:
                continue
            R = N // slices
            for tpr in (1, 2, 4):                              # fewest threads per row: the atomics leave in full waves
                if chunks % tpr == 0 and chunks // tpr <= 8 and R * tpr <= 256:
                    return slices, tpr
        return None

    def _lower(self):
        """Build the launch records from the model as it is now (_lower_model): per layer the four- or five-launch chain over the engine's
        own single-row buffers."""
        prefetch, prefetch_delay_us = self._prefetch
        self._rows = None         # T-row phases of step_tokens: lowered on first use, from the layers' images (_lower_rows)
        self._row_graphs = {}
        self._row_sel = None      # mq_sample_rows over the T-row buffers (sample_rows): built on first use
        self._row_sample_graphs = {}                         # (T, penalised) -> the captured rows step + selection graph
        self.oproj_images = []
        self._lower_model()
        t = _Target(self.x, self.qkv, self.attn_q, self.attn_part, self.attn_ticket, self.gate_q, self.k_cache, self.v_cache, nsplit=self.attn_splits)
        with torch.no_grad():
            for li, layer in enumerate(self.model.layers):
                im = self._layer_images(layer, head_sliced=self.launches == 4)
                chain = self._lower_chain4(li, im, t) if self.launches == 4 else self._lower_chain(li, im, t)
                self.phases += [p for p in chain if p is not None]
                # The attention launch of layer L pulls (a share of) layer L's w1|w3 stream into the L2s with extra workgroups: it keeps 32 of
                # 256 CUs busy and leaves the memory fabric idle, while w1|w3 is the step's biggest stream.  Measured (TinyLlama shape, context
                # 256): share 0 / 0.5 / 0.7 / 1.0 -> 0.678 / 0.656 / 0.665 / 0.690 ms per token: the attention's own dependent loads queue
                # behind the prefetch stream, so half of it, started 1.5 us into the launch, is the optimum.
                at, (kind, gate) = chain.attn[1], chain.gate
                if prefetch and kind == "gemv":           # the grouped launch spreads its rows differently: its workgroups would not meet these bytes
                    n, per, tot = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
                    _lib.call("mq_decode_gemv_geometry", ctypes.byref(gate), ctypes.byref(n), ctypes.byref(per), ctypes.byref(tot))
                    at.prefetch, at.prefetch_stride, at.prefetch_total, at.prefetch_wgs = gate.w, per.value, tot.value, n.value
                    at.prefetch_bytes_per_wg = min(per.value, int(per.value * float(prefetch)) // 1024 * 1024)
                    at.prefetch_delay = int(prefetch_delay_us * 100)

    def _lower_chain4(self, li: int, im: _Images, t: _Target) -> _Chain:
        """Layer li as four launches (csrc/mq_decode.hip: decode_attention_oproj_kernel, OPRE): the q|k|v launch also clears o_proj's sums,
        the attention launch contracts o_proj (split-K over the heads, exact integer atomics), the w1|w3 launch starts with o_proj's
        epilogue + residual into x_mid, and w2 adds that stream behind the attention block."""
        s, op = self.shape, im.op
        qkv = self._qkv_launch(im, t, zero_acc=self.o_acc.data_ptr(), zero_n=s.hidden)
        at = self._attention_oproj(li, im)
        gate, w2 = self._ffn_launches(im, t, self.x_mid, o_acc=self.o_acc.data_ptr(), o_alpha=op.alpha.data_ptr(), o_ct=op.col_term.data_ptr(),
                                      o_bias=op.bias.data_ptr() if op.bias is not None else None,
                                      o_out=_grid(im.layer.self_attn.o_proj.output_quantizer, self._keep), x_mid=self.x_mid.data_ptr())
        return _Chain(qkv, ("attn_oproj", at), None, gate, w2)

    def _attention_oproj(self, li: int, im: _Images) -> MqDecodeAttentionOprojArgs:
        """The four-launch chain's RoPE / cache append / attention + o_proj's contraction launch."""
        s, keep, op, o_w = self.shape, self._keep, im.op, im.o_w
        slices, tpr = self.oproj_geom
        at = MqDecodeAttentionOprojArgs()
        at.qkv, at.k_cache, at.v_cache = self.qkv.data_ptr(), self.k_cache[li].data_ptr(), self.v_cache[li].data_ptr()
        at.rope_row, at.pos = self.rope_row.data_ptr(), self.pos.data_ptr()
        at.heads, at.kv_heads, at.head_dim, at.cache_len, at.rot_dim = s.heads, s.kv_heads, s.head_dim, self.cache_len, self.cos.shape[1]
        self._attention_grids(im.layer.self_attn, at, im.g_o)
        keep += [o_w, op]
        self.oproj_images.append((o_w, op))                   # (per layer; tests read them)
        keep.sources += op.sources
        keep.weights += op.weights
        at.o_w, at.o_wzp, at.o_acc, at.N, at.slices, at.tpr = o_w.data_ptr(), op.w_zp.data_ptr(), self.o_acc.data_ptr(), op.N, slices, tpr
        lg = lambda n: n.bit_length() - 1 if n > 0 and n & (n - 1) == 0 else None      # noqa: E731
        lgs, lgg, lgk = lg(slices), lg(s.heads // s.kv_heads), lg(s.kv_heads)
        ok = None not in (lgs, lgg, lgk) and (lgk > 3 or lgs + lgg >= 3 - lgk)
        at.lg_slices, at.lg_group, at.lg_kv = (lgs, lgg, lgk) if ok else (-1, 0, 0)
        at._mq_bytes = o_w.numel()
        return at

    # -- T-row phases (step_tokens) -----------------------------------------------------------------------------------------
    def _lower_rows(self):
        """The launch records of a multi-token step (_lower_row_chain): mq_decode_attention_multi over the engine's own caches in its
        value layout, on the images the single chain holds (incl. o_proj's row image `op` that the four-launch chain keeps next to its
        head-sliced copy).  The rows' tokens (rtok) and what sample_rows draws from them (rsel) are buffers of their own."""
        self.rtok = torch.zeros(self.max_rows, dtype=torch.int64, device=self.dev)
        self.rsel = torch.zeros(self.max_rows, dtype=torch.int64, device=self.dev)      # sample_rows: row j's drawn token
        self._row_sel, self._row_sample_graphs = None, {}
        self._lower_row_chain(attn="multi", v_chunked=self.v_transposed)

    def _finish_rows(self, T: int):
        self.logits.copy_(self.rlogits[T - 1])
        self.pos.add_(T)

    def _capture_rows(self, T: int, sel: Optional[RowsLaunch] = None):
        """Record the T-row step (incl. self.logits <- its last row and the position advance) as a hipGraph; with sel, mq_sample_rows
        over the rows behind it, in the same graph.  The warm-up launch outside the capture runs with the position at the cache_len
        sentinel: every attention row is idle, no cache byte changes (the selection's own warm-up writes rsel only)."""
        self._set_rows(T)
        pos0 = self.pos.clone()
        self.pos.fill_(self.cache_len)
        if sel is None:
            g = self._row_graphs[T] = self._record(lambda: self._launch_rows(T), lambda: self._finish_rows(T))
        else:
            with torch.cuda.device(self.dev):
                sel.launch(T)                                  # outside the capture: the select kernel's LDS ceiling

            def finish():
                self._finish_rows(T)
                sel.launch(T)
                if self._lp is not None:
                    self._lp.launch_rows(sel, T)
            g = self._row_sample_graphs[self._lp_key(T, self._sampler.penalized)] = self._record(lambda: self._launch_rows(T), finish)
        self.pos.copy_(pos0)
        return g

    @torch.no_grad()
    def step_tokens(self, tokens: Sequence[int]) -> torch.Tensor:
        """T = len(tokens) <= max_rows tokens of this sequence in ONE step: appended at positions p .. p + T - 1 (p = position()).
        Returns logits [T, vocab] (a device tensor, overwritten by the next call): row j is, bit for bit, what step(tokens[j]) returns
        after the earlier tokens, and the caches end as those T steps leave them.  The position advances by T; self.logits holds the
        last row.  After capture() a graph per row count is recorded on first use and replayed; the uncaptured launches give the same
        bits.  Raises if p + T > cache_len."""
        return self._step_rows(tokens, False, "step_tokens")

    def _step_rows(self, tokens: Sequence[int], select: bool, who: str) -> torch.Tensor:
        t = [int(v) for v in tokens]
        T = len(t)
        if not 1 <= T <= self.max_rows:
            raise ValueError(f"DecodeEngine.{who}: {T} tokens outside 1..{self.max_rows} (max_rows)")
        if self._host_pos + T > self.cache_len:
            raise RuntimeError(f"DecodeEngine.{who}: {T} tokens at position {self._host_pos} overflow the KV cache ({self.cache_len} positions)")
        if self._rows is None:
            self._lower_rows()
        sel = self._row_launch() if select else None
        self.rtok[:T].copy_(torch.tensor(t, dtype=torch.int64), non_blocking=False)
        if self.graph is not None:
            if select:
                (self._row_sample_graphs.get(self._lp_key(T, self._sampler.penalized)) or self._capture_rows(T, sel)).replay()
            else:
                (self._row_graphs.get(T) or self._capture_rows(T)).replay()
        else:
            self._set_rows(T)
            with torch.cuda.device(self.dev):
                self._launch_rows(T)
                self._finish_rows(T)
                if select:
                    sel.launch(T)
                    if self._lp is not None:
                        self._lp.launch_rows(sel, T)
        self._host_pos += T
        self._rows_at = (T, self._host_pos)
        return self.rsel[:T] if select else self.rlogits[:T]

    def _row_launch(self) -> RowsLaunch:
        if self._sampler is None:
            self.set_sampling(SamplingParams(temperature=0.0))
        if self._rows is None:
            self._lower_rows()
        if self._row_sel is None:
            self._row_sel = RowsLaunch(self._sampler, self.rlogits, self.pos, self.rtok[1:], self.rsel)
        return self._row_sel

    @torch.no_grad()
    def sample_rows(self, T: int) -> torch.Tensor:
        """mq_sample_rows on the T rows of the last step_tokens call, under the request of set_sampling (greedy until
        one is set): returns a device tensor [T] (overwritten by the next call; no host read) whose entry j is the token plain sampling
        draws at index position() - T + 1 + j from row j -- the token that follows tokens[:j + 1] of that call.  Under a penalised
        request row j sees the sequence's history plus tokens[1:j + 1], the proposals in front of it (read from the engine's own
        row-token buffer); the history is not written: count what is kept with sampling.history_count.  T must be that call's row
        count, with the position still behind it."""
        T = int(T)
        if self._rows_at != (T, self._host_pos):
            raise RuntimeError(f"DecodeEngine.sample_rows: T={T} is not the row count of a step_tokens call that the position ({self._host_pos}) "
                               f"still stands behind")
        with torch.cuda.device(self.dev):
            sel = self._row_launch()
            sel.launch(T)
            if self._lp is not None:
                self._lp.launch_rows(sel, T)
        return self.rsel[:T]

    @torch.no_grad()
    def step_sample_tokens(self, tokens: Sequence[int]) -> torch.Tensor:
        """step_tokens(tokens) and sample_rows(len(tokens)): returns the drawn tokens [T] (device).  After capture() the rows step and
        the selection are ONE graph per (T, penalised), recorded on first use like the sample + step graphs; the uncaptured launches
        give the same bits.  step_tokens' logits rows are in self.rlogits[:T]."""
        return self._step_rows(tokens, True, "step_sample_tokens")

    @torch.no_grad()
    def extend(self, tokens: Sequence[int]) -> torch.Tensor:
        """Append any number of tokens to the live sequence (no reset), max_rows per step: the same logits and caches as that many
        step() calls.  Returns self.logits (the last token's row)."""
        t = [int(v) for v in tokens]
        if self._host_pos + len(t) > self.cache_len:
            raise RuntimeError(f"DecodeEngine.extend: {len(t)} tokens at position {self._host_pos} overflow the KV cache ({self.cache_len} positions)")
        for i in range(0, len(t), self.max_rows):
            self.step_tokens(t[i:i + self.max_rows])
        return self.logits

    def rewind(self, n: int):
        """Drop the positions >= n (n <= position()): later steps compute what an engine that never saw them computes.  Only the
        position moves: no launch reads a cached byte at or past the position (the attention launches mask the keys, the values, the
        16-position chunk tail of the four-launch layout and the split blocks by it), so the dropped bytes are never read before they
        are overwritten.  self.logits is left as it is."""
        n = int(n)
        if not 0 <= n <= self._host_pos:
            raise ValueError(f"DecodeEngine.rewind: n={n} outside 0..{self._host_pos} (the current position)")
        self.set_position(n)
        return self

    def position(self) -> int:
        """Cached positions of the sequence (where the next token is appended)."""
        return self._host_pos

    # -- running -------------------------------------------------------------------------------------------------------------
    _ENTRY = {"gemv": "mq_decode_gemv", "gemv_grouped": "mq_decode_gemv_grouped", "attn": "mq_decode_attention", "attn_oproj": "mq_decode_attention_oproj"}

    def _launch(self, phases=None):
        """embedding gather + 4 (or 5) launches per layer + norm / lm_head, on the current stream; reads self.tok / self.pos."""
        st = torch.cuda.current_stream(self.dev).cuda_stream
        phases = self.phases if phases is None else phases
        if phases and phases[1][0] == "attn_oproj":             # token start: embedding row + this position's cos / sin row
            _lib.call("mq_decode_embed", self.embed.data_ptr(), self.tok.data_ptr(), self.shape.hidden, self.embed.shape[0], self.cos.data_ptr(),
                      self.sin.data_ptr(), self.pos.data_ptr(), self.cos.shape[1], self.cos.shape[0], self.x.data_ptr(), self.rope_row.data_ptr(), st)
        else:
            torch.index_select(self.embed, 0, self.tok, out=self.x.view(1, -1))
        for kind, a in phases:
            _lib.call(self._ENTRY[kind], ctypes.byref(a), st)
        _lib.call("mq_decode_head", self.x.data_ptr(), self.norm_w.data_ptr(), self.norm_b.data_ptr() if self.norm_b is not None else None,
                  int(self.norm_ln), float(self.model.norm.eps), self.lm_w.data_ptr(),
                  self.lm_b.data_ptr() if self.lm_b is not None else None, self.shape.hidden, self.shape.vocab, self.logits.data_ptr(), st)

    @staticmethod
    def _set_splits(phases, n: int):
        for kind, a in phases:
            if kind == "attn":
                a.nsplit = int(n)
            elif kind == "attn_oproj":                            # n > 1: the long-cache launch (1024 threads; the prefetch share inside the workgroups)
                a.threads = 1024 if n > 1 else 256

    def _variants(self):
        """[(phases, attention splits)]: what runs below / from LONG_FROM positions on (5 launches: the split attention launch)."""
        if self.launches == 4:
            if self.long_from <= 0:
                return [(self.phases, 2)]
            return [(self.phases, 1)] + ([(self.phases, 2)] if self.cache_len > self.long_from else [])
        v = [(self.phases, self.attn_splits)]
        if self.auto_splits and self.cache_len > self.LONG_FROM:
            v.append((self.phases, self.LONG_SPLITS))
        return v

    def _long_threshold(self) -> int:
        return self.long_from if self.launches == 4 else self.LONG_FROM

    def _variant_at(self, pos: int) -> int:
        return 1 if len(self._variants()) > 1 and pos >= self._long_threshold() else 0

    def capture(self):
        """Record one decode step (incl. the position increment) as a hipGraph; replay it with step().  Where a second variant exists
        (5 launches: the split attention from LONG_FROM cached positions on) a second graph is recorded; step() picks by position.
        Quantizers changed since the engine was built (recalibration, scale.copy_) are picked up here, in reset() and in prefill()."""
        if self._keep.stale():
            self._lower()
        self._row_graphs = {}                                    # (multi-token steps: one graph per row count, recorded on first use)
        self._row_sample_graphs = {}                             # (rows step + mq_sample_rows: one graph per row count and selection kind)
        self._sample_graphs = {}                                 # (sample + step: one graph per step variant and selection entry, recorded on first use)
        tok0, pos0, hp0 = self.tok.clone(), self.pos.clone(), self._host_pos
        graphs = []
        for phases, splits in self._variants():
            self._set_splits(phases, splits)
            self.attn_ticket.zero_()
            graphs.append(self._record(lambda: self._launch(phases), lambda: self.pos.add_(1)))
            self.tok.copy_(tok0); self.pos.copy_(pos0)
        self._set_splits(*self._variants()[0])                  # a direct launch after capture() runs the base variant again
        self._host_pos = hp0
        self.graph, self.graph_long = graphs[0], (graphs[1] if len(graphs) > 1 else None)
        return self

    def set_position(self, pos: int):
        """Continue from a cache that already holds `pos` positions (benchmarks; prefill() and reset() call this)."""
        assert 0 <= int(pos) <= self.cache_len
        self.pos.fill_(int(pos))
        self._host_pos = int(pos)
        self._rows_at = None

    def cached_values(self, li: int, n: Optional[int] = None) -> torch.Tensor:
        """Layer li's cached values as [kv_heads, n positions, head_dim] int8 indices (index - 128), whatever the engine's layout."""
        n = self._host_pos if n is None else int(n)
        c = self.v_cache[li]
        if not self.v_transposed:
            return c[:, :n]
        s = self.shape
        return c.permute(0, 1, 3, 2).reshape(s.kv_heads, self.cache_len, s.head_dim)[:, :n]      # [kv, chunk, 16, dim] -> [kv, position, dim]

    def load_cached_values(self, li: int, values: torch.Tensor):
        """values [kv_heads, n, head_dim] int8 -> positions 0 .. n - 1 of layer li's value cache."""
        n = values.shape[1]
        if self.v_transposed:
            s, full = self.shape, (n + 15) // 16
            pad = torch.zeros(s.kv_heads, full * 16, s.head_dim, dtype=torch.int8, device=self.dev)
            pad[:, :n] = values
            old = self.v_cache[li][:, :full].permute(0, 1, 3, 2).reshape(s.kv_heads, full * 16, s.head_dim)
            pad[:, n:] = old[:, n:]                                  # (positions behind n in the last chunk keep what they held)
            self.v_cache[li][:, :full] = pad.view(s.kv_heads, full, 16, s.head_dim).permute(0, 1, 3, 2)
        else:
            self.v_cache[li][:, :n] = values

    def fill_cache_random(self, n: int, seed: int = 0):
        """Benchmark helper: n positions of random cached indices (the same logical content for both cache layouts)."""
        g = torch.Generator(device=self.dev).manual_seed(seed)
        s = self.shape
        rnd = lambda: torch.randint(-128, 128, (s.kv_heads, n, s.head_dim), generator=g, device=self.dev, dtype=torch.int8)      # noqa: E731
        for c in self.k_cache:
            c[:, :n] = rnd()
        for li in range(len(self.v_cache)):
            self.load_cached_values(li, rnd())
        self.set_position(n)

    def reset(self):
        self._sync_grids()
        self.set_position(0)
        self.attn_ticket.zero_()
        for c in self.k_cache + self.v_cache:
            c.zero_()

    @torch.no_grad()
    def step(self, token: Optional[int] = None) -> torch.Tensor:
        """One token in, logits [vocab] out (device tensor, overwritten by the next step); the position advances by one.
        token None: use the token already sitting in self.tok (e.g. written by a device-side argmax)."""
        if self._host_pos >= self.cache_len:            # the kernels also refuse (they do nothing past the cache); fail loudly here
            raise RuntimeError(f"DecodeEngine.step: the KV cache is full ({self.cache_len} positions); reset() or build a longer cache")
        if token is not None:
            self.tok.fill_(int(token))
        if self.graph is not None:
            (self.graph_long if self.graph_long is not None and self._host_pos >= self._long_threshold() else self.graph).replay()
        else:
            phases, splits = self._variants()[self._variant_at(self._host_pos)]
            self._set_splits(phases, splits)
            with torch.cuda.device(self.dev):
                self._launch(phases)
            self.pos.add_(1)
        self._host_pos += 1
        self._rows_at = None
        return self.logits

    # -- seeded token selection on the device (csrc/mq_sample.hip) ---------------------------------------------
    def set_sampling(self, sampling: SamplingParams, stream: int = 0):
        """The request sample() serves from now on: rewritten in device memory, the captured graphs stay valid.  A request with a
        penalty or a logit bias (sampling.penalized) is served by mq_sample_penalized from the sequence's token history: generate()
        rebuilds that history itself; a caller who drives sample_step() gives it with observe_history(ids).  rewind() and
        set_position() do not touch it."""
        if not isinstance(sampling, SamplingParams):
            raise TypeError(f"DecodeEngine.set_sampling: expected SamplingParams, got {type(sampling).__name__}")
        if self._sampler is None:
            self._sampler = SampleLaunch(self.logits, self.pos, self.tok, self.cache_len)
        self._sampler.set_rows([sampling], [check_stream(stream)])
        return self

    def observe_history(self, ids):
        """Make `ids` the token history the penalties see: the history is cleared and every id is marked as a prompt token (the
        repetition penalty covers it; presence and frequency count generated tokens only).  Every token drawn afterwards by sample() /
        sample_step() under a penalised request is counted on the device.  After rewind() or set_position() the history is stale: call
        this again with the tokens the sequence now holds.  Without a penalised request since the engine was built it does nothing."""
        if self._sampler is None:
            self.set_sampling(SamplingParams(temperature=0.0))
        self._sampler.observe_prompt(0, ids, clear=True)
        return self

    @torch.no_grad()
    def sample(self) -> torch.Tensor:
        """mq_sample on self.logits into self.tok (a device tensor; no host read): token n = position() of the sequence under the
        request of set_sampling (greedy until one is set).  step() with no argument then consumes it."""
        if self._sampler is None:
            self.set_sampling(SamplingParams(temperature=0.0))
        with torch.cuda.device(self.dev):
            self._select()
        return self.tok

    def logprob_records(self, start: int, stop: int) -> TokenLogprobs:
        """The records of the tokens at sequence indices [start, stop) (CPU tensors, read back here): index n is the token sample()
        drew at position() == n.  Only indices drawn since set_logprobs(n_top) hold records."""
        return self._records(0, start, stop)

    def _capture_sample_step(self, variant: int, penalized: bool):
        """Record mq_sample (penalized: mq_sample_penalized) followed by the step (and the position advance) as one graph: the embedding launch reads the token the
        sample launch of the same replay wrote, and the sample launch reads the position in front of the step.  The launch outside
        the capture (the kernel's LDS ceiling) runs with the position at the cache_len sentinel: the row is idle, the token stays."""
        phases, splits = self._variants()[variant]
        self._set_splits(phases, splits)
        pos0 = self.pos.clone()
        self.pos.fill_(self.cache_len)

        def step():
            self._launch(phases)
            self.pos.add_(1)
        g = self._sample_graphs[self._lp_key(variant, penalized)] = self._record(self._select, step, before_capture=lambda: self.pos.copy_(pos0))
        self._set_splits(*self._variants()[0])
        return g

    @torch.no_grad()
    def sample_step(self) -> torch.Tensor:
        """sample() and step() on the drawn token.  After capture(): ONE graph replay (recorded on first use, per step variant); the
        uncaptured launches give the same token and the same logits.  self.tok holds the drawn token, self.logits the next row."""
        if self._host_pos >= self.cache_len:
            raise RuntimeError(f"DecodeEngine.sample_step: the KV cache is full ({self.cache_len} positions); reset() or build a longer cache")
        if self._sampler is None:
            self.set_sampling(SamplingParams(temperature=0.0))
        if self.graph is None:
            self.sample()
            return self.step()
        key = (self._variant_at(self._host_pos), self._sampler.penalized)      # a request of the other kind records a graph of its own
        (self._sample_graphs.get(self._lp_key(*key)) or self._capture_sample_step(*key)).replay()
        self._host_pos += 1
        self._rows_at = None
        return self.logits

    @torch.no_grad()
    def prefill(self, context_ids, append: bool = False) -> torch.Tensor:
        """Context encoding in ONE forward over the whole context (sim_model.py:176-193) instead of len(context) steps: the module
        graph's prefill (with llama.fuse_decoder_layer: 9 launches per layer) runs with a KV cache attached, the cached keys /
        values are put on their QMatMul input grids (what the step kernels keep in the cache) and the position is set behind the
        context.  Returns the logits of the last context position (self.logits).
        append=True: the tokens CONTINUE the live sequence at P = position().  P + len(ids) > cache_len raises
        RuntimeError before anything runs; P == 0 is the path above.  Otherwise the first (-P) % 64 tokens are stepped (extend():
        the bits of step()) up to a multiple of 64, P'; the rest -- if at least APPEND_MIN_TOKENS (and 2) tokens -- is ONE chunked
        forward of the model over image caches imported from the engine's caches (ops.attention_cache_import), whose new rows are
        exported back (ops.attention_cache_export); fewer tokens, a model whose attention is not the fused one, or grids / a head_dim
        the fused attention does not serve are stepped instead.  self.append_stats = {"stepped", "prefilled", "reason"} says what ran.
        Contract: the stepped tokens carry step()'s bits; the prefilled chunk carries the bits of the model's own chunked forward
        (model(chunk, cache=image_cache, pos=P')) over an image cache that holds the engine's cached indices.  The two paths agree
        with each other only within the bound that holds between prefill() and the steps behind it; no bitwise claim between them."""
        return self._prefill_append(context_ids) if append else self._prefill_fill(context_ids, False)

    # the one sequence as _DecodeBase's prefill and speculative bodies see it
    def _store_values(self, li: int, values: torch.Tensor):
        self.load_cached_values(li, values)

    def _step_seq(self, tokens: Sequence[int]):
        self.extend(tokens)

    def _seq_caches(self, li: int):
        return self.k_cache[li], self.v_cache[li]

    def _logits_row(self) -> torch.Tensor:
        return self.logits

    @torch.no_grad()
    def generate(self, context_ids, max_new_tokens: int, eos_token_id=None, prefill: bool = True, do_sample: bool = False,
                 temperature: float = 0.5, generator: Optional[torch.Generator] = None,
                 draft: Union[None, "DecodeEngine", Callable[[List[int], int], List[int]]] = None, num_draft: int = 4,
                 sampling: Optional[SamplingParams] = None, stream: int = 0, logprobs: Optional[int] = None):
        """SimModel.generate (mobilellm/model/sim_model.py:160-221): context encoding in one prefill forward (prefill=False: token by
        token through the step kernels), then per new token: next = argmax(logits) or, with do_sample, multinomial(softmax(logits /
        temperature)) (:198-201) -- on the device, into self.tok --, append it, stop if it is an EOS (:202-204), else run the step.
        The host reads one token id per step only to test for EOS and to return the ids.
        draft (greedy only): speculative generation -- another DecodeEngine over a model of the same vocabulary size, or a callable
        draft(ids, k) -> at most k proposals (prompt_lookup_draft) -- verified num_draft tokens at a time with step_tokens.  The
        returned ids equal the plain greedy ones token for token; self.spec_stats counts the rounds (_speculate).
        sampling (with stream, the sequence's identity): seeded selection on the device by mq_sample's rule (temperature, top-k, top-p,
        min-p, behind the repetition / presence / frequency penalties and the logit bias of the sequence's own tokens; DESIGN.md
        4.3e) -- the ids depend on (context, sampling, stream) only: BatchDecodeEngine.generate returns the same ids for this sequence
        in any batch and slot.  After capture() a token costs one graph replay (sample + step) and one token read-back; a sequence
        that ends on an EOS has then cached that token too (position() is one past the returned ids).
        logprobs (with sampling= only; 0 .. 20): returns (ids, TokenLogprobs) -- one record per new token (its log-probability under
        the model's RAW distribution, its rank, and the `logprobs` most likely alternatives), written on the device
        behind every sample launch and read back once at the end.  The ids are those of the same call without logprobs.  None (the
        default) returns what it always did, through the launches and graphs without mq_logprob_top."""
        n_top = check_logprobs("DecodeEngine.generate", logprobs, sampling)
        if sampling is not None:
            validate_generate_args("DecodeEngine.generate", sampling, do_sample, draft)
            with self._logprobs_for(n_top):
                return self._generate_sampled(context_ids, max_new_tokens, eos_token_id, prefill, sampling, stream, n_top)
        if draft is not None:
            if do_sample:
                raise ValueError("DecodeEngine.generate: a draft is for greedy decoding only (do_sample=True with a draft)")
            return self._speculate("DecodeEngine.generate", context_ids, max_new_tokens, eos_token_id, prefill, _Greedy(), draft, num_draft)
        ids = [int(t) for t in context_ids]
        assert len(ids) + max_new_tokens <= self.cache_len
        self._start_sequence(ids, prefill)
        out = list(ids)
        eos = _eos_set(eos_token_id)
        for _ in range(max_new_tokens):
            if do_sample:
                probs = torch.softmax(self.logits / temperature, dim=-1)
                self.tok.copy_(torch.multinomial(probs, num_samples=1, generator=generator))
            else:
                torch.argmax(self.logits, dim=-1, keepdim=True, out=self.tok)
            nxt = int(self.tok.item())
            out.append(nxt)
            if nxt in eos:
                break
            if self._host_pos >= self.cache_len:
                break
            self.step()
        return out

    def _generate_sampled(self, context_ids, max_new_tokens: int, eos_token_id, prefill: bool, sampling: SamplingParams, stream: int,
                          n_top: Optional[int] = None):
        ids = [int(t) for t in context_ids]
        assert len(ids) + max_new_tokens <= self.cache_len
        self.set_sampling(sampling, stream)
        self._start_sequence(ids, prefill)
        if self._sampler.penalized:
            self._sampler.observe_prompt(0, ids)                   # the history is rebuilt for every sequence
        out = list(ids)
        eos = _eos_set(eos_token_id)
        for made in range(1, max_new_tokens + 1):
            if made < max_new_tokens:
                self.sample_step()                                 # token n from the logits of n - 1, and the step on it
            else:
                self.sample()                                      # the last token needs no step
            nxt = int(self.tok.item())
            out.append(nxt)
            if nxt in eos:
                break
        return out if n_top is None else (out, self.logprob_records(len(ids), len(out)))

    def _start_sequence(self, ids: List[int], prefill: bool):
        self.reset()
        if prefill and len(ids) > 1:
            self.prefill(ids)
        else:
            for t in ids:
                self.step(t)

    @torch.no_grad()
    def _speculate(self, who: str, context_ids, max_new_tokens: int, eos_token_id, prefill: bool, select, draft, num_draft: int):
        """Speculative decoding, for generate(draft=...) (select: _Greedy) and generate_speculative (_Sampled).  The sequence starts as
        in the plain loop and the first new token is chosen from the context's logits.  Then per round, with t the last token (not yet
        cached) and P the position: k = min(num_draft, max_rows - 1, tokens still allowed - 1, cache room - 1) proposals d1..dk from
        the draft, ONE rows step over [t, d1..dk] whose tokens `select` chooses, spec_accept on them and rewind to P + the kept tokens
        (_spec_keep).  Every kept token is the plain loop's: row i holds the logits after t, d1..di, bit for bit, and a token depends
        on its row (greedy) or on its row and its index (sampling) alone.  The stops are plain generate's: EOS, max_new_tokens, the
        cache end.  Afterwards the caches hold out[:position()]."""
        d_eng = _check_draft(who, self, draft, num_draft, (DecodeEngine,))
        draft = _CallableDraft(draft) if d_eng is None else _EngineDraft(d_eng, select)
        ids = [int(t) for t in context_ids]
        assert len(ids) + max_new_tokens <= self.cache_len
        eos = _eos_set(eos_token_id)
        stats = self.spec_stats = _spec_stats()
        select.start(self, ids, prefill)
        out = list(ids)
        if max_new_tokens <= 0:
            return out
        draft.start(ids, prefill)
        new = [select.first(self)]                                 # (under a penalised request its own launch has counted it)
        draft.settle(out, new, 0, [])
        out += new
        made = 1
        if new[0] in eos or made >= max_new_tokens or self._host_pos >= self.cache_len:
            return out
        while True:
            k = max(0, min(int(num_draft), self.max_rows - 1, max_new_tokens - made - 1, self.cache_len - self._host_pos - 1))
            props = draft.propose(out, k) if k > 0 else []
            drawn = select.rows(self, [out[-1]] + props)
            stats["rounds"] += 1
            stats["target_steps"] += 1
            new, acc, stop = self._spec_keep(drawn, props, eos, max_new_tokens - made, self.rlogits)
            select.recount(self, [], new)
            draft.settle(out, new, acc, props)
            out += new
            made += len(new)
            if stop:
                return out

    @torch.no_grad()
    def generate_speculative(self, context_ids, max_new_tokens: int, draft, *, sampling: SamplingParams, stream: int = 0, num_draft: int = 4,
                             eos_token_id=None, prefill: bool = True, logprobs: Optional[int] = None):
        """Speculative decoding under seeded sampling: returns, token for token, the ids of
        generate(context_ids, max_new_tokens, sampling=sampling, stream=stream, ...).  Token n of a sequence is a function of its logits,
        the request, the stream and n alone, so no rejection scheme is needed: the first token comes from sample(); then per round
        (_speculate) ONE step_tokens([t, d1..dk]) with mq_sample_rows drawing every row at its own index (one graph after capture()),
        one read-back of the T tokens, spec_accept on them and rewind to P + the kept tokens; under a penalised request row j sees the
        history plus d1..dj, and the kept tokens are then counted with history_count(+1).  draft: another DecodeEngine of the same
        vocabulary size, or a callable draft(ids, k).  An engine draft is set to the SAME sampling and stream and proposes with its own
        sample_step() / sample(): it shares the Gumbel noise with the target, so it is accepted wherever its logits are close (a
        self-draft: always); its history is brought back to the sequence's with history_count (-1 for the rejected proposals, +1 for the
        token that replaced them and for the first token), its cache with extend / rewind.  self.spec_stats counts the rounds.
        logprobs (0 .. 20): returns (ids, TokenLogprobs), the records of generate(..., logprobs=logprobs).  Every row of a round writes
        its record at its own token index, so a rejected row's record is overwritten when that index is drawn again (by the next
        round's row 0 at the latest) and nothing behind the returned ids is read: no bookkeeping is needed.  Only the target computes
        log-probabilities; a draft engine's switch is left as it is."""
        if not isinstance(sampling, SamplingParams):
            raise TypeError(f"DecodeEngine.generate_speculative: sampling must be SamplingParams, got {type(sampling).__name__}")
        n_top = check_logprobs("DecodeEngine.generate_speculative", logprobs, sampling)
        ids = [int(t) for t in context_ids]
        with self._logprobs_for(n_top):
            out = self._speculate("DecodeEngine.generate_speculative", ids, max_new_tokens, eos_token_id, prefill,
                                  _Sampled(sampling, check_stream(stream)), draft, num_draft)
            return out if n_top is None else (out, self.logprob_records(len(ids), len(out)))
