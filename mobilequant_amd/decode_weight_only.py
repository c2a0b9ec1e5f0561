"""Single-sequence decode engine for weight-only (W4A16) models.

`WeightOnlyDecodeEngine` runs one token of a `LlamaForCausalLM` whose linears are `WeightOnlyLinear`s (create_weight_only_qmodel, or
gptq_quantize_model(..., weight_only=True)) as 5 launches per decoder layer between the token-start launch and the head launch, all
hand-written HIP (csrc/mq_w4a16_decode.hip, and mq_decode_embed / mq_decode_head of csrc/mq_decode.hip):

    mq_decode_embed              x = embed_tokens[tok] (* hidden ** 0.5), and this position's cos / sin row
    per layer
      mq_w4a16_decode_gemv       qkv = (q | k | v)(input_layernorm(x))          norm prologue, bias epilogue, one concatenated image
      mq_w4a16_decode_attention  RoPE, cache append at pos, softmax(q k / sqrt D) v over the fp32 cache
      mq_w4a16_decode_gemv       x_mid = x + o_proj(o)                           plain prologue, residual epilogue
      mq_w4a16_decode_gemv       h = act(w1(y2)) * w3(y2), y2 = post_attention_layernorm(x_mid)   norm prologue, gated epilogue on the
                                                                                 row-interleaved w1 | w3 image
      mq_w4a16_decode_gemv       x' = x_mid + w2(h)                              plain prologue, residual epilogue
    mq_decode_head               logits = lm_head(norm(x'))                      fp32

It computes what the module chain `model(ids[:, t:t+1], cache, pos=t)` computes, up to the order of floating-point sums; the caches are
`model.new_cache(1, cache_len)`, so prefill is the model's own forward over them.  Nothing falls back to another path: a model the
kernels do not serve is refused at construction with the module and the reason.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional

import torch
import torch.nn as nn

from . import _lib, weight_only
from .decode import _eos_set
from .llama import LlamaForCausalLM
from .quantization import qmodule as Q
from .quantization.fp_ops import FMatMul, HFRMSNorm
from .sampling import SampleLaunch, SamplingParams, check_stream

ATTN_HEAD_DIMS = (32, 64, 128, 256)
ATTN_MAX_SPLITS = 16
ATTN_MAX_CHUNK = 8192            # cached positions per attention split (its scores sit in LDS)
HEAD_MAX_HIDDEN = 12288          # mq_decode_head


def concat_rows(mods) -> tuple:
    """The packed images of several WeightOnlyLinears over the same input, concatenated row-wise: (qweight [sum N, K / 2], scales, zeros
    [sum N, G], bias fp32 [sum N] or None).  One launch then streams them; a module without a bias contributes zeros when another has one."""
    mods = list(mods)
    grids = [m._grid16() for m in mods]
    bias = None
    if any(m.bias is not None for m in mods):
        bias = torch.cat([m.bias.detach().float() if m.bias is not None else torch.zeros(m.out_features, device=m.qweight.device) for m in mods])
    return (torch.cat([m.qweight for m in mods]).contiguous(), torch.cat([s for s, _ in grids]).contiguous(),
            torch.cat([z for _, z in grids]).contiguous(), None if bias is None else bias.contiguous())


def interleave_rows(gate, up) -> tuple:
    """The packed images of the gate (w1) and the up (w3) linear interleaved row by row -- image row 2 n is w1's row n, row 2 n + 1 w3's --
    with scales and zeros to match: (qweight [2 N, K / 2], scales, zeros [2 N, G])."""
    (gs, gz), (us, uz) = gate._grid16(), up._grid16()
    il = lambda a, b: torch.stack((a, b), dim=1).reshape(2 * a.shape[0], a.shape[1]).contiguous()   # noqa: E731
    return il(gate.qweight, up.qweight), il(gs, us), il(gz, uz)


def _refuse(name: str, why: str):
    raise ValueError(f"mobilequant_amd: WeightOnlyDecodeEngine: {name}: {why}")


def _norm_fields(norm, name: str) -> dict:
    """prologue / norm_weight / norm_bias / eps of mq_w4a16_decode_gemv for a HFRMSNorm or an nn.LayerNorm."""
    f32 = lambda t: None if t is None else t.detach().float().contiguous()   # noqa: E731
    if type(norm) is HFRMSNorm:
        if norm.l2norm_as_rmsnorm:
            _refuse(name, "the l2norm form of HFRMSNorm is not served (x * rsqrt(mean(x^2) + eps) only)")
        return dict(prologue="rmsnorm", norm_weight=f32(norm.weight), norm_bias=f32(norm.bias), eps=float(norm.eps))
    if type(norm) is nn.LayerNorm:
        return dict(prologue="layernorm", norm_weight=f32(norm.weight), norm_bias=f32(norm.bias), eps=float(norm.eps))
    _refuse(name, f"{type(norm).__name__} is neither HFRMSNorm nor nn.LayerNorm")


class WeightOnlyDecodeEngine:
    """One sequence of a weight-only LlamaForCausalLM, a token per step(), one hipGraph per token after capture().

    cache_len: positions of the fp32 KV caches (default: the model's max_pos; more is refused).  attn_splits: workgroups per head the
    attention launch spreads the cached positions over (1 .. 16; default: 1 up to 1024 positions, else 256 // heads); the logits' bits
    depend on it and on nothing else -- the same step gives the same bits every time, eager or replayed."""

    def __init__(self, model, cache_len: Optional[int] = None, attn_splits: Optional[int] = None):
        if not isinstance(model, LlamaForCausalLM):
            raise ValueError(f"mobilequant_amd: WeightOnlyDecodeEngine: expected a LlamaForCausalLM, got {type(model).__name__}")
        s = self.shape = model.shape
        self.model = model
        self.cache_len = int(s.max_pos if cache_len is None else cache_len)
        if not 1 <= self.cache_len <= s.max_pos:
            _refuse("cache_len", f"{self.cache_len} outside 1 .. max_pos = {s.max_pos} (the RoPE tables end there)")
        L = len(model.layers)
        # ---- refusals first: they need no device --------------------------------------------------------------------------------------
        for i, layer in enumerate(model.layers):
            for name, mod in (("self_attn.q_proj", layer.self_attn.q_proj), ("self_attn.k_proj", layer.self_attn.k_proj),
                              ("self_attn.v_proj", layer.self_attn.v_proj), ("self_attn.o_proj", layer.self_attn.o_proj),
                              ("mlp.w1", layer.mlp.w1), ("mlp.w3", layer.mlp.w3), ("mlp.w2", layer.mlp.w2)):
                if not isinstance(mod, Q.WeightOnlyLinear):
                    _refuse(f"layers.{i}.{name}", f"{type(mod).__name__} is not a WeightOnlyLinear (create_weight_only_qmodel first; QLinear "
                                                  "chains run on DecodeEngine)")
            att, mlp = layer.self_attn, layer.mlp
            if type(att.qk_bmm) is not FMatMul or type(att.pv_bmm) is not FMatMul:
                _refuse(f"layers.{i}.self_attn", "quantized qk_bmm / pv_bmm are not served (floating-point attention only)")
            qkv = (att.q_proj, att.k_proj, att.v_proj)
            if len({m.group_size for m in qkv}) != 1 or mlp.w1.group_size != mlp.w3.group_size:
                _refuse(f"layers.{i}", "q / k / v (and w1 / w3) share a launch and need one group_size")
            if mlp.w1.bias is not None or mlp.w3.bias is not None:
                _refuse(f"layers.{i}.mlp", "w1 / w3 with a bias are not served by the gated epilogue")
            for name, n, k, g, epi in ((f"layers.{i}.self_attn.q_proj|k_proj|v_proj", sum(m.out_features for m in qkv), att.q_proj.in_features,
                                        att.q_proj.group_size, "bias"),
                                       (f"layers.{i}.self_attn.o_proj", att.o_proj.out_features, att.o_proj.in_features, att.o_proj.group_size, "resid"),
                                       (f"layers.{i}.mlp.w1|w3", 2 * mlp.w1.out_features, mlp.w1.in_features, mlp.w1.group_size, "gated"),
                                       (f"layers.{i}.mlp.w2", mlp.w2.out_features, mlp.w2.in_features, mlp.w2.group_size, "resid")):
                if not weight_only.w4a16_decode_supported(n, k, g, epi):
                    _refuse(name, f"N={n}, K={k}, group_size={g} is outside mq_w4a16_decode_supported ({weight_only.DECODE_RULE})")
            if not (type(mlp.act_fn) is nn.SiLU or (type(mlp.act_fn) is nn.GELU and mlp.act_fn.approximate == "none")):
                _refuse(f"layers.{i}.mlp.act_fn", f"{mlp.act_fn!r} is neither SiLU nor the erf GELU")
            _norm_fields(layer.input_layernorm, f"layers.{i}.input_layernorm")
            _norm_fields(layer.post_attention_layernorm, f"layers.{i}.post_attention_layernorm")
        if s.head_dim not in ATTN_HEAD_DIMS:
            _refuse("self_attn", f"head_dim {s.head_dim} is not served by mq_w4a16_decode_attention ({ATTN_HEAD_DIMS})")
        if s.heads % s.kv_heads or s.rot_dim < 2 or s.rot_dim % 2 or s.rot_dim > s.head_dim:
            _refuse("self_attn", f"heads={s.heads}, kv_heads={s.kv_heads}, rot_dim={s.rot_dim}: heads % kv_heads == 0 and an even rot_dim in "
                                 "2 .. head_dim are needed")
        head_norm = _norm_fields(model.norm, "norm")
        if head_norm["prologue"] == "rmsnorm" and head_norm["norm_bias"] is not None:
            _refuse("norm", "a final HFRMSNorm with a bias is not served by mq_decode_head")
        if type(model.lm_head) is not nn.Linear:
            _refuse("lm_head", f"{type(model.lm_head).__name__} is not a floating-point nn.Linear (mq_decode_head streams fp32 weights)")
        if s.hidden % 4 or s.hidden > HEAD_MAX_HIDDEN:
            _refuse("lm_head", f"hidden={s.hidden}: mq_decode_head needs hidden % 4 == 0 and hidden <= {HEAD_MAX_HIDDEN}")
        if attn_splits is None:
            attn_splits = 1 if self.cache_len <= 1024 else max(1, min(ATTN_MAX_SPLITS, 256 // s.heads))
            while attn_splits < ATTN_MAX_SPLITS and -(-self.cache_len // attn_splits) > ATTN_MAX_CHUNK:
                attn_splits += 1
        self.attn_splits = int(attn_splits)
        if not 1 <= self.attn_splits <= ATTN_MAX_SPLITS or -(-self.cache_len // self.attn_splits) > ATTN_MAX_CHUNK:
            _refuse("attn_splits", f"{self.attn_splits} with cache_len={self.cache_len}: 1 .. {ATTN_MAX_SPLITS} splits of at most "
                                   f"{ATTN_MAX_CHUNK} positions each")
        w = model.embed_tokens.weight
        if not w.is_cuda or w.dtype != torch.float32:
            raise RuntimeError("mobilequant_amd: WeightOnlyDecodeEngine: the model must be an fp32 model on a ROCm device (there is no CPU path)")
        dev = self.dev = w.device

        # ---- buffers ------------------------------------------------------------------------------------------------------------------
        f32 = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)   # noqa: E731
        H, KV, D = s.heads, s.kv_heads, s.head_dim
        self.tok = torch.zeros(1, dtype=torch.int64, device=dev)
        self.pos = torch.zeros(1, dtype=torch.int32, device=dev)
        self._host_pos = 0
        self.x, self.x_mid = f32(s.hidden), f32(s.hidden)
        self.qkv, self.attn_out, self.h = f32((H + 2 * KV) * D), f32(H * D), f32(s.ffn)
        self.rope_row = f32(2 * s.rot_dim)
        self.logits = f32(s.vocab)
        self.caches = model.new_cache(1, self.cache_len, device=dev)       # [(k, v)] per layer, each [1, KV, T, D] fp32
        self.attn_part = f32(H * self.attn_splits * (D + 4)) if self.attn_splits > 1 else None
        self.attn_ticket = torch.zeros(H, dtype=torch.int32, device=dev) if self.attn_splits > 1 else None
        emb = w.detach()
        self.embed = (emb * (s.hidden ** 0.5) if s.embed_scale else emb).contiguous()
        self.cos, self.sin = model.cos.detach().float().contiguous(), model.sin.detach().float().contiguous()
        self.norm_w, self.norm_b = head_norm["norm_weight"], head_norm["norm_bias"]
        self.norm_ln, self.norm_eps = head_norm["prologue"] == "layernorm", head_norm["eps"]
        self.lm_w = model.lm_head.weight.detach().float().contiguous()
        self.lm_b = None if model.lm_head.bias is None else model.lm_head.bias.detach().float().contiguous()

        # ---- the launches: argument blocks filled once; self._keep holds every tensor they point at -----------------------------------
        self._keep: List[torch.Tensor] = []
        self.phases = []
        for i, layer in enumerate(model.layers):
            att, mlp = layer.self_attn, layer.mlp
            qw, qs, qz, qb = concat_rows((att.q_proj, att.k_proj, att.v_proj))
            gw, gs_, gz = interleave_rows(mlp.w1, mlp.w3)
            n_in = _norm_fields(layer.input_layernorm, "input_layernorm")
            n_post = _norm_fields(layer.post_attention_layernorm, "post_attention_layernorm")
            ow, (os_, oz), ob = att.o_proj.qweight, att.o_proj._grid16(), att.o_proj.bias
            dw, (ds_, dz), db = mlp.w2.qweight, mlp.w2._grid16(), mlp.w2.bias
            ob = None if ob is None else ob.detach().float().contiguous()
            db = None if db is None else db.detach().float().contiguous()
            k_c, v_c = self.caches[i]
            self._keep += [t for t in (qw, qs, qz, qb, gw, gs_, gz, ow, os_, oz, ob, dw, ds_, dz, db, *n_in.values(), *n_post.values())
                           if isinstance(t, torch.Tensor)]
            self.phases += [
                ("mq_w4a16_decode_gemv", weight_only.w4a16_decode_gemv_args(self.x, qw, qs, qz, self.qkv, group_size=att.q_proj.group_size,
                                                                           epilogue="bias", bias=qb, **n_in)),
                ("mq_w4a16_decode_attention", weight_only.w4a16_decode_attention_args(
                    self.qkv, k_c, v_c, self.rope_row, self.pos, self.attn_out, heads=H, kv_heads=KV, head_dim=D, rot_dim=s.rot_dim,
                    nsplit=self.attn_splits, part=self.attn_part, ticket=self.attn_ticket)),
                ("mq_w4a16_decode_gemv", weight_only.w4a16_decode_gemv_args(self.attn_out, ow, os_, oz, self.x_mid, group_size=att.o_proj.group_size,
                                                                           epilogue="resid", bias=ob, resid=self.x)),
                ("mq_w4a16_decode_gemv", weight_only.w4a16_decode_gemv_args(self.x_mid, gw, gs_, gz, self.h, group_size=mlp.w1.group_size,
                                                                           epilogue="gated", act="silu" if type(mlp.act_fn) is nn.SiLU else "gelu", **n_post)),
                ("mq_w4a16_decode_gemv", weight_only.w4a16_decode_gemv_args(self.h, dw, ds_, dz, self.x, group_size=mlp.w2.group_size,
                                                                           epilogue="resid", bias=db, resid=self.x_mid)),
            ]
        self.launches_per_token = len(self.phases) + 2
        assert self.launches_per_token == 5 * L + 2
        self.graph = None
        self._sampler = None

    # -- running -----------------------------------------------------------------------------------------------------------------------
    def _launch(self):
        """Token start, 5 launches per layer, head: on the current stream; reads self.tok / self.pos."""
        s = self.shape
        st = torch.cuda.current_stream(self.dev).cuda_stream
        _lib.call("mq_decode_embed", self.embed.data_ptr(), self.tok.data_ptr(), s.hidden, self.embed.shape[0], self.cos.data_ptr(),
                  self.sin.data_ptr(), self.pos.data_ptr(), self.cos.shape[1], self.cos.shape[0], self.x.data_ptr(), self.rope_row.data_ptr(), st)
        for entry, a in self.phases:
            _lib.call(entry, ctypes.byref(a), st)
        _lib.call("mq_decode_head", self.x.data_ptr(), None if self.norm_w is None else self.norm_w.data_ptr(),
                  None if self.norm_b is None else self.norm_b.data_ptr(), int(self.norm_ln), float(self.norm_eps), self.lm_w.data_ptr(),
                  None if self.lm_b is None else self.lm_b.data_ptr(), s.hidden, s.vocab, self.logits.data_ptr(), st)

    def capture(self):
        """Record one step (and the position's increment) as a hipGraph; step() then replays it at every position.  The launches first
        run once outside the capture (they set their LDS ceilings, which must not happen while capturing): self.logits is overwritten,
        the position stays."""
        with torch.cuda.device(self.dev):
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                self._launch()
            torch.cuda.current_stream().wait_stream(side)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._launch()
                self.pos.add_(1)
        self.graph = g
        return self

    def position(self) -> int:
        """Cached positions of the sequence (where the next token is appended)."""
        return self._host_pos

    def set_position(self, pos: int):
        """Continue from caches that already hold `pos` positions."""
        pos = int(pos)
        if not 0 <= pos <= self.cache_len:
            raise ValueError(f"WeightOnlyDecodeEngine.set_position: {pos} outside 0 .. {self.cache_len}")
        self.pos.fill_(pos)
        self._host_pos = pos
        return self

    def reset(self):
        self.set_position(0)
        if self.attn_ticket is not None:
            self.attn_ticket.zero_()
        for k, v in self.caches:
            k.zero_()
            v.zero_()
        return self

    def cached_keys(self, li: int, n: Optional[int] = None) -> torch.Tensor:
        """Layer li's cached (roped) keys [kv_heads, n positions, head_dim] fp32 (a view)."""
        return self.caches[li][0][0, :, :self._host_pos if n is None else int(n)]

    def cached_values(self, li: int, n: Optional[int] = None) -> torch.Tensor:
        return self.caches[li][1][0, :, :self._host_pos if n is None else int(n)]

    @torch.no_grad()
    def step(self, token: Optional[int] = None) -> torch.Tensor:
        """One token in, logits [vocab] out (fp32 device tensor, overwritten by the next step); the position advances by one.  token
        None: the token already in self.tok (written by the device-side selection)."""
        if self._host_pos >= self.cache_len:
            raise RuntimeError(f"WeightOnlyDecodeEngine.step: the KV cache is full ({self.cache_len} positions); reset() or build a longer cache")
        if token is not None:
            self.tok.fill_(int(token))
        if self.graph is not None:
            self.graph.replay()
        else:
            with torch.cuda.device(self.dev):
                self._launch()
            self.pos.add_(1)
        self._host_pos += 1
        return self.logits

    @torch.no_grad()
    def prefill(self, context_ids) -> torch.Tensor:
        """The context in ONE forward of the model over the engine's caches (from position 0); sets the position behind it and returns
        the last position's logits (self.logits)."""
        ids = [int(t) for t in context_ids]
        if not 1 <= len(ids) <= self.cache_len:
            raise RuntimeError(f"WeightOnlyDecodeEngine.prefill: {len(ids)} tokens do not fit the KV cache ({self.cache_len} positions)")
        out = self.model(torch.tensor([ids], dtype=torch.int64, device=self.dev), cache=self.caches, pos=0, last_logits_only=True)
        self.logits.copy_(out.reshape(-1))
        self.set_position(len(ids))
        return self.logits

    # -- generation --------------------------------------------------------------------------------------------------------------------
    def set_sampling(self, sampling: SamplingParams, stream: int = 0):
        if not isinstance(sampling, SamplingParams):
            raise TypeError(f"WeightOnlyDecodeEngine.set_sampling: expected SamplingParams, got {type(sampling).__name__}")
        if sampling.penalized:
            raise NotImplementedError("WeightOnlyDecodeEngine: a penalised request (repetition / presence / frequency penalty or logit_bias) "
                                      "is not served; DecodeEngine serves it for QLinear models")
        if self._sampler is None:
            self._sampler = SampleLaunch(self.logits, self.pos, self.tok, self.cache_len)
        self._sampler.set_rows([sampling], [check_stream(stream)])
        return self

    @torch.no_grad()
    def sample(self) -> torch.Tensor:
        """mq_sample on self.logits into self.tok: token n = position() of the sequence under the request of set_sampling (the draw
        index DecodeEngine.sample uses).  step() with no argument then consumes it."""
        if self._sampler is None:
            self.set_sampling(SamplingParams(temperature=0.0))
        with torch.cuda.device(self.dev):
            self._sampler.launch()
        return self.tok

    def _start_sequence(self, ids: List[int]):
        self.reset()
        if len(ids) > 1:
            self.prefill(ids)
        else:
            for t in ids:
                self.step(t)

    @torch.no_grad()
    def generate(self, context_ids, max_new_tokens: int, eos_token_id=None, sampling: Optional[SamplingParams] = None, stream: int = 0):
        """Context encoding by prefill(), then per new token: argmax of the logits (greedy, the default) or, with sampling=, a seeded draw
        on the device by mq_sample from the engine's logits row -- token n of the sequence is drawn at index n, as DecodeEngine.generate
        counts it, so the ids depend on (context, sampling, stream) only, captured or not.  Stops at an EOS (None, one id or several),
        after max_new_tokens, or when the cache is full.  Returns context + new ids."""
        ids = [int(t) for t in context_ids]
        if not ids or len(ids) + max_new_tokens > self.cache_len:
            raise ValueError(f"WeightOnlyDecodeEngine.generate: {len(ids)} context tokens + {max_new_tokens} new ones need 1 .. {self.cache_len} positions")
        if sampling is not None:
            self.set_sampling(sampling, stream)
        eos = _eos_set(eos_token_id)
        self._start_sequence(ids)
        out = list(ids)
        for made in range(1, max_new_tokens + 1):
            if sampling is not None:
                self.sample()
            else:
                torch.argmax(self.logits, dim=-1, keepdim=True, out=self.tok)
            nxt = int(self.tok.item())
            out.append(nxt)
            if nxt in eos or made == max_new_tokens or self._host_pos >= self.cache_len:
                break
            self.step()
        return out
