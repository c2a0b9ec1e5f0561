"""Oracle of the W4A16 decode step, numpy, built on tests/w4a16_ref.py.

One chain, two arithmetics: dt = float64 is the oracle -- the linear contract through R.linear64 (x16 = fp16(y), exact products, float64
sums), norms, RoPE, attention and the gated product in float64; dt = float32 is the emulation of the same chain in fp32 arithmetic (numpy
fp32 operations, fp32-accumulating matrix products), whose distance from the oracle is the reference's own sensitivity to rounding and
summation order: the tolerances of tests/test_gpu_w4a16_decode.py are multiples of it, measured on the CPU, never on the code under test.
"""
import math

import numpy as np

import w4a16_ref as R

F16, F32, F64 = np.float16, np.float32, np.float64


# ---- the pieces ------------------------------------------------------------------------------------------------------------------------
def norm(x, kind, w, b, eps, dt=F64):
    """HFRMSNorm: w * (x * rsqrt(mean(x^2) + eps)) (+ b); nn.LayerNorm: (x - mu) * rsqrt(var + eps) * w + b (biased variance)."""
    x = np.asarray(x, dt)
    if kind == "rmsnorm":
        y = x * (dt(1.0) / np.sqrt(np.mean(x * x, dtype=dt) + dt(eps)))
        y = y if w is None else np.asarray(w, dt) * y
    else:
        mu = np.mean(x, dtype=dt)
        d = x - mu
        y = d * (dt(1.0) / np.sqrt(np.mean(d * d, dtype=dt) + dt(eps)))
        y = y if w is None else y * np.asarray(w, dt)
    return (y if b is None else y + np.asarray(b, dt)).astype(dt)


def linear(x, lin, dt=F64):
    """The linear contract on one row.  lin = (w16 [N, K] fp16, bias fp32 or None)."""
    w16, bias = lin
    if dt == F64:
        return R.linear64(np.asarray(x, F64)[None, :], w16, bias)[0][0]
    y = R.x16(np.asarray(x, F32)).astype(F32) @ w16.astype(F32).T
    return (y if bias is None else y + np.asarray(bias, F32)).astype(F32)


def rope(x, cos, sin, dt=F64):
    """llama.apply_rope on [heads, D] at one position: the first rot = len(cos) dims rotate (rotate-half), the rest passes through."""
    x = np.asarray(x, dt)
    rd = len(cos)
    xr, h = x[:, :rd], rd // 2
    rot = np.concatenate((-xr[:, h:], xr[:, :h]), axis=1)
    out = x.copy()
    out[:, :rd] = xr * np.asarray(cos, dt)[None, :] + rot * np.asarray(sin, dt)[None, :]
    return out


def attention(q, k, v, dt=F64):
    """q [H, D] (roped), k / v [KV, n, D] (positions 0 .. pos, k roped) -> o [H, D]."""
    q, k, v = np.asarray(q, dt), np.asarray(k, dt), np.asarray(v, dt)
    H, D = q.shape
    rep = H // k.shape[0]
    o = np.empty((H, D), dt)
    for h in range(H):
        s = (k[h // rep] @ q[h]) / dt(math.sqrt(D))
        p = np.exp(s - s.max())
        o[h] = (p / p.sum(dtype=dt)) @ v[h // rep]
    return o


def act(a, kind, dt=F64):
    a = np.asarray(a, dt)
    if kind == "silu":
        return a / (dt(1.0) + np.exp(-a))
    erf = np.vectorize(math.erf, otypes=[F64])
    return (a * dt(0.5) * (dt(1.0) + erf(a.astype(F64) * math.sqrt(0.5)).astype(dt))).astype(dt)


def gated(a, b, kind, dt=F64):
    return (act(a, kind, dt) * np.asarray(b, dt)).astype(dt)


def ulp32(v):
    """One fp32 ulp at |v| (float64 in)."""
    a = np.maximum(np.abs(np.asarray(v, F64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(a)) - 23)


def fp16_boundary_distance(y64):
    """For every element of y64 (float64, what a norm prologue hands to the fp16 conversion): its distance to the nearest fp16 ROUNDING
    BOUNDARY (the midpoint of two neighbouring fp16 numbers), in fp32 ulps at that magnitude.  Far from a boundary the kernel's fp32 value
    and the oracle's float64 value round to the same fp16 number."""
    y = np.abs(np.asarray(y64, F64))
    lo = y.astype(F16)
    with np.errstate(over="ignore"):
        up, dn = np.nextafter(lo, F16(np.inf)).astype(F64), np.nextafter(lo, F16(-np.inf)).astype(F64)
    lo = lo.astype(F64)
    d = np.minimum(np.abs(y - (lo + up) / 2), np.abs(y - (lo + dn) / 2))
    return d / ulp32(y)


# ---- a model ---------------------------------------------------------------------------------------------------------------------------
def _np(t):
    return None if t is None else t.detach().cpu().numpy()


class Chain:
    """The decode step of a weight-only LlamaForCausalLM on numpy weights.  from_float(): the float model quantised by the oracle's own
    grid and index (R.grid_from_minmax, R.stored); from_packed(): the buffers of a model create_weight_only_qmodel made."""

    def __init__(self, shape, embed, layers, final_norm, lm_head, cos, sin):
        self.shape, self.embed, self.layers, self.final_norm, self.lm_head, self.cos, self.sin = shape, embed, layers, final_norm, lm_head, cos, sin

    @staticmethod
    def _norm_of(m):
        kind = "layernorm" if type(m).__name__ == "LayerNorm" else "rmsnorm"
        return (kind, _np(m.weight), _np(getattr(m, "bias", None)), float(m.eps))

    @classmethod
    def _build(cls, model, lin_of):
        s = model.shape
        layers = []
        for layer in model.layers:
            a, m = layer.self_attn, layer.mlp
            layers.append(dict(n1=cls._norm_of(layer.input_layernorm), n2=cls._norm_of(layer.post_attention_layernorm),
                               q=lin_of(a.q_proj), k=lin_of(a.k_proj), v=lin_of(a.v_proj), o=lin_of(a.o_proj), w1=lin_of(m.w1), w2=lin_of(m.w2),
                               w3=lin_of(m.w3)))
        emb = _np(model.embed_tokens.weight).astype(F32)
        if s.embed_scale:
            emb = (emb * F32(s.hidden ** 0.5)).astype(F32)
        return cls(s, emb, layers, cls._norm_of(model.norm), (_np(model.lm_head.weight).astype(F32), _np(model.lm_head.bias)), _np(model.cos), _np(model.sin))

    @classmethod
    def from_float(cls, model, group_size, is_symmetric=False):
        def lin_of(m):
            w = _np(m.weight).astype(F32)
            s, o = R.grid_from_minmax(w, is_symmetric, group_size)
            u, s16, z16 = R.stored(w, s, o, is_symmetric, group_size)
            return (R.w16(u, s16, z16, group_size), _np(m.bias))
        return cls._build(model, lin_of)

    @classmethod
    def from_packed(cls, model):
        def lin_of(m):
            return (R.w16(R.unpack(_np(m.qweight)), _np(m.scales).astype(F16), _np(m.zeros).astype(F16), m.group_size), _np(m.bias))
        return cls._build(model, lin_of)

    def new_cache(self, T, dt=F64):
        s = self.shape
        return [(np.zeros((s.kv_heads, T, s.head_dim), dt), np.zeros((s.kv_heads, T, s.head_dim), dt)) for _ in self.layers]

    def step(self, tok, pos, cache, dt=F64):
        """One token at position pos over cache (written at pos): logits [vocab] in dt."""
        s = self.shape
        H, KV, D = s.heads, s.kv_heads, s.head_dim
        x = self.embed[tok].astype(dt)
        for L, (kc, vc) in zip(self.layers, cache):
            y = norm(x, *L["n1"], dt=dt)
            q = rope(linear(y, L["q"], dt).reshape(H, D), self.cos[pos], self.sin[pos], dt)
            kc[:, pos] = rope(linear(y, L["k"], dt).reshape(KV, D), self.cos[pos], self.sin[pos], dt)
            vc[:, pos] = np.asarray(linear(y, L["v"], dt), dt).reshape(KV, D)
            o = attention(q, kc[:, :pos + 1], vc[:, :pos + 1], dt)
            x = (x + np.asarray(linear(o.reshape(-1), L["o"], dt), dt)).astype(dt)
            y2 = norm(x, *L["n2"], dt=dt)
            h = gated(linear(y2, L["w1"], dt), linear(y2, L["w3"], dt), s.hidden_act, dt)
            x = (x + np.asarray(linear(h, L["w2"], dt), dt)).astype(dt)
        w, b = self.lm_head
        logits = w.astype(dt) @ norm(x, *self.final_norm, dt=dt)
        return (logits if b is None else logits + np.asarray(b, dt)).astype(dt)

    def run(self, ids, dt=F64, T=None):
        """Teacher-forced steps from an empty cache: (logits [len(ids), vocab], cache)."""
        cache = self.new_cache(T or len(ids), dt)
        return np.stack([self.step(int(t), p, cache, dt) for p, t in enumerate(ids)]), cache

    def greedy(self, prompt, n_new, dt=F64):
        """(ids, smallest top-2 gap over the steps that chose a token): prompt + n_new greedy tokens."""
        ids = [int(t) for t in prompt]
        cache = self.new_cache(len(ids) + n_new, dt)
        logits, gap = None, math.inf
        for p in range(len(ids) + n_new - 1):
            logits = self.step(ids[p], p, cache, dt)
            if p >= len(prompt) - 1:
                top = np.sort(logits)[-2:]
                gap = min(gap, float(top[1] - top[0]))
                ids.append(int(np.argmax(logits)))
        return ids, gap
