"""GPU: the decode step's attention launches against an exact oracle (oracle.decode_attention_step: row `pos` of attention_sim with exact
integer contractions) at long caches, up to the largest cache_len each launch admits (DecodeEngine.max_cache_len).

Each attention launch runs on its own with an explicit variant -- mq_decode_attention_oproj at 256 and 1024 threads, mq_decode_attention
with 1 split and with LONG_SPLITS -- on test-owned caches of that variant's largest length, filled so that the softmax sits where
rounding matters.  What must hold, per case:
  1. the k / v bytes appended at `pos` are the oracle's, and no other cache byte moves;
  2. (four launches) o_proj's accumulators are the exact int64 sums over the launch's own int8 output image;
  3. every output index is within one step of the oracle driven by the fp32 softmax (attention_sim's order);
  4. every output index lies in the range the float64 oracle allows once each probability index may take any value its pre-rounding
     value reaches within the fp32 error bound of the kernel's softmax (_p_index_bounds: derived from T and the documented order).
The number of output indices that differ from the fp32 oracle is printed per case."""
import ctypes
import dataclasses
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import mq_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
U = 2.0 ** -24                                    # unit roundoff of fp32
GEOMS = {32: (8, 2), 64: (4, 4), 128: (4, 1), 256: (4, 2)}        # head_dim -> (heads, kv_heads): GQA, MHA, MQA, GQA
VARIANTS = ("ao256", "ao1024", "attn1", "attn_split")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _model(dev, D):
    """One-layer model of the given attention geometry, calibrated, with the attention QMatMuls on fixed grids (pv input: set later)."""
    import mobilequant_amd as mq
    from mobilequant_amd import llama
    from mobilequant_amd.calibration import get_act_range
    from mobilequant_amd.llama import LlamaForCausalLM, LlamaShape
    H, KV = GEOMS[D]
    shape = LlamaShape(hidden=256, layers=1, heads=H, kv_heads=KV, head_dim=D, ffn=512, vocab=64, max_pos=64)
    m = LlamaForCausalLM(shape)
    m.reset_parameters(seed=3, std=0.08)
    m = m.to(dev).eval().requires_grad_(False)
    g = torch.Generator().manual_seed(1)
    act = get_act_range(m, [torch.randint(0, shape.vocab, (1, 32), generator=g)])
    a8 = mq.QuantConfig(bitwidth=8)
    mq.create_sim_qmodel(m, mq.QuantConfig(bitwidth=8), a8)
    for n, mod in m.named_modules():
        if isinstance(mod, mq.QLinear) and ("w2" in n or "o_proj" in n):
            mod.output_quantizer.qcfg.bitwidth = 16
        elif isinstance(mod, (mq.QRMSNorm, mq.QLayerNorm)):
            mod.input_quantizer.qcfg.bitwidth = 16
            mod.weight_quantizer.qcfg.bitwidth = 16
    mq.set_scale_and_offset(m, act, "buffer")
    at = m.layers[0].self_attn
    for q, bits, lo, hi in ((at.qk_bmm.input_quantizer, 8, -4.0, 4.0), (at.qk_bmm.input2_quantizer, 8, -4.5, 4.5),
                            (at.qk_bmm.output_quantizer, 16, -60.0, 60.0), (at.pv_bmm.input2_quantizer, 8, -4.0, 4.0),
                            (at.pv_bmm.output_quantizer, 8, -1.5, 1.5)):
        q.qcfg.bitwidth = bits
        q.set_scale_offset_from_minmax(torch.tensor(lo), torch.tensor(hi), "buffer", dev)
    cos, sin = llama.rope_tables(dataclasses.replace(shape, max_pos=32768))      # max_pos >= every cache_len below
    m.cos, m.sin = cos.to(dev), sin.to(dev)
    return m


def _oracle_grid(q):
    return O.quantizer_oracle_from(float(q.scale.reshape(-1)[0]), float(q.offset.reshape(-1)[0]), q.qmin, q.qmax)


class _Rig:
    """Both chains' engines on one model, their attention argument blocks, and the oracle's view of the grids."""

    def __init__(self, m, dev, pv_bits):
        from mobilequant_amd.decode import DecodeEngine
        from mobilequant_amd.quantization import qmodule as Q
        at = m.layers[0].self_attn
        pa = at.pv_bmm.input_quantizer
        pa.qcfg.bitwidth = pv_bits
        pa.set_scale_offset_from_minmax(torch.tensor(0.0), torch.tensor(1.0), "buffer", dev)
        self.e4 = DecodeEngine(m, cache_len=16, prefetch=0.0)
        self.e5 = DecodeEngine(m, cache_len=16, launches=5, attn_splits=1, prefetch=0.0)
        assert self.e4.launches == 4 and self.e5.launches == 5
        self.m, self.dev, self.s = m, dev, m.shape
        qk, pv = at.qk_bmm, at.pv_bmm
        self.qk = tuple(_oracle_grid(q) for q in (qk.input_quantizer, qk.input2_quantizer, qk.output_quantizer))
        self.pv = tuple(_oracle_grid(q) for q in (pv.input_quantizer, pv.input2_quantizer, pv.output_quantizer))
        g_o = at.o_proj.input_quantizer if at.o_proj.input_quantizer is not None else (
            pv.output_quantizer if Q._static_per_tensor(pv.output_quantizer, 8) else at.o_proj._input_grid)    # (DecodeEngine._attention_grids)
        self.o_in = _oracle_grid(g_o)
        o_w, op = self.e4.oproj_images[0]
        self.w_nk = o_w.permute(1, 0, 2).reshape(self.s.hidden, -1).cpu().numpy()
        self.w_zp = op.w_zp.cpu().numpy()
        self.out_q = torch.zeros(self.s.heads * self.s.head_dim, dtype=torch.int8, device=dev)

    def cache_len(self, variant):
        from mobilequant_amd.decode import DecodeEngine
        D = self.s.head_dim
        return {"ao256": DecodeEngine.max_cache_len(4, D, 256), "ao1024": DecodeEngine.max_cache_len(4, D, 1024)}.get(
            variant, DecodeEngine.max_cache_len(5, D))

    def run(self, variant, CL, pos, keys, values, qkv):
        """One attention launch at position pos over test-owned caches of CL positions: keys / values [kv, CL, D] int8 (logical layout;
        positions >= pos hold garbage the launch must not read).  Returns (k cache, logical v cache, out_q, o_acc or None) after it."""
        from mobilequant_amd import _lib
        s, dev = self.s, self.dev
        KV, D = s.kv_heads, s.head_dim
        four = variant.startswith("ao")
        eng = self.e4 if four else self.e5
        kc = keys.clone()
        vc = values.view(KV, CL // 16, 16, D).permute(0, 1, 3, 2).contiguous() if four else values.clone()
        eng.qkv.copy_(qkv)
        eng.pos.fill_(pos)
        a = type(eng.phases[1][1]).from_buffer_copy(eng.phases[1][1])
        a.k_cache, a.v_cache, a.cache_len = kc.data_ptr(), vc.data_ptr(), CL
        st = torch.cuda.current_stream().cuda_stream
        if four:
            eng.rope_row.copy_(torch.cat([eng.cos[pos], eng.sin[pos]]))   # (what mq_decode_embed stages at the start of a token)
            eng.o_acc.zero_()                                             # (cleared by the q|k|v launch in the chain)
            self.out_q.fill_(99)
            a.out_q, a.threads = self.out_q.data_ptr(), 1024 if variant == "ao1024" else 256
            _lib.call("mq_decode_attention_oproj", ctypes.byref(a), st)
            torch.cuda.synchronize()
            vlog = vc.permute(0, 1, 3, 2).reshape(KV, CL, D)
            return kc, vlog, self.out_q.clone(), eng.o_acc.clone()
        eng.attn_q.fill_(99)
        eng.attn_ticket.zero_()
        a.nsplit = eng.LONG_SPLITS if variant == "attn_split" else 1
        _lib.call("mq_decode_attention", ctypes.byref(a), st)
        torch.cuda.synchronize()
        return kc, vc, eng.attn_q.clone(), None


def _p_index_bounds(p_t64, scores, pa, T):
    """Lowest / highest probability index the kernels' fp32 softmax can produce, per head and position, around the float64 oracle.
    The kernels evaluate e_t = expf(fl(s_t - max)), S = sum_t e_t (thread j adds e_j, e_{j+256}, ... in order, then a 6-level DPP tree per
    wave and (w0 + w1) + (w2 + w3): every term passes through at most n = ceil(T / 256) + 7 roundings), p_t = fl(e_t / S), and the index
    rint(p_t / s) + o with the IEEE quotient.  Relative errors (u = 2^-24): fl(s_t - max) moves the exponent by <= u |s_t - max|, expf is
    within 1 ulp (<= 2u relative: HIP device math), so e_t carries a_t <= 2u + u |s_t - max|; S carries <= max_t a_t + gamma_n (1 + max_t
    a_t), gamma_n = n u / (1 - n u); each division one u.  The index of t* = p* / s can only differ from rint(t*) where t* lies within
    eps_t t* of a rounding boundary, eps_t = that sum (+1 % for second-order terms, + the float64 oracle's own 1e-12)."""
    n = math.ceil(T / 256) + 7
    gamma = n * U / (1 - n * U)
    x = np.abs(scores.astype(np.float64) - scores.max(axis=-1, keepdims=True).astype(np.float64))
    a_t = 2 * U + U * x
    a_max = a_t.max(axis=-1, keepdims=True)
    eps = (a_t + a_max + gamma * (1 + a_max) + 2 * U) * 1.01 + 1e-12
    idx = lambda t: np.clip(np.rint(t) + np.float64(F32(pa.offset)), pa.qmin, pa.qmax).astype(np.int64)   # noqa: E731  (monotone in t)
    return idx(p_t64 * (1 - eps) - 1e-30), idx(p_t64 * (1 + eps) + 1e-30)


def _fill(kind, gen, dev, KV, CL, D, H, pos, hot_row):
    """(keys, values [kv, CL, D] int8; q scale) for a named content.  Positions >= pos get random bytes too (never read)."""
    rnd = lambda lo, hi: torch.randint(lo, hi, (KV, CL, D), generator=gen, device=dev, dtype=torch.int8)      # noqa: E731
    keys, values = rnd(-128, 128), rnd(-128, 128)
    if kind in ("hot_first", "hot_mid", "hot_new", "saturate"):
        keys[:, :pos] = rnd(-8, 9)[:, :pos]                             # small keys: scores near zero ...
    if kind == "flat":
        keys[:, :pos] = keys[:, :1]                                     # identical keys: a flat softmax over the cached positions
    elif kind == "hot_first":
        keys[:, 0] = hot_row
    elif kind == "hot_mid":
        keys[:, pos // 2] = hot_row
    elif kind == "saturate":                                            # ... or at either end of the qk output grid
        sign = torch.randint(0, 2, (KV, CL, 1), generator=gen, device=dev, dtype=torch.int8) * 2 - 1
        keys[:, :pos] = (hot_row[:, None, :].to(torch.int16) * sign.to(torch.int16)).clamp(-127, 127).to(torch.int8)[:, :pos]
    elif kind == "v_zero":
        values[:, :pos] = 0
    elif kind == "v_extreme":
        values[:, :pos] = torch.where(rnd(0, 2) > 0, 127, -128).to(torch.int8)[:, :pos]
    return keys, values


def _case(rig, variant, pos, kind, seed, tally):
    s, dev = rig.s, rig.dev
    H, KV, D = s.heads, s.kv_heads, s.head_dim
    CL = rig.cache_len(variant)
    assert 0 <= pos < CL
    gen = torch.Generator(device=dev).manual_seed(seed)
    qkv = torch.randn((H + 2 * KV) * D, generator=gen, device=dev) * 1.5
    cos, sin = rig.e4.cos[pos].cpu().numpy(), rig.e4.sin[pos].cpu().numpy()
    q_np = qkv[:H * D].cpu().numpy()
    # the hot key of each KV group: the sign pattern of its first head's RoPE'd query image (a score at the top of the qk output grid)
    sq = O._index(O.rope_partial(q_np.reshape(H, 1, D), cos[None], sin[None])[:, 0], rig.qk[0]) - F32(rig.qk[0].offset)
    hot = torch.from_numpy(np.where(sq[::H // KV] >= 0, 127, -127).astype(np.int8)).to(dev)
    if kind == "hot_new":                                              # the new key IS the group's first query: its score comes from registers
        qkv[H * D:(H + KV) * D] = qkv[:H * D].view(KV, H // KV, D)[:, 0].reshape(-1)
    keys, values = _fill(kind, gen, dev, KV, CL, D, H, pos, hot)
    kc, vc, out_q, o_acc = rig.run(variant, CL, pos, keys, values, qkv)
    qkv_np = qkv.cpu().numpy()
    k_np, v_np = keys.cpu().numpy(), values.cpu().numpy()
    want = O.decode_attention_step(q_np, qkv_np[H * D:(H + KV) * D], qkv_np[(H + KV) * D:], k_np, v_np, pos, cos, sin, H, KV,
                                   rig.qk, rig.pv, rig.o_in)
    what = (variant, D, rig.pv[0].bitwidth, pos, kind)
    # 1. the appended bytes, and nothing else written
    k_want, v_want = k_np.copy(), v_np.copy()
    k_want[:, pos], v_want[:, pos] = want["k_new"], want["v_new"]
    assert np.array_equal(kc.cpu().numpy(), k_want), what
    assert np.array_equal(vc.cpu().numpy(), v_want), what
    got = out_q.cpu().numpy().astype(np.int64)
    # 2. o_proj's split-K accumulators: the exact sums over the launch's own image
    if o_acc is not None:
        assert np.array_equal(o_acc.cpu().numpy().astype(np.int64), O.oproj_int_sums(rig.w_nk, rig.w_zp, out_q.cpu().numpy())), what
    # 3. within one step of the fp32 oracle
    ref = want["out_q"].astype(np.int64)
    assert np.abs(got - ref).max() <= 1, (what, int(np.abs(got - ref).max()))
    # 4. inside what the float64 oracle allows under the fp32 error bound of the softmax
    lo, hi = _p_index_bounds(want["p_t64"], want["scores"], rig.pv[0], pos + 1)
    acc_lo, acc_hi = O.decode_pv_sums(lo, want["iv"], rig.pv[0], rig.pv[1], p_hi=hi)
    out_lo = O.decode_pv_output(acc_lo, *rig.pv, rig.o_in)[1].astype(np.int64)
    out_hi = O.decode_pv_output(acc_hi, *rig.pv, rig.o_in)[1].astype(np.int64)
    bad = (got < out_lo) | (got > out_hi)
    assert not bad.any(), (what, int(bad.sum()), np.nonzero(bad)[0][:8], got[bad][:8], out_lo[bad][:8], out_hi[bad][:8])
    n_diff, n_amb = int((got != ref).sum()), int((hi != lo).sum())
    tally.append((what, n_diff, n_amb))
    print(f"{variant:10s} D={D:3d} pv_bits={rig.pv[0].bitwidth:2d} pos={pos:5d} {kind:9s}: {n_diff} of {got.size} output indices differ "
          f"from the fp32 oracle ({n_amb} of {lo.size} probability indices within the bound of a boundary)")


POSITIONS = (1023, 1024, 1025, 2048, 4096, 8192, 16384)
STRUCTURED = ("flat", "hot_first", "hot_mid", "hot_new", "saturate", "v_zero", "v_extreme")


@pytest.mark.parametrize("D", [32, 64, 128, 256])
def test_decode_attention_launches_against_the_exact_oracle_at_long_caches(dev, D):
    m = _model(dev, D)
    tally = []
    for bits in (16, 12, 8):
        rig = _Rig(m, dev, bits)
        for vi, variant in enumerate(VARIANTS):
            last = rig.cache_len(variant) - 1                            # the full cache at the variant's largest cache_len
            seed = 1000 * D + 100 * bits + 10 * vi
            if bits == 16:
                for pos in POSITIONS + (last,):
                    _case(rig, variant, pos, "random", seed + pos, tally)
                for kind in STRUCTURED:
                    _case(rig, variant, 16384, kind, seed + 1, tally)
                for kind in ("flat", "hot_new"):
                    _case(rig, variant, last, kind, seed + 2, tally)
            else:
                for pos, kind in ((1025, "random"), (last, "random"), (16384, "flat")):
                    _case(rig, variant, pos, kind, seed + 3, tally)
    print(f"D={D}: {len(tally)} cases, {sum(t[1] for t in tally)} output indices off the fp32 oracle by one step in all")


def test_prefill_then_steps_at_long_context_match_the_module_chain(dev):
    """One layer: prefill a 4 096-token context through the fused prefill path, take 8 steps; the logits of every step are those of the
    module chain's forward over the same 4 104 tokens within test_gpu_round2's bars() budget (a systematic one-step bias anywhere in
    the step moves the median by orders of magnitude)."""
    from mobilequant_amd import llama
    from mobilequant_amd.decode import DecodeEngine
    m = _model(dev, 64)
    at = m.layers[0].self_attn
    at.pv_bmm.input_quantizer.qcfg.bitwidth = 16
    at.pv_bmm.input_quantizer.set_scale_offset_from_minmax(torch.tensor(0.0), torch.tensor(1.0), "buffer", dev)
    S, n = 4096, 8
    ids = torch.randint(0, m.shape.vocab, (S + n,), generator=torch.Generator().manual_seed(4))
    eng = DecodeEngine(m, cache_len=S + 16)
    assert eng.launches == 4 and eng.graph is None
    with torch.no_grad():
        want = m(ids[None].to(dev))[0, S - 1:].float().cpu().numpy()       # logits behind the context and behind each new token
    assert llama.fuse_decoder_layer(m) == 1
    eng.reset()
    got = [eng.prefill(ids[:S].tolist()).cpu().numpy().copy()]
    assert int(eng.pos.item()) == S
    for t in ids[S:S + n - 1].tolist():
        got.append(eng.step(int(t)).cpu().numpy().copy())
    got = np.stack(got)
    span = float(np.ptp(want))
    d = np.abs(got - want[:n]) / span
    assert d.max() <= 0.02 and np.quantile(d, 0.99) <= 0.006 and np.median(d) <= 5e-6, (d.max(), np.quantile(d, 0.99), np.median(d))


def test_direct_launch_after_capture_runs_the_base_variant(dev):
    """capture() records the long-cache graph last; the launch records must hold the base variant again afterwards, so that a direct
    launch below long_from runs the 256-thread kernel (four launches) / the unsplit attention (five)."""
    from mobilequant_amd.decode import DecodeEngine
    m = _model(dev, 64)
    m.layers[0].self_attn.pv_bmm.input_quantizer.qcfg.bitwidth = 16
    m.layers[0].self_attn.pv_bmm.input_quantizer.set_scale_offset_from_minmax(torch.tensor(0.0), torch.tensor(1.0), "buffer", dev)
    eng = DecodeEngine(m, cache_len=2048, prefetch=0.0)
    e5 = DecodeEngine(m, cache_len=2048, launches=5, prefetch=0.0)
    assert eng.launches == 4 and len(eng._variants()) == 2 and len(e5._variants()) == 2
    for e in (eng, e5):
        e.fill_cache_random(100, seed=2)
        e.capture()
        assert e.graph_long is not None
    assert [a.threads for kind, a in eng.phases if kind == "attn_oproj"] == [256]
    assert [a.nsplit for kind, a in e5.phases if kind == "attn"] == [1]
    # a direct launch of the record after capture() is the captured short-cache step, bit for bit
    ref = eng.step(5).clone()                                          # (graph replay at position 100)
    eng.set_position(100)
    eng.tok.fill_(5)
    eng._launch()
    torch.cuda.synchronize()
    assert torch.equal(eng.logits, ref)
