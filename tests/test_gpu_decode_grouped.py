"""GPU: per-group weight grids on the decode path (csrc/mq_decode_grouped.hip; DecodeEngine / BatchDecodeEngine).

Launch level, every role of a five-launch GEMV (ready int8 image + residual; RMS / LayerNorm prologue with three q|k|v segments; the
gate with QSiLU / QGELU), int8 and packed 4-bit streams, symmetric and asymmetric grids, group sizes 64 / 128 / 256, B = 1 / 3 / 8:
  * grids off: y equals mq_w8a8_linear_grouped on the same image bit for bit (at a ragged N, which that kernel refuses, this file's own
    replay: exact integer brackets, one correctly rounded fp32 fma per group in ascending g, then + bias);
  * grids on: y / the gate's int8 indices equal the per-channel batched launch's epilogue fed the same fp32 values (zero weights, the
    values as its bias: its own code, op for op);
  * row b of a batched launch equals the B = 1 launch of that row; canaries behind every output row stay untouched.
The norm prologue's images come from fp32 reductions this file does not replay: an identity-row probe observes them, through the
per-channel batched launch and through the grouped one, and they must agree.
Engines: DecodeEngine on small TinyLlama / StableLM-2 / Gemma-shaped grouped models against the module graph's forward (the bound of
test_decode_engine_w4a8_matches_module_graph), eager steps against graph replays, and every BatchDecodeEngine slot against the single
engine bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

F32 = np.float32
CANARY_F = -1.25e30
CANARY_Q = 77
PAD = 16                                           # canary floats / bytes behind every output row


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _lib():
    from mobilequant_amd import _lib as L
    return L


def _st():
    return torch.cuda.current_stream().cuda_stream


def _t(a, dev, keep, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    if dtype is not None:
        t = t.to(dtype)
    keep.append(t)
    return t


def _grid(dev, keep, s=None, o=None, qmin=0.0, qmax=255.0):
    L = _lib()
    if s is None:
        return L.MqGrid(None, None, 0.0, 0.0)
    st, ot = _t(np.array([s], F32), dev, keep), _t(np.array([o], F32), dev, keep)
    return L.MqGrid(st.data_ptr(), ot.data_ptr(), float(qmin), float(qmax))


def _consts(a, dev, keep):
    L = _lib()
    grids = [a.norm_in, a.a_grid, a.out_grid[0], a.out_grid[1], a.out_grid[2], a.gate_mid, a.gate_actout, a.gate_out, a.o_out]
    out = torch.zeros(64, device=dev)
    L.call("mq_decode_pack_grids", (L.MqGrid * 9)(*grids), 9, out.data_ptr(), _st())
    keep.append(out)
    a.consts = out.data_ptr()


# ---- oracle ------------------------------------------------------------------------------------------------------------------------
def _fma32(a, b, c):
    """Correctly rounded fp32 fma of fp32 arrays: the product is exact in fp64, TwoSum gives the sum's error, and the one case where
    rounding the fp64 sum to fp32 differs from rounding the exact sum -- the sum sitting on an fp32 midpoint -- is resolved by its sign."""
    a64, b64, c64 = a.astype(np.float64), b.astype(np.float64), c.astype(np.float64)
    p = a64 * b64
    s = p + c64
    bp = s - p
    e = (p - (s - bp)) + (c64 - bp)
    r = s.astype(F32)
    r64 = r.astype(np.float64)
    nb = np.nextafter(r, np.where(s > r64, np.inf, -np.inf).astype(F32))
    nb64 = nb.astype(np.float64)
    mid = (s != r64) & ((r64 + nb64) * 0.5 == s) & (e != 0)
    return np.where(mid & (np.sign(e) == np.sign(nb64 - r64)), nb, r)


def _replay(img, wb, gs, alpha, cw, t, bias):
    """[B, N] fp32: exact int32 brackets P_g + cw A_g + t, folded acc = fma((float)bracket, alpha, acc) from 0 in ascending g, + bias."""
    B, K = img.shape
    N, G = wb.shape[0], K // gs
    i3 = img.reshape(B, G, gs).astype(np.int64)
    P = np.einsum("bgk,ngk->bgn", i3, wb.reshape(N, G, gs).astype(np.int64))
    br = P + cw.astype(np.int64)[None] * i3.sum(-1)[:, :, None] + t.astype(np.int64)[None]
    assert np.abs(br).max() < 2 ** 31
    acc = np.zeros((B, N), F32)
    for g in range(G):
        acc = _fma32(br[:, g].astype(F32), np.broadcast_to(alpha[g], (B, N)).astype(F32), acc)
    return acc if bias is None else (acc + bias[None]).astype(F32)


def _gemm_oracle(dev, img, wb, gs, alpha, cw, t, bias):
    """mq_w8a8_linear_grouped on the same image and stored weights (4-bit: the nibbles as int8 values)."""
    from mobilequant_amd import ops
    B, K = img.shape
    G = K // gs
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    a_q = dv(img.astype(np.int8))
    a_gsum = a_q.view(B, G, gs).sum(-1, dtype=torch.int32).t().contiguous()
    y = ops.int8_linear_grouped(a_q, dv(wb.astype(np.int8)), gs, a_gsum, dv(alpha), dv(cw.astype(np.int32)), dv(t.astype(np.int32)),
                                None if bias is None else dv(bias))
    return y.cpu().numpy()


def _pre_grid(dev, img, wb, gs, alpha, cw, t, bias):
    N = wb.shape[0]
    if N % 128 == 0:
        return _gemm_oracle(dev, img, wb, gs, alpha, cw, t, bias)
    return _replay(img, wb, gs, alpha, cw, t, bias)


# ---- cases and launches ------------------------------------------------------------------------------------------------------------
def _weights(rng, N, K, gs, w4, sym):
    """Stored weights [N, K] (int8 index - 128 / symmetric index; 4-bit: unsigned nibbles) and cw [G, N] of that storage."""
    G = K // gs
    if w4:
        wb = rng.integers(0, 16, (N, K))
        cw = np.full((G, N), -8) if sym else -rng.integers(0, 16, (G, N))            # qmin - o_w
    else:
        wb = rng.integers(-128, 128, (N, K))
        cw = np.zeros((G, N), np.int64) if sym else 128 - rng.integers(0, 256, (G, N))
    return wb, cw


def _vectors(rng, wb, cw, gs, c_a):
    N, K = wb.shape
    wsum = wb.reshape(N, K // gs, gs).sum(-1).T
    t = np.ascontiguousarray(c_a * wsum + gs * c_a * cw)
    alpha = (rng.uniform(0.5, 2.0, cw.shape) * 2e-3).astype(F32)
    return alpha, t


class Launch:
    """One mq_decode_gemv_grouped / mq_decode_gemv_batch launch record over B rows, its buffers (with canaries) and what it wrote."""

    def __init__(self, dev, p, B, rows=None):
        from mobilequant_amd._lib import MqDecodeGemvArgs
        self.dev, self.p, self.keep = dev, p, []
        self.rows = list(range(B)) if rows is None else rows
        self.B = len(self.rows)
        K, N = p["K"], p["N"]
        a = MqDecodeGemvArgs()
        a.K, a.N = K, N
        k = self.keep
        if p["mode"] == "xq":
            self.x = _t(p["xq"][self.rows], dev, k)
            a.xq = self.x.data_ptr()
            self.xs = K
        else:
            self.x = _t(p["x"][self.rows], dev, k)
            a.x = self.x.data_ptr()
            self.xs = K
            a.norm_w = _t(p["norm_w"], dev, k).data_ptr()
            a.layernorm = int(p["mode"] == "ln")
            if p["mode"] == "ln":
                a.norm_bias = _t(p["norm_b"], dev, k).data_ptr()
            a.norm_in, a.eps = _grid(dev, k, *p["norm_in"], 0.0, 65535.0), 1e-5
        a.a_grid = _grid(dev, k, *p["a_grid"])
        self.a = a
        self.gate = p.get("gate") is not None
        NL = N // 2 if self.gate else N
        self.NL = NL
        self.ys = NL + PAD
        self.y = torch.full((self.B, self.ys), CANARY_F, device=dev)
        a.seg_end[0], a.seg_end[1] = p.get("seg_end", (N, N))
        if self.gate:
            self.gq = torch.full((self.B, self.ys), CANARY_Q, dtype=torch.int8, device=dev)
            a.gate_q, a.gate_act = self.gq.data_ptr(), p["gate"]
            a.out_grid[0], a.out_grid[1] = _grid(dev, k, *p["out"][0]), _grid(dev, k, *p["out"][1])
            a.gate_mid = _grid(dev, k, 1.0 / 255, 0.0) if p["gate"] == 0 else _grid(dev, k)
            a.gate_actout, a.gate_out = _grid(dev, k, 0.02, 128.0), _grid(dev, k, 0.01, 128.0)
        else:
            for i, gdef in enumerate(p.get("out") or ()):
                a.out_grid[i] = _grid(dev, k, *gdef) if gdef else _grid(dev, k)
            if p.get("resid") is not None:
                self.res = _t(np.concatenate([p["resid"][self.rows], np.zeros((self.B, PAD), F32)], 1), dev, k)
                a.resid = self.res.data_ptr()
        a.y = self.y.data_ptr()
        _consts(a, dev, k)

    def grouped(self, wstream, w4, gs, alpha, cw, t, bias):
        L = _lib()
        a, k = self.a, self.keep
        a.w, a.w4 = _t(wstream, self.dev, k).data_ptr(), int(w4)
        if bias is not None:
            a.bias = _t(bias, self.dev, k).data_ptr()
        b = L.MqDecodeGemvBatchArgs()
        b.g, b.batch, b.x_stride, b.y_stride, b.gate_stride = a, self.B, self.xs, self.ys, self.ys
        ga = L.MqDecodeGemvGroupedArgs()
        ga.b, ga.group_size = b, gs
        ga.alpha = _t(alpha, self.dev, k).data_ptr()
        ga.cw = _t(cw.astype(np.int32), self.dev, k).data_ptr()
        ga.t = _t(t.astype(np.int32), self.dev, k).data_ptr()
        from mobilequant_amd import ops
        ops.decode_gemv_grouped(ga)
        return self._out()

    def per_channel(self, w8, alpha, zp, ct, bias):
        L = _lib()
        a, k = self.a, self.keep
        a.w, a.w4 = _t(w8, self.dev, k).data_ptr(), 0
        a.alpha, a.w_zp, a.col_term = _t(alpha, self.dev, k).data_ptr(), _t(zp, self.dev, k).data_ptr(), _t(ct, self.dev, k).data_ptr()
        a.bias = _t(bias, self.dev, k).data_ptr() if bias is not None else None
        b = L.MqDecodeGemvBatchArgs()
        b.g, b.batch, b.x_stride, b.y_stride, b.gate_stride = a, self.B, self.xs, self.ys, self.ys
        L.call("mq_decode_gemv_batch", __import__("ctypes").byref(b), _st())
        return self._out()

    def _out(self):
        torch.cuda.synchronize()
        y = self.y.cpu().numpy()
        assert np.all(y[:, self.NL:] == CANARY_F), "a canary behind y changed"
        if not self.gate:
            return y[:, :self.NL].copy(), None
        gq = self.gq.cpu().numpy()
        assert np.all(gq[:, self.NL:] == CANARY_Q), "a canary behind gate_q changed"
        return y[:, :self.NL].copy(), gq[:, :self.NL].copy()


def _pack(wb, w4):
    from mobilequant_amd import ops
    if not w4:
        return wb.astype(np.int8)
    return ops.pack_w4(torch.from_numpy(wb.astype(np.uint8)).cuda()).cpu().numpy()


def _image(dev, p, B):
    """The int8 images the prologue builds: an identity-row probe through the per-channel batched launch and through the grouped one."""
    if p["mode"] == "xq":
        return p["xq"][:B].astype(np.int64)
    K = p["K"]
    q = dict(p, N=K, gate=None, out=None, seg_end=(K, K), resid=None)
    eye = np.eye(K, dtype=np.int8)
    pc, _ = Launch(dev, q, B).per_channel(eye, np.ones(K, F32), np.zeros(K, np.int32), np.zeros(K, np.int32), None)
    G = K // 64
    gr, _ = Launch(dev, q, B).grouped(eye, False, 64, np.ones((G, K), F32), np.zeros((G, K), np.int64), np.zeros((G, K), np.int64), None)
    assert np.array_equal(pc, gr), "the grouped launch's prologue built another image than the per-channel launch's"
    assert np.all(pc == np.rint(pc)) and np.abs(pc).max() <= 128
    return pc.astype(np.int64)


def _case(rng, mode, K, NL, B=8, gate_act=None):
    p = dict(mode=mode, K=K, N=2 * NL if gate_act is not None else NL, a_grid=(0.03, 131.0))
    if mode == "xq":
        p["xq"] = rng.integers(-128, 128, (B, K)).astype(np.int8)
        p["resid"] = rng.normal(0, 1, (B, NL)).astype(F32)
        p["out"] = [(0.05, 3.0, -32768.0, 32767.0)]
    else:
        p["x"] = (rng.normal(0, 1, (B, K)) * rng.uniform(0.5, 2.0, K)).astype(F32)
        p["norm_w"] = rng.uniform(0.5, 1.5, K).astype(F32)
        p["norm_b"] = rng.normal(0, 0.1, K).astype(F32)
        p["norm_in"] = (8.0 / 32768, 32768.0)
        if gate_act is None:
            s0, s1 = NL * 3 // 4, NL * 7 // 8
            p["seg_end"] = (s0, s1)
            p["out"] = [(0.04, 128.0), (0.05, 120.0), (0.03, 135.0)]
        else:
            p["gate"] = gate_act
            p["out"] = [(0.04, 128.0), (0.05, 120.0)]
    return p


def _check_launch(dev, p, wb, w4, gs, alpha, cw, t, bias):
    """Grids off against the oracle, grids on against the per-channel epilogue, batched rows against B = 1, canaries (in Launch)."""
    stream = _pack(wb, w4)
    B, N = 8, p["N"]
    img = _image(dev, p, B)
    want = _pre_grid(dev, img, wb, gs, alpha, cw, t, bias)            # [B, N] in front of the output grid(s)
    bare = dict(p, gate=None, out=None, resid=None, seg_end=(N, N))
    y0, _ = Launch(dev, bare, B).grouped(stream, w4, gs, alpha, cw, t, bias)
    assert np.array_equal(y0.view(np.int32), want.view(np.int32)), ("grids off", float(np.abs(y0 - want).max()))
    full, full3 = Launch(dev, p, B), None
    yg, qg = full.grouped(stream, w4, gs, alpha, cw, t, bias)
    rows3 = [1, 4, 6]
    y3, q3 = Launch(dev, p, 3, rows=rows3).grouped(stream, w4, gs, alpha, cw, t, bias)
    zeros = np.zeros((N, p["K"]), np.int8)
    for b in range(B):
        y1, q1 = Launch(dev, p, 1, rows=[b]).grouped(stream, w4, gs, alpha, cw, t, bias)
        assert np.array_equal(y1[0].view(np.int32), yg[b].view(np.int32)), ("B = 1 vs B = 8", b)
        # the per-channel launch's epilogue on the same values: zero weights, alpha 1, the values as its bias
        ye, qe = Launch(dev, p, 1, rows=[b]).per_channel(zeros, np.ones(N, F32), np.zeros(N, np.int32), np.zeros(N, np.int32), want[b].copy())
        assert np.array_equal(ye[0].view(np.int32), yg[b].view(np.int32)), ("epilogue", b)
        if qg is not None:
            assert np.array_equal(q1[0], qg[b]) and np.array_equal(qe[0], qg[b]), ("gate indices", b)
        if b in rows3:
            i = rows3.index(b)
            assert np.array_equal(y3[i].view(np.int32), yg[b].view(np.int32)), ("B = 3 vs B = 8", b)
            if qg is not None:
                assert np.array_equal(q3[i], qg[b])


MODES = [("xq", None), ("rms", None), ("ln", None), ("rms", 0), ("ln", 1)]
MODE_IDS = ["xq_resid", "rms_qkv", "ln_qkv", "gate_silu", "gate_gelu"]


@pytest.mark.parametrize("gs", [64, 128, 256])
@pytest.mark.parametrize("w4", [False, True], ids=["w8", "w4"])
@pytest.mark.parametrize("mode,gate", MODES, ids=MODE_IDS)
def test_launch_at_tinyllama_shapes(dev, mode, gate, w4, gs):
    """TinyLlama-1.1B rows: q|k|v 2048 -> 2048 | 256 | 256, w1|w3 2048 -> 2 x 5632, o_proj 2048 -> 2048 (xq + residual)."""
    rng = np.random.default_rng(1000 + gs + 7 * w4 + 31 * MODE_IDS.index(MODE_IDS[MODES.index((mode, gate))]))
    K = 2048
    NL = 5632 if gate is not None else (2560 if mode != "xq" else 2048)
    p = _case(rng, mode, K, NL, gate_act=gate)
    if mode != "xq" and gate is None:
        p["seg_end"] = (2048, 2304)
    sym = (gs == 128) == w4                                        # symmetric and asymmetric grids across the grid of cases
    wb, cw = _weights(rng, p["N"], K, gs, w4, sym)
    alpha, t = _vectors(rng, wb, cw, gs, int(rng.integers(-60, 61)))
    bias = rng.normal(0, 0.3, p["N"]).astype(F32) if mode != "xq" else None
    _check_launch(dev, p, wb, w4, gs, alpha, cw, t, bias)


@pytest.mark.parametrize("w4", [False, True], ids=["w8", "w4"])
@pytest.mark.parametrize("mode,gate", MODES, ids=MODE_IDS)
def test_launch_at_a_ragged_n(dev, mode, gate, w4):
    """N off every multiple of 128 (and of the rows per workgroup): the file's own replay of the fold is the oracle."""
    rng = np.random.default_rng(77 + 7 * w4 + 31 * MODE_IDS.index(MODE_IDS[MODES.index((mode, gate))]))
    K, gs = (5632, 256) if mode == "xq" else (1024, 64)
    NL = 333 if gate is not None else 461
    p = _case(rng, mode, K, NL, gate_act=gate)
    wb, cw = _weights(rng, p["N"], K, gs, w4, sym=False)
    alpha, t = _vectors(rng, wb, cw, gs, 17)
    bias = rng.normal(0, 0.3, p["N"]).astype(F32)
    _check_launch(dev, p, wb, w4, gs, alpha, cw, t, bias)


def test_one_group_per_row_is_the_per_channel_launch(dev):
    """group_size = K (one group spanning whole passes): the fold is one fma from zero, i.e. the per-channel epilogue's product --
    the grouped gate launch equals mq_decode_gemv_batch with w_zp = -cw and col_term = t, bit for bit."""
    rng = np.random.default_rng(5)
    K, NL = 2048, 5632
    p = _case(rng, "rms", K, NL, gate_act=0)
    wb, cw = _weights(rng, p["N"], K, K, False, sym=False)
    alpha, t = _vectors(rng, wb, cw, K, -23)
    bias = rng.normal(0, 0.3, p["N"]).astype(F32)
    yg, qg = Launch(dev, p, 8).grouped(wb.astype(np.int8), False, K, alpha, cw, t, bias)
    yp, qp = Launch(dev, p, 8).per_channel(wb.astype(np.int8), alpha[0], (-cw[0]).astype(np.int32), t[0].astype(np.int32), bias)
    assert np.array_equal(qg, qp) and np.array_equal(yg.view(np.int32), yp.view(np.int32))


# ---- engines -------------------------------------------------------------------------------------------------------------------------
GEOMS = {
    "llama": dict(hidden=256, heads=32, kv_heads=4, head_dim=64, ffn=512, vocab=160),
    "stablelm": dict(hidden=256, heads=4, kv_heads=4, head_dim=64, ffn=512, vocab=96, norm="layernorm", qkv_bias=True, rotary_pct=0.25),
    "gemma": dict(hidden=256, heads=2, kv_heads=1, head_dim=256, ffn=512, vocab=128, hidden_act="gelu", embed_scale=True, eps=1e-6),
}
RECIPES = [(8, 128), (4, 64), (4, 128)]
RECIPE_IDS = ["w8g128", "w4g64", "w4g128"]


def _model(dev, geom, layers, wbits, gs, seed=11, max_pos=1024):
    """test_gpu_decode_batch._model's recipe with per-group weight grids on every linear."""
    import mobilequant_amd as mq
    from mobilequant_amd.calibration import get_act_range
    from mobilequant_amd.llama import LlamaForCausalLM, LlamaShape
    shape = LlamaShape(layers=layers, max_pos=max_pos, **GEOMS[geom])
    m = LlamaForCausalLM(shape)
    m.reset_parameters(seed=seed, std=0.08)
    m = m.to(dev).eval().requires_grad_(False)
    g = torch.Generator().manual_seed(5)
    act = get_act_range(m, [torch.randint(0, shape.vocab, (1, 48), generator=g) for _ in range(2)])
    mq.create_sim_qmodel(m, mq.QuantConfig(bitwidth=wbits, is_per_channel=True, group_size=gs), mq.QuantConfig(bitwidth=8))
    for n, mod in m.named_modules():                          # ptq/mobilequant.py:175-201
        if isinstance(mod, mq.QLinear):
            if "w2" in n or "o_proj" in n:
                mod.output_quantizer.qcfg.bitwidth = 16
        elif isinstance(mod, (mq.QRMSNorm, mq.QLayerNorm)):
            mod.input_quantizer.qcfg.bitwidth = 16
            mod.weight_quantizer.qcfg.bitwidth = 16
            mod.weight_quantizer.qcfg.is_symmetric = False
            mod.weight_quantizer.qcfg.is_per_channel = False
        elif isinstance(mod, mq.QMatMul):
            if "qk_bmm" in n:
                mod.output_quantizer.qcfg.bitwidth = 16
            if "pv_bmm" in n:
                mod.input_quantizer.qcfg.bitwidth = 16
    mq.set_scale_and_offset(m, act, "buffer")
    return m


@pytest.mark.parametrize("recipe", RECIPES, ids=RECIPE_IDS)
@pytest.mark.parametrize("geom", ["llama", "stablelm", "gemma"])
def test_decode_engine_matches_module_graph(dev, geom, recipe):
    from mobilequant_amd.decode import DecodeEngine
    wbits, gs = recipe
    m = _model(dev, geom, 2, wbits, gs, max_pos=64)
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(0, m.shape.vocab, (1, 24), generator=g)
    with torch.no_grad():
        want = m(ids.to(dev))[0].cpu().numpy()
    for launches in (4, 5):                                   # an explicit four-launch request falls back to five
        eng = DecodeEngine(m, cache_len=64, launches=launches)
        assert eng.launches == 5
        assert [k for k, _ in eng.phases[:5]] == ["gemv_grouped", "attn", "gemv_grouped", "gemv_grouped", "gemv_grouped"]
        assert all(a.b.batch == 1 and a.b.g.w4 == int(wbits == 4) and a.group_size == gs for k, a in eng.phases if k == "gemv_grouped")
    got = np.stack([eng.step(int(t)).cpu().numpy().copy() for t in ids[0]])
    eng.reset()
    eng.capture()
    replay = np.stack([eng.step(int(t)).cpu().numpy().copy() for t in ids[0]])
    assert np.array_equal(got, replay)
    span = float(np.ptp(want))
    d = np.abs(got - want)
    assert d.max() <= 0.05 * span and np.median(d) <= 0.001 * span and (d <= 0.01 * span).mean() >= 0.97, (d.max() / span, np.median(d) / span)


def test_per_channel_models_lower_as_before(dev):
    from test_gpu_decode_batch import _model as pc_model
    from mobilequant_amd.decode import DecodeEngine
    from mobilequant_amd.decode_batch import BatchDecodeEngine
    m = pc_model(dev, "llama", 1, 4)
    assert DecodeEngine(m, cache_len=64).launches == 4
    assert [k for k, _ in DecodeEngine(m, cache_len=64, launches=5).phases] == ["gemv", "attn", "gemv", "gemv", "gemv"]
    assert [k for k, _ in BatchDecodeEngine(m, 2, cache_len=64).phases] == ["gemv", "attn", "gemv", "gemv", "gemv"]


CACHE = 848
PROMPT_LENS = [1, 7, 63, 64, 65, 300, 767, 700]
STEPS = 40


@pytest.mark.parametrize("geom,recipe", [("llama", (4, 128)), ("stablelm", (8, 128)), ("gemma", (4, 64))], ids=["llama-w4g128", "stablelm-w8g128", "gemma-w4g64"])
def test_every_slot_is_the_single_engine_bit_for_bit(dev, geom, recipe):
    from test_gpu_decode_batch import _prompts, _single_run, _start_slot
    from mobilequant_amd.decode import DecodeEngine
    from mobilequant_amd.decode_batch import BatchDecodeEngine
    m = _model(dev, geom, 2, *recipe)
    prompts = _prompts(m.shape.vocab, PROMPT_LENS)
    single = DecodeEngine(m, cache_len=CACHE)
    assert single.launches == 5
    refs = [_single_run(single, p, STEPS) for p in prompts]
    for B, pick in ((1, [6]), (3, [0, 3, 7]), (8, list(range(8)))):
        be = BatchDecodeEngine(m, B, cache_len=CACHE)
        assert [k for k, _ in be.phases[:5]] == ["gemv_grouped", "attn", "gemv_grouped", "gemv_grouped", "gemv_grouped"]
        for b, i in enumerate(pick):
            _start_slot(be, b, prompts[i])
        be.capture()
        for k in range(STEPS):
            out = be.step([refs[i][0][k] for i in pick])
            for b, i in enumerate(pick):
                assert torch.equal(out[b], refs[i][1][k]), (B, b, k, float((out[b] - refs[i][1][k]).abs().max()))
        for b, i in enumerate(pick):
            for li, (kc, vc) in enumerate(refs[i][2]):
                assert torch.equal(be.cached_keys(b, li), kc) and torch.equal(be.cached_values(b, li), vc), (B, b, li)


def test_swapping_a_slot_leaves_the_others_unchanged(dev):
    from mobilequant_amd.decode_batch import BatchDecodeEngine
    m = _model(dev, "llama", 2, 4, 128)
    V = m.shape.vocab
    g = torch.Generator().manual_seed(9)
    prompts = [torch.randint(0, V, (n,), generator=g).tolist() for n in (40, 100, 70)]
    newp = torch.randint(0, V, (55,), generator=g).tolist()
    toks = torch.randint(0, V, (20, 3), generator=g).tolist()
    runs = {}
    for swap in (False, True):
        be = BatchDecodeEngine(m, 3, cache_len=160)
        for b in range(3):
            be.prefill(b, prompts[b])
        be.capture()
        rows = []
        for k in range(20):
            if swap and k == 8:
                be.release(1)
                be.prefill(1, newp)
            rows.append(be.step(toks[k]).clone())
        runs[swap] = (torch.stack(rows), [c.clone() for c in be.k_cache], [c.clone() for c in be.v_cache])
    a, b_ = runs[False], runs[True]
    for s in (0, 2):
        assert torch.equal(a[0][:, s], b_[0][:, s])
        assert all(torch.equal(x[s], y[s]) for x, y in zip(a[1], b_[1])) and all(torch.equal(x[s], y[s]) for x, y in zip(a[2], b_[2]))


def test_refusals(dev):
    from mobilequant_amd.decode import DecodeEngine
    from mobilequant_amd.decode_batch import BatchDecodeEngine
    m = _model(dev, "llama", 1, 4, 128, max_pos=64)
    attn = m.layers[0].self_attn
    attn.k_proj.weight_quantizer.qcfg.group_size = 64                 # a phase with two group sizes
    for E in (lambda: DecodeEngine(m, cache_len=64), lambda: BatchDecodeEngine(m, 2, cache_len=64)):
        with pytest.raises(RuntimeError, match="mix group sizes"):
            E()
    attn.k_proj.weight_quantizer.qcfg.group_size = -1                 # per-channel k_proj beside grouped q / v
    with pytest.raises(RuntimeError, match="mix per-group and per-channel"):
        DecodeEngine(m, cache_len=64)
    m = _model(dev, "llama", 1, 8, 64, max_pos=64)
    mlp = m.layers[0].mlp
    for lin in (mlp.w1, mlp.w3):
        lin.weight_quantizer.qcfg.group_size = 192                    # a multiple of 64 that is not a power of two (nor divides K)
    with pytest.raises(RuntimeError, match="group_size 192"):
        DecodeEngine(m, cache_len=64)
