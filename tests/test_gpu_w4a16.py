"""GPU: W4A16 -- mq_w4a16_linear (csrc/mq_w4a16.hip: the M <= 8 weight-streaming GEMV and the MFMA GEMM), weight_only.py, WeightOnlyLinear
and create_weight_only_qmodel, against the numpy oracle of the contract (tests/w4a16_ref.py).

Exact cases: integer x, power-of-two scales, random nibbles and zeros -- every partial sum is an integer multiple of a power of two below
2^24, so the result equals the float64 oracle bit for bit whatever the summation order: they pin nibble order, group mapping, zero
handling, lane maps and tails.  Rounding cases pin the fp16 conversions (ties of both parities, subnormal products).  Gaussian cases are
held to the derived bound 2 K 2^-24 sum|x16 w16| + ulp_out(|y64|); the model to four times the reference arithmetic's own order
sensitivity (MODEL_ORDER_SENSITIVITY below)."""
import copy
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(1, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import w4a16_ref as R  # noqa: E402
from w4a16_cases import exact_x, one_hot_x  # noqa: E402,F401  (shared with the launch-branch pin, tests/test_gpu_w4a16_oracle.py)
from oracle import mq_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

F16, F32 = np.float16, np.float32

# The toy model's logits under the torch emulation of the contract (every converted linear as F.linear(fp16(x), w16)) move by at most this
# much when the emulation's linears accumulate in float32 instead of float64 -- measured on the CPU with emulated_toy() below (seed 0, ids
# of toy_ids(); `python tests/test_gpu_w4a16.py` prints it): the reference arithmetic's own sensitivity to the summation order, the code
# under test not involved.  The device model may differ from the float64-accumulating emulation by MODEL_ORDER_FACTOR times that.
MODEL_ORDER_SENSITIVITY = 1.069e-3     # at max |logit| = 3.23: a late fp32 bit upstream flips fp16 roundings of the next linear's input
MODEL_ORDER_FACTOR = 4.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def launch(dev, x, packed, s16, z16, bias, g, out_dtype):
    """mq_w4a16_linear through the C entry itself (x and out dtypes chosen apart); numpy in, numpy out."""
    from mobilequant_amd import _lib as L
    xt, wt, st, zt = _t(x, dev), _t(packed, dev), _t(s16, dev), _t(z16, dev)
    bt = _t(bias, dev) if bias is not None else None
    M, K = x.shape
    N = packed.shape[0]
    out = torch.full((M, N), float("nan"), dtype=torch.float32 if out_dtype == F32 else torch.float16, device=dev)
    a = L.MqW4A16Args()
    a.x, a.x_dtype = xt.data_ptr(), L.MQ_F32 if x.dtype == F32 else L.MQ_F16
    a.M, a.N, a.K, a.group_size = M, N, K, K if g == -1 else g
    a.w_packed, a.scales, a.zeros = wt.data_ptr(), st.data_ptr(), zt.data_ptr()
    a.bias = bt.data_ptr() if bt is not None else None
    a.out, a.out_dtype = out.data_ptr(), L.MQ_F32 if out_dtype == F32 else L.MQ_F16
    L.call("mq_w4a16_linear", ctypes.byref(a), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == F32 else np.uint16)


def assert_bits(got, want, what):
    if not np.array_equal(bits(got), bits(want)):
        bad = np.argwhere(bits(got) != bits(want))
        m, n = bad[0]
        raise AssertionError(f"{what}: {len(bad)} of {got.size} outputs differ, first at [m={m}, n={n}]: got {got[m, n]!r}, want {want[m, n]!r}; "
                             f"rows {sorted(set(bad[:, 0]))[:8]}, cols {sorted(set(bad[:, 1]))[:8]}")


# ---- exact cases -----------------------------------------------------------------------------------------------------------------------
def exact_weights(rng, N, K, g):
    """Random nibbles, zeros in [-3, 18], scales 2^e with e in [-6, -1] drawn per row and group: nothing symmetric or constant."""
    gs, G = R.groups(K, g)
    u = rng.integers(0, 16, size=(N, K), dtype=np.uint8)
    z16 = rng.integers(-3, 19, size=(N, G)).astype(F16)
    s16 = (2.0 ** rng.integers(-6, 0, size=(N, G))).astype(F16)
    return u, s16, z16


GEMV_SHAPES = [(16, 64, 32), (48, 128, 64), (272, 512, 128), (16, 256, 256)]
GEMM_SHAPES = [(16, 64, 32), (80, 192, 64), (272, 512, 32)]
EXACT = [(M, *s) for s in GEMV_SHAPES for M in (1, 3, 8)] + [(M, *s) for s in GEMM_SHAPES for M in (9, 16, 17, 100)]


@pytest.mark.parametrize("M,N,K,g", EXACT)
def test_exact_fp32_out(dev, M, N, K, g):
    """fp32 and fp16 x, with and without bias, random and one-hot x: bit-equal to the float64 oracle."""
    from mobilequant_amd import weight_only
    rng = np.random.default_rng(M * 1000003 + N * 1009 + K + g)
    assert weight_only.w4a16_variant(M, N, K, g) == (1 if M <= 8 else 2)
    u, s16, z16 = exact_weights(rng, N, K, g)
    packed, w16 = R.pack(u), R.w16(u, s16, z16, g)
    bias = (rng.integers(-40, 41, size=N) / 64.0).astype(F32)
    for xname, x in (("random", exact_x(rng, M, K)), ("one-hot", one_hot_x(rng, M, K))):
        for xdt in (F32, F16):
            for b in (None, bias):
                y64, _ = R.linear64(x.astype(xdt), w16, b)
                want = y64.astype(F32)
                assert np.array_equal(want.astype(np.float64), y64)                     # the case IS exact
                got = launch(dev, x.astype(xdt), packed, s16, z16, b, g, F32)
                assert_bits(got, want, f"M={M} N={N} K={K} g={g} x={xname}/{np.dtype(xdt).name} bias={b is not None}")


@pytest.mark.parametrize("M,N,K,g", [(1, 48, 128, 64), (8, 272, 512, 128), (9, 80, 192, 64), (100, 272, 512, 32)])
def test_exact_fp16_out(dev, M, N, K, g):
    """fp16 output: one scale exponent per row and sparse x keep |y| below 2048 x the row's power of two, so y is an fp16 number."""
    rng = np.random.default_rng(M + N + K + g)
    gs, G = R.groups(K, g)
    u = rng.integers(0, 16, size=(N, K), dtype=np.uint8)
    z16 = rng.integers(-3, 19, size=(N, G)).astype(F16)
    e = rng.integers(-6, 0, size=(N, 1))
    s16 = np.broadcast_to(2.0 ** e, (N, G)).astype(F16)
    x = np.zeros((M, K), F32)
    for m in range(M):
        x[m, rng.choice(K, size=8, replace=False)] = rng.choice([-4, -3, -2, -1, 1, 2, 3, 4], size=8)      # |sum| <= 8 * 4 * 21 = 672
    bias = (rng.integers(-40, 41, size=N) * 2.0 ** e[:, 0]).astype(F32)
    packed, w16 = R.pack(u), R.w16(u, s16, z16, g)
    for xdt in (F32, F16):
        for b in (None, bias):
            y64, _ = R.linear64(x.astype(xdt), w16, b)
            want = y64.astype(F16)
            assert np.array_equal(want.astype(np.float64), y64)
            got = launch(dev, x.astype(xdt), packed, s16, z16, b, g, F16)
            assert_bits(got, want, f"fp16 out M={M} N={N} K={K} g={g} x={np.dtype(xdt).name} bias={b is not None}")


def test_dispatch_boundary_m8_m9(dev):
    """The same weights at M = 8 (GEMV) and M = 9 (GEMM): every row equals the oracle, and the entry's rule (mq_w4a16_supported returns
    the kernel it takes) says both kernels ran."""
    from mobilequant_amd import weight_only
    rng = np.random.default_rng(89)
    N, K, g = 48, 128, 64
    assert weight_only.w4a16_variant(8, N, K, g) == 1 and weight_only.w4a16_variant(9, N, K, g) == 2
    u, s16, z16 = exact_weights(rng, N, K, g)
    packed, w16 = R.pack(u), R.w16(u, s16, z16, g)
    x = exact_x(rng, 9, K)
    want = R.linear64(x, w16)[0].astype(F32)
    got8, got9 = launch(dev, x[:8], packed, s16, z16, None, g, F32), launch(dev, x, packed, s16, z16, None, g, F32)
    assert_bits(got8, want[:8], "M=8")
    assert_bits(got9, want, "M=9")
    assert_bits(got9[:8], got8, "rows 0..7 of M=9 against M=8")


# ---- rounding cases --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [3, 17])
def test_x_ties_round_to_even(dev, M):
    """fp32 x exactly half way between two fp16 numbers, both parities of the lower neighbour: x16 = fp16_rne(x)."""
    rng = np.random.default_rng(M)
    N, K, g = 16, 64, 32
    h = (1.0 + rng.integers(0, 1024, size=(M, K)) / 1024.0).astype(F16)          # [1, 2): spacing 2^-10
    h[:, 0], h[:, 1] = F16(1.0), F16(1.0 + 2.0 ** -10)                           # an even and an odd significand for sure
    x = (h.astype(F32) + F32(2.0 ** -11)).astype(F32)
    x16 = R.x16(x)
    even = (bits(h) & 1) == 0
    assert np.array_equal(bits(x16)[even], bits(h)[even]) and np.array_equal(bits(x16)[~even], bits(h)[~even] + 1) and even.any() and (~even).any()
    u = rng.integers(0, 16, size=(N, K), dtype=np.uint8)
    z16 = rng.integers(-3, 19, size=(N, K // g)).astype(F16)
    s16 = (2.0 ** rng.integers(-3, 0, size=(N, K // g))).astype(F16)
    y64, _ = R.linear64(x, R.w16(u, s16, z16, g))
    want = y64.astype(F32)
    assert np.array_equal(want.astype(np.float64), y64)          # multiples of 2^-13 below 2^12: exact in any order
    assert_bits(launch(dev, x, R.pack(u), s16, z16, None, g, F32), want, f"x ties M={M}")


@pytest.mark.parametrize("M", [3, 17])
def test_scale_ties_and_subnormal_products(dev, M):
    """Scales whose fp16 rounding is a tie (through w4a16_pack: s16 = fp16_rne(s)), and scales so small that s16 * (u - z') is an fp16
    subnormal: dequantize() equals the oracle's w16 bit for bit, and a K = 64 product with integer x is exact."""
    from mobilequant_amd import weight_only
    rng = np.random.default_rng(40 + M)
    N, K, g = 16, 64, 32
    G = K // g
    h = (1.0 + rng.integers(0, 1024, size=(N, G)) / 1024.0).astype(F16)
    h[0, 0], h[0, 1] = F16(1.0), F16(1.0 + 2.0 ** -10)
    s_tie = ((h.astype(F32) + F32(2.0 ** -11)) * F32(2.0 ** -4)).astype(F32)               # ties in [2^-4, 2^-3)
    s_sub = (rng.integers(1, 64, size=(N, G)) * 2.0 ** -24).astype(F32)                    # fp16 subnormals: products k d 2^-24
    for what, s, sym in (("tie", s_tie, False), ("subnormal", s_sub, True)):
        qmin, _ = R.limits(sym)
        o = (rng.integers(-3, 19, size=(N, G)) + qmin).astype(F32)
        q_target = rng.integers(qmin, qmin + 16, size=(N, K)).astype(F32)
        w = ((q_target.reshape(N, G, g) - o[:, :, None]) * s[:, :, None]).astype(F32).reshape(N, K)
        u, s16, z16 = R.stored(w, s, o, sym, g)
        assert len(np.unique(u)) == 16
        w16 = R.w16(u, s16, z16, g)
        if what == "subnormal":
            sub = (np.abs(w16.astype(np.float64)) < 2.0 ** -14) & (w16 != 0)
            assert sub.sum() > N * K // 8                                                   # plenty of subnormal weights
        else:
            assert not np.array_equal(s16.astype(F32), s)                                   # the scales do round
        qw, ds, dz = weight_only.w4a16_pack(_t(w, dev), _t(s, dev), _t(o, dev), 4, sym, g)
        assert np.array_equal(qw.cpu().numpy(), R.pack(u)), what
        assert_bits(ds.cpu().numpy(), s16, what + " s16")
        assert_bits(dz.cpu().numpy(), z16, what + " zeros")
        assert_bits(weight_only.w4a16_dequantize(qw, ds, dz, g).cpu().numpy(), w16, what + " dequantize")
        x = rng.integers(-2, 3, size=(M, K)).astype(F32)
        x[:, 0] = 1.0
        y64, _ = R.linear64(x, w16)
        want = y64.astype(F32)
        assert np.array_equal(want.astype(np.float64), y64)
        got = weight_only.w4a16_linear(_t(x, dev), qw, ds, dz, None, g)
        torch.cuda.synchronize()
        assert_bits(got.cpu().numpy(), want, f"{what} M={M}")


# ---- tolerance cases -------------------------------------------------------------------------------------------------------------------
def check_bound(got, x, w16, bias, K, out_dtype, what):
    y64, sumabs = R.linear64(x, w16, bias)
    err = np.abs(got.astype(np.float64) - y64)
    bnd = R.bound(K, sumabs, y64, out_dtype)
    ratio = float((err / bnd).max())
    print(f"{what}: max |y - y64| / bound = {ratio:.4f}")
    assert np.all(err <= bnd), f"{what}: worst error / bound = {ratio:.3f}"
    return ratio


@pytest.mark.parametrize("xdt", [F32, F16])
@pytest.mark.parametrize("M,N,K,g", [(1, 256, 2048, 128), (8, 256, 2048, 64), (64, 256, 2048, 128), (130, 128, 1024, 32)])
def test_gaussian_within_the_derived_bound(dev, M, N, K, g, xdt):
    from mobilequant_amd import weight_only
    import mobilequant_amd.quantization.qmodule as Q
    sym = (M + g) % 3 == 0
    rng = np.random.default_rng(M + N + K + g)
    w = rng.standard_normal((N, K)).astype(F32)
    x = rng.standard_normal((M, K)).astype(xdt)
    bias = rng.standard_normal(N).astype(F32)
    wt = _t(w, dev)
    mn, mx = Q.compute_min_max_from_tensor(wt, True, g)
    s, o, *_ = Q.compute_scale_offset_from_min_max(mn, mx, 4, sym)
    qw, ds, dz = weight_only.w4a16_pack(wt, s, o, 4, sym, g)
    # the packed form is the oracle's, from the oracle's own grid
    so, oo = R.grid_from_minmax(w, sym, g)
    u, s16, z16 = R.stored(w, so, oo, sym, g)
    assert np.array_equal(qw.cpu().numpy(), R.pack(u))
    assert_bits(ds.cpu().numpy(), s16, "scales")
    assert_bits(dz.cpu().numpy(), z16, "zeros")
    w16 = R.w16(u, s16, z16, g)
    got = weight_only.w4a16_linear(_t(x, dev), qw, ds, dz, _t(bias, dev), g)
    torch.cuda.synchronize()
    assert got.dtype == (torch.float32 if xdt == F32 else torch.float16) and got.shape == (M, N)
    check_bound(got.cpu().numpy(), x, w16, bias, K, xdt, f"M={M} N={N} K={K} g={g} {np.dtype(xdt).name}")


# ---- module ----------------------------------------------------------------------------------------------------------------------------
def _qlinear(dev, N, K, g, sym, bias, seed):
    import mobilequant_amd.quantization.qmodule as Q
    torch.manual_seed(seed)
    lin = nn.Linear(K, N, bias=bias)
    with torch.no_grad():
        lin.weight.mul_(3.0)
        lin.weight[1, :g].abs_().add_(0.5)                    # an all-positive group: a negative zero on the asymmetric grid
    lin = lin.to(dev)
    return Q.QLinear.from_float(lin, Q.QuantConfig(bitwidth=16), Q.QuantConfig(bitwidth=4, group_size=g, is_symmetric=sym, is_per_channel=True),
                                Q.QuantConfig(bitwidth=32))


@pytest.mark.parametrize("kind", ["asymmetric", "symmetric", "lwc"])
def test_module_from_qlinear(dev, kind):
    import mobilequant_amd.quantization.qmodule as Q
    N, K, g = 48, 128, 64
    sym = kind == "symmetric"
    ql = _qlinear(dev, N, K, g, sym, True, 5)
    w = ql.weight.detach().cpu().numpy()
    G = K // g
    if kind == "lwc":
        wq = ql.weight_quantizer
        wq.enable_lwc(ql.weight)
        gen = torch.Generator().manual_seed(3)
        with torch.no_grad():
            wq.upbound_factor.copy_((torch.rand(wq.upbound_factor.shape, generator=gen) * 3.0 + 0.5).to(dev))
            wq.lowbound_factor.copy_((torch.rand(wq.lowbound_factor.shape, generator=gen) * 3.0 + 0.5).to(dev))
        sig_lo = torch.sigmoid(wq.lowbound_factor.detach()).cpu().numpy().reshape(-1)
        sig_hi = torch.sigmoid(wq.upbound_factor.detach()).cpu().numpy().reshape(-1)
        f = O.lwc_fused_forward(w.reshape(N * G, g), sig_lo, sig_hi, 4, sym)
        s, o = f["scale"].reshape(N, G), f["offset"].reshape(N, G)
        assert not np.array_equal(s, R.grid_from_minmax(w, sym, g)[0])          # the clipped grid is another grid
    else:
        s, o = R.grid_from_minmax(w, sym, g)
    wo = Q.to_weight_only_quantized_linear(ql, name="blk.w")
    assert type(wo) is Q.WeightOnlyLinear and (wo.in_features, wo.out_features, wo.bits, wo.group_size) == (K, N, 4, g)
    u, s16, z16 = R.stored(w, s, o, sym, g)
    if kind == "asymmetric":
        assert float(z16[1, 0]) < 0
    w16 = R.w16(u, s16, z16, g)
    assert np.array_equal(wo.qweight.cpu().numpy(), R.pack(u))
    assert_bits(wo.dequantize().cpu().numpy(), w16, kind + " dequantize")
    bias = ql.bias.detach().cpu().numpy()
    rng = np.random.default_rng(11)
    x = rng.standard_normal((2, 5, K)).astype(F32)
    y = wo(_t(x, dev))
    assert y.shape == (2, 5, N) and y.dtype == torch.float32
    check_bound(y.cpu().numpy().reshape(10, N), x.reshape(10, K), w16, bias, K, F32, kind + " 3-D fp32")
    # a non-contiguous input: every second row of a wider buffer, transposed leading dims
    big = rng.standard_normal((5, 4, 2 * K)).astype(F32)
    xt = _t(big, dev)[:, ::2, ::2].transpose(0, 1)
    assert not xt.is_contiguous() and xt.shape == (2, 5, K)
    y = wo(xt)
    check_bound(y.cpu().numpy().reshape(10, N), xt.cpu().numpy().reshape(10, K), w16, bias, K, F32, kind + " non-contiguous")
    # fp16 in, fp16 out
    xh = rng.standard_normal((12, K)).astype(F16)
    yh = wo(_t(xh, dev))
    assert yh.dtype == torch.float16
    check_bound(yh.cpu().numpy(), xh, w16, bias, K, F16, kind + " fp16")
    # state_dict into a fresh module: identical output bits
    fresh = Q.WeightOnlyLinear(K, N, g, bias=True, device=dev)
    fresh.load_state_dict(wo.state_dict())
    assert torch.equal(fresh(_t(x, dev)), wo(_t(x, dev))) and torch.equal(fresh(_t(xh, dev)), yh)
    fl = wo.to_float()
    assert type(fl) is nn.Linear and torch.equal(fl.weight, wo.dequantize().float()) and torch.equal(fl.bias, wo.bias)
    cov = Q.int8_coverage(nn.Sequential(wo, nn.SiLU()))
    assert cov["w4a16_modules"] == ["0"] and cov["modules"]["0"]["w4a16"] >= 4


def test_refusals_come_at_conversion_not_at_forward(dev):
    import mobilequant_amd.quantization.qmodule as Q
    cfg = Q.QuantConfig(bitwidth=4, group_size=-1, is_per_channel=True)
    for shape, needle in (((96, 48), "K % 64 == 0"), ((128, 24), "N % 16 == 0")):
        with pytest.raises(ValueError, match=needle) as e:
            Q.to_weight_only_quantized_linear(nn.Linear(*shape).to(dev), cfg, name="head.fc")
        assert "head.fc" in str(e.value)
    with pytest.raises(ValueError, match="3-bit"):
        Q.to_weight_only_quantized_linear(nn.Linear(128, 32).to(dev), Q.QuantConfig(bitwidth=3, group_size=-1, is_per_channel=True))
    # a grid whose zero point leaves +-1024 is refused with the module's name
    lin = nn.Linear(128, 16, bias=False).to(dev)
    with torch.no_grad():
        lin.weight.uniform_(5.0, 5.001)
    with pytest.raises(ValueError, match="zero point") as e:
        Q.to_weight_only_quantized_linear(lin, cfg, name="head.far")
    assert "head.far" in str(e.value)


# ---- model -----------------------------------------------------------------------------------------------------------------------------
TOY_CFG = dict(bitwidth=4, group_size=64, is_symmetric=False, is_per_channel=True)


def toy_model(seed=0):
    from mobilequant_amd.llama import LlamaForCausalLM, LlamaShape
    m = LlamaForCausalLM(LlamaShape.toy()).eval()
    m.reset_parameters(0.08, seed=seed)
    return m


def toy_ids():
    return torch.from_numpy(np.random.default_rng(1).integers(0, 97, size=(2, 24)))


class EmulatedLinear(nn.Module):
    """The contract in torch: F.linear(fp16(x), w16) accumulated in `acc` (float64 or float32), back to x's dtype."""

    def __init__(self, w16, acc):
        super().__init__()
        self.register_buffer("w16", w16)
        self.acc = acc

    def forward(self, x):
        return F.linear(x.half().float().to(self.acc), self.w16.to(self.acc)).to(x.dtype)


def emulated_toy(model, acc):
    """A copy of the float model with every linear the surgery converts replaced by EmulatedLinear on the ORACLE's w16."""
    m = copy.deepcopy(model)
    for name, mod in list(m.named_modules()):
        for cname, child in list(mod._modules.items()):
            if type(child) is nn.Linear and "lm_head" not in cname:
                w = child.weight.detach().cpu().numpy()
                s, o = R.grid_from_minmax(w, TOY_CFG["is_symmetric"], TOY_CFG["group_size"])
                u, s16, z16 = R.stored(w, s, o, TOY_CFG["is_symmetric"], TOY_CFG["group_size"])
                w16 = torch.from_numpy(R.w16(u, s16, z16, TOY_CFG["group_size"])).to(child.weight.device)
                mod._modules[cname] = EmulatedLinear(w16, acc)
    return m


def measure_order_sensitivity():
    """CPU: max |logits(float64-accumulating emulation) - logits(float32-accumulating emulation)| of the toy model."""
    base = toy_model()
    with torch.no_grad():
        a = emulated_toy(base, torch.float64)(toy_ids())
        b = emulated_toy(base, torch.float32)(toy_ids())
    return float((a.double() - b.double()).abs().max()), float(a.abs().max())


def test_model_logits_and_perplexity(dev):
    import mobilequant_amd.quantization.qmodule as Q
    from mobilequant_amd import scoring
    base = toy_model().to(dev)
    ids = toy_ids().to(dev)
    with torch.no_grad():
        want = emulated_toy(base, torch.float64)(ids)
    m = Q.create_weight_only_qmodel(copy.deepcopy(base), Q.QuantConfig(**TOY_CFG))
    kinds = {n: type(mod).__name__ for n, mod in m.named_modules()}
    assert kinds["layers.1.mlp.w2"] == "WeightOnlyLinear" and kinds["layers.0.self_attn.k_proj"] == "WeightOnlyLinear" and kinds["lm_head"] == "Linear"
    assert sum(k == "WeightOnlyLinear" for k in kinds.values()) == 14
    with torch.no_grad():
        got = m(ids)
    torch.cuda.synchronize()
    assert got.shape == want.shape == (2, 24, 97) and torch.isfinite(got).all()
    err = float((got.double() - want.double()).abs().max())
    print(f"toy logits: max |device - emulation| = {err:.3e}, allowed {MODEL_ORDER_FACTOR * MODEL_ORDER_SENSITIVITY:.3e}, max |logit| = {float(want.abs().max()):.3f}")
    assert MODEL_ORDER_SENSITIVITY > 0 and err <= MODEL_ORDER_FACTOR * MODEL_ORDER_SENSITIVITY
    # the quantized model is a different model from the float one, and scoring runs on it
    with torch.no_grad():
        assert float((base(ids) - got).abs().max()) > 100 * MODEL_ORDER_SENSITIVITY
    streams = [np.random.default_rng(2).integers(0, 97, size=40).tolist(), np.random.default_rng(3).integers(0, 97, size=33).tolist()]
    p = scoring.perplexity(m, streams, max_length=64)
    assert p.tokens == 71 and np.isfinite(p.ppl) and np.isfinite(p.sum_logprob) and p.ppl > 1.0
    lp, lse, _ = scoring.token_logprobs(m, ids)
    assert torch.isfinite(lp).all() and torch.isfinite(lse[:, :-1]).all()
    cov = Q.int8_coverage(m)
    assert len(cov["w4a16_modules"]) == 14 and cov["simulated_calls"] == 0


if __name__ == "__main__":
    print("MODEL_ORDER_SENSITIVITY = %.3e (max |logit| %.3f)" % measure_order_sensitivity())
