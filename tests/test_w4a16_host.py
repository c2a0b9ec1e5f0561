"""Host side of W4A16 (no GPU): the numpy oracle of the contract against oracle.mq_oracle, the packed layout, the C entry's argument
checks (they come back before any HIP call), the surgery of create_weight_only_qmodel on meta tensors, and the barrier audit of the
compiled kernels."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import w4a16_ref as R  # noqa: E402
from oracle import mq_oracle as O  # noqa: E402
from toy_models import Block  # noqa: E402

import mobilequant_amd.quantization.qmodule as Q  # noqa: E402
from mobilequant_amd.quantization.fp_ops import FMatMul, HFRMSNorm  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the oracle helper ---------------------------------------------------------------------------------------------------------------
def _weights(rng, N, K, positive_group=None, g=None):
    w = rng.standard_normal((N, K)).astype(np.float32)
    if positive_group is not None:
        n, gi = positive_group
        w[n, gi * g:(gi + 1) * g] = np.abs(w[n, gi * g:(gi + 1) * g]) + np.float32(0.75)      # min > 0: offset < 0 on an asymmetric grid
    return w


@pytest.mark.parametrize("sym", [False, True])
@pytest.mark.parametrize("g", [32, 64, -1])
def test_helper_index_and_dequant_equal_the_oracles_fake_quant(sym, g):
    rng = np.random.default_rng(100 + 2 * (g % 97) + sym)
    N, K = 6, 128
    gs, G = R.groups(K, g)
    w = _weights(rng, N, K, positive_group=(2, G - 1), g=gs)
    s, o = R.grid_from_minmax(w, sym, g)
    qmin, qmax = R.limits(sym)
    u, s16, zp = R.stored(w, s, o, sym, g)
    if not sym:
        assert float(zp[2, G - 1]) < 0                       # the all-positive group: a zero auto_gptq could not store
    zp32 = (o - np.float32(qmin)).astype(np.float32)
    want = O.fake_quant(w.reshape(N * G, gs), s.reshape(-1, 1), o.reshape(-1, 1), qmin, qmax).reshape(N, K)
    got = R.dequant_f32(u, s, zp32, g)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    q = R.index(w, s, o, sym, g)
    assert np.array_equal(q, O.quantize_index(w.reshape(N * G, gs), s.reshape(-1, 1), o.reshape(-1, 1), qmin, qmax).reshape(N, K))
    assert np.array_equal(u.astype(np.int32) + qmin, q.astype(np.int32))
    # stored forms: fp16 to nearest even, the zero exactly
    assert np.array_equal(s16, s.astype(np.float16)) and np.array_equal(zp.astype(np.float32), zp32)


def test_helper_pack_roundtrip_and_documented_layout():
    rng = np.random.default_rng(7)
    u = rng.integers(0, 16, size=(5, 128), dtype=np.uint8)
    p = R.pack(u)
    assert p.shape == (5, 64) and np.array_equal(R.unpack(p), u)
    # byte j of 16-byte group kb: element 32 kb + j low, 32 kb + 16 + j high
    assert p[3, 16 * 2 + 5] == (u[3, 64 + 5] | (u[3, 64 + 21] << 4))
    # the same image as the W4A8 kernels' (oracle.pack_w4 takes indices and qmin)
    assert np.array_equal(p, O.pack_w4(u.astype(np.int32) - 8, -8)) and np.array_equal(R.unpack(p).astype(np.int32) - 8, O.unpack_w4(p, -8))


def test_helper_w16_is_one_rounding():
    # s16 = 1 + 2^-10, u - z' = 3: the product 3 + 3 * 2^-10 is no fp16 number (spacing 2^-9 there) and is rounded once, from float64
    s16 = np.array([[1 + 2.0 ** -10]], np.float16)
    u = np.full((1, 32), 5, np.uint8)
    w = R.w16(u, s16, np.array([[2.0]], np.float16), 32)
    exact = float(s16[0, 0]) * 3.0
    assert float(w[0, 0]) == float(np.float64(exact).astype(np.float16))
    # a negative zero point and the bound's floor
    assert float(R.w16(u, np.array([[0.5]], np.float16), np.array([[-3.0]], np.float16), 32)[0, 0]) == 4.0
    assert R.ulp_out(np.array([0.0]), np.float16)[0] == 2.0 ** -24


# ---- the C boundary ------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_built():
    from mobilequant_amd import _lib, build
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mobilequant_amd.h")).read(), flags=re.S)
    for name in ("mq_w4a16_linear", "mq_w4a16_supported"):
        assert name in _lib.EXPORTED_SYMBOLS
        assert re.search(r"\b%s\s*\(" % name, hdr)
    assert "mq_w4a16.hip" in build.SOURCES
    assert "mq_w4a16_args" in hdr and ctypes.sizeof(_lib.MqW4A16Args) == 96
    ver = int(re.search(r"#define MQ_VERSION (\d+)", hdr).group(1))
    assert ver // 100 == _lib.HEADER_MAJOR              # the major the ctypes structs mirror: additive entries keep it


def _args(L, **kw):
    a = L.MqW4A16Args()
    p = 0x10000
    a.x, a.x_dtype, a.M, a.N, a.K, a.group_size = p, L.MQ_F32, 4, 32, 128, 64
    a.w_packed, a.scales, a.zeros, a.bias, a.out, a.out_dtype = p, p, p, None, p, L.MQ_F32
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_entry_refuses_bad_arguments_before_any_hip_call():
    from mobilequant_amd import _lib as L
    lib = L.load()

    def run(**kw):
        a = _args(L, **kw)
        rc = lib.mq_w4a16_linear(ctypes.byref(a), None)
        return rc, lib.mq_last_error().decode(), lib.mq_w4a16_supported(a.M, a.N, a.K, a.group_size)

    assert lib.mq_w4a16_linear(None, None) == 1 and "null pointer" in lib.mq_last_error().decode()
    for field in ("x", "w_packed", "scales", "zeros", "out"):
        rc, msg, _ = run(**{field: None})
        assert rc == 1 and "null pointer" in msg, field
    for field in ("x", "w_packed", "out", "bias"):
        rc, msg, _ = run(**{field: 0x10004})
        assert rc == 1 and "misaligned" in msg, field
    assert run(scales=0x10001)[0] == 1 and run(zeros=0x10001)[0] == 1
    for field in ("x_dtype", "out_dtype"):
        for bad in (L.MQ_I8, L.MQ_U8, L.MQ_I32, 17, -1):
            rc, msg, _ = run(**{field: bad})
            assert rc == 1 and "MQ_F32 or MQ_F16" in msg, (field, bad)
    # shapes: MQ_EUNSUPPORTED with the rule, and the predicate agrees
    for kw, rule in ((dict(K=96, group_size=32), "K % 64 == 0"), (dict(N=24), "N % 16 == 0"), (dict(group_size=48), "multiple of 32"),
                     (dict(K=192, group_size=128), "must divide K"), (dict(N=0), "N % 16 == 0"), (dict(K=0), "K % 64 == 0"),
                     (dict(group_size=0), "multiple of 32"), (dict(group_size=-1), "multiple of 32")):
        rc, msg, sup = run(**kw)
        assert rc == 3 and rule in msg and "mq_w4a16_supported" in msg and sup == 0, (kw, msg)
    assert run(M=-1)[0] == 1
    # M == 0: a no-op, whatever else is in the block
    assert run(M=0, x=None, out=None)[0] == 0
    # served shapes: which kernel the entry takes (1: GEMV, 2: GEMM)
    assert lib.mq_w4a16_supported(1, 16, 64, 32) == 1 and lib.mq_w4a16_supported(8, 5632, 2048, 128) == 1
    assert lib.mq_w4a16_supported(9, 16, 64, 32) == 2 and lib.mq_w4a16_supported(2048, 2048, 5632, 128) == 2
    assert lib.mq_w4a16_supported(8, 2048, 5632, 128) == 1 and lib.mq_w4a16_supported(8, 16, 8192, 8192) == 1
    assert lib.mq_w4a16_supported(8, 16, 8256, 32) == 2        # M * K beyond the GEMV's staging buffer: the GEMM serves it
    assert lib.mq_w4a16_supported(4, 48, 192, 96) == 1         # a group size that is no power of two


# ---- surgery (structure on meta tensors: packing needs the device) -------------------------------------------------------------------
class ToyLM128(nn.Module):
    """tests/toy_models.ToyLM at widths mq_w4a16_linear serves (K % 64 == 0, N % 16 == 0)."""

    def __init__(self, d=128, f=192, device=None):
        super().__init__()
        with torch.device(device) if device is not None else torch.device("cpu"):
            self.layers = nn.ModuleList([Block(d, f), Block(d, f)])
            self.norm = HFRMSNorm(d)
            self.lm_head = nn.Linear(d, 48, bias=False)

    def forward(self, x):
        for layer in self.layers:
            x = layer(x)
        return self.lm_head(self.norm(x))


W4G64 = dict(bitwidth=4, group_size=64, is_per_channel=True)


def _sim_meta(wcfg, acfg=None):
    m = ToyLM128(device="meta").eval()
    Q.create_sim_qmodel(m, Q.QuantConfig(**wcfg), acfg if acfg is not None else Q.QuantConfig(bitwidth=16))
    return m


def _check_structure(m, g):
    for blk in m.layers:
        for name in ("q_proj", "k_proj", "v_proj", "o_proj", "w1", "w2", "w3"):
            lin = getattr(blk, name)
            assert type(lin) is Q.WeightOnlyLinear, name
            N, K = (192, 128) if name in ("w1", "w3") else (128, 192) if name == "w2" else (128, 128)
            assert (lin.out_features, lin.in_features, lin.bits, lin.group_size) == (N, K, 4, g)
            sd = lin.state_dict()
            assert list(sd) == ["qweight", "scales", "zeros"]
            assert sd["qweight"].shape == (N, K // 2) and sd["qweight"].dtype == torch.uint8
            for k in ("scales", "zeros"):
                assert sd[k].shape == (N, K // g) and sd[k].dtype == torch.float16
            assert "bits=4" in repr(lin) and f"group_size={g}" in repr(lin)
        assert type(blk.input_layernorm).__name__ == "HFRMSNorm" and type(blk.post_attention_layernorm).__name__ == "HFRMSNorm"
        assert type(blk.qk_bmm) is FMatMul and type(blk.pv_bmm) is FMatMul and type(blk.act_fn) is nn.SiLU
    assert type(m.lm_head) is nn.Linear and type(m.norm).__name__ == "HFRMSNorm"
    assert not any(isinstance(mod, Q._Q_TYPES) for mod in m.modules())


def test_surgery_from_a_sim_model_follows_the_reference_rules():
    m = _sim_meta(W4G64)
    assert type(m.layers[0].q_proj) is Q.QLinear and type(m.layers[0].act_fn) is Q.QSiLU
    out = Q.create_weight_only_qmodel(m)
    assert out is m
    _check_structure(m, 64)
    cov = Q.int8_coverage(m)
    assert cov["w4a16_modules"] == [f"layers.{i}.{n}" for i in (0, 1) for n in ("q_proj", "k_proj", "v_proj", "o_proj", "w1", "w3", "w2")]
    assert cov["modules"]["layers.0.w2"] == {"w4a16": 0} and cov["int8_calls"] == 0 and "14 weight-only" in cov["summary"]


def test_surgery_from_a_float_model_uses_w_qcfg_and_leaves_lm_head():
    m = ToyLM128(device="meta").eval()
    Q.create_weight_only_qmodel(m, Q.QuantConfig(bitwidth=4, group_size=-1, is_per_channel=True))
    assert m.layers[0].w2.group_size == 192 and m.layers[0].q_proj.group_size == 128 and type(m.lm_head) is nn.Linear
    m = ToyLM128(device="meta").eval()
    Q.create_weight_only_qmodel(m, Q.QuantConfig(**W4G64))
    _check_structure(m, 64)
    # a bias becomes an fp32 buffer
    lin = nn.Linear(128, 32, bias=True, device="meta")
    wo = Q.to_weight_only_quantized_linear(lin, Q.QuantConfig(**W4G64))
    assert list(wo.state_dict()) == ["qweight", "scales", "zeros", "bias"] and wo.bias.dtype == torch.float32 and wo.bias.shape == (32,)
    with pytest.raises(ValueError, match="w_qcfg"):
        Q.create_weight_only_qmodel(ToyLM128(device="meta").eval())


def test_the_recursion_condition_is_the_references():
    # a container with ONE child is not descended into (qmodule.py:884: len(children) > 1)
    m = nn.Sequential(nn.Sequential(nn.Linear(128, 64, device="meta")))
    Q.create_weight_only_qmodel(m, Q.QuantConfig(**W4G64))
    assert type(m[0][0]) is nn.Linear
    m = nn.Sequential(nn.Sequential(nn.Linear(128, 64, device="meta"), nn.SiLU()), nn.SiLU())
    Q.create_weight_only_qmodel(m, Q.QuantConfig(**W4G64))
    assert type(m[0][0]) is Q.WeightOnlyLinear


@pytest.mark.parametrize("wcfg,acfg,needle", [
    (dict(bitwidth=3, group_size=64, is_per_channel=True), None, "3-bit weight grid"),
    (dict(bitwidth=2, group_size=64, is_per_channel=True), None, "2-bit weight grid"),
    (dict(bitwidth=8, group_size=64, is_per_channel=True), None, "8-bit weight grid"),
    (dict(bitwidth=4, group_size=-1, is_per_channel=False), None, "per-tensor weight grid"),
    (W4G64, Q.QuantConfig(bitwidth=8), "8-bit input quantizer"),
    (dict(bitwidth=4, group_size=80, is_per_channel=True), None, "does not divide K"),
    (dict(bitwidth=4, group_size=16, is_per_channel=True), None, "mq_w4a16_supported"),
])
def test_conversion_refuses_with_the_modules_name_and_the_rule(wcfg, acfg, needle):
    m = _sim_meta(wcfg, acfg)
    with pytest.raises(ValueError) as e:
        Q.create_weight_only_qmodel(m)
    msg = str(e.value)
    assert needle in msg and re.search(r"layers\.1\.(w2|o_proj)", msg), msg          # (reversed traversal: the last block's linear comes first)


def test_conversion_refuses_an_8_bit_output_quantizer_and_an_unserved_shape():
    lin = Q.QLinear.from_float(nn.Linear(128, 64, device="meta"), Q.QuantConfig(bitwidth=16), Q.QuantConfig(**W4G64), Q.QuantConfig(bitwidth=8))
    with pytest.raises(ValueError, match="8-bit output quantizer"):
        Q.to_weight_only_quantized_linear(lin, name="blk.w9")
    for shape, needle in (((96, 64), "does not divide K"), ((128, 24), "mq_w4a16_supported")):
        with pytest.raises(ValueError, match=needle) as e:
            Q.to_weight_only_quantized_linear(nn.Linear(*shape, device="meta"), Q.QuantConfig(**W4G64), name="blk.w9")
        assert "blk.w9" in str(e.value)
    with pytest.raises(ValueError, match="N % 16 == 0"):
        Q.to_weight_only_quantized_linear(nn.Linear(128, 24, device="meta"), Q.QuantConfig(bitwidth=4, group_size=-1, is_per_channel=True))


def test_state_dict_roundtrips_into_a_fresh_module_on_the_host():
    a = Q.WeightOnlyLinear(128, 32, 64, bias=True)
    a.qweight.copy_(torch.randint(0, 256, a.qweight.shape, dtype=torch.uint8))
    a.scales.copy_(torch.rand(a.scales.shape).half())
    a.zeros.copy_(torch.randint(-3, 19, a.zeros.shape).half())
    a.bias.copy_(torch.randn(32))
    b = Q.WeightOnlyLinear(128, 32, 64, bias=True)
    assert b.load_state_dict(a.state_dict()).missing_keys == []
    for k, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k]) and v.dtype == b.state_dict()[k].dtype
    # dequantize / to_float are host-side torch: equal to the oracle bit for bit
    w = a.dequantize()
    want = R.w16(R.unpack(a.qweight.numpy()), a.scales.numpy(), a.zeros.numpy(), 64)
    assert w.dtype == torch.float16 and np.array_equal(w.numpy().view(np.uint16), want.view(np.uint16))
    f = a.to_float()
    assert type(f) is nn.Linear and torch.equal(f.weight, w.float()) and torch.equal(f.bias, a.bias)
    with pytest.raises(RuntimeError, match="no CPU path"):
        a(torch.zeros(1, 128))


def test_exports():
    import mobilequant_amd
    from mobilequant_amd import quantization
    for mod in (mobilequant_amd, quantization):
        for name in ("WeightOnlyLinear", "to_weight_only_quantized_linear", "create_weight_only_qmodel"):
            assert getattr(mod, name) is getattr(Q, name)
    from mobilequant_amd import ops, weight_only
    assert not hasattr(ops, "w4a16_linear") and callable(weight_only.w4a16_linear) and callable(weight_only.w4a16_pack)


# ---- the compiled kernels ----------------------------------------------------------------------------------------------------------------
def test_no_barrier_with_lds_traffic_in_flight(tmp_path):
    """tests/test_cabi.py's audit, for csrc/mq_w4a16.hip (its barriers are the compiler's)."""
    from mobilequant_amd import build
    flags = [f for f in build.FLAGS if f != "-fPIC"]
    src = "mq_w4a16.hip"
    asm = str(tmp_path / "mq_w4a16.s")
    cmd = [build.HIPCC, *flags, *build.PER_FILE_FLAGS.get(src, ()), "-w", "--cuda-device-only", "-S", os.path.join(ROOT, "mobilequant_amd", "csrc", src), "-o", asm]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-2000:]
    rep = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "barrier_audit.py"), asm], stdout=subprocess.PIPE, text=True).stdout
    assert "PENDING" not in rep and "possibly in flight 0" in rep, rep
    text = open(asm).read()
    assert "v_mfma_f32_16x16x32_f16" in text                                     # the GEMM is on the fp16 MFMA
    assert not re.search(r"\.private_segment_fixed_size:\s*[1-9]", text) and not re.search(r"\.vgpr_spill_count:\s*[1-9]", text)
