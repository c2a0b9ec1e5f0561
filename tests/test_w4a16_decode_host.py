"""CPU: the W4A16 decode entries and engine without a device -- both entries refuse bad argument blocks before any
launch, the ctypes structs have the header's layout, the engine's constructor refuses what the kernels do not serve with the module and
the reason, and the concatenated / interleaved images hold the modules' own weights."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

P = 0x10000          # a fake, 16-byte aligned device address: never dereferenced
EINVAL, EUNSUPPORTED = 1, 3          # mq_status


@pytest.fixture(scope="module")
def lib():
    from mobilequant_amd import _lib, build
    build.build()
    return _lib.load()


def gemv_args(**kw):
    from mobilequant_amd import _lib as L
    a = L.MqW4A16DecodeGemvArgs()
    a.x, a.w_packed, a.scales, a.zeros, a.out = P, 2 * P, 3 * P, 4 * P, 5 * P
    a.N, a.K, a.group_size = 256, 128, 64
    a.prologue, a.epilogue, a.eps, a.act = L.MQ_W4A16_PRO_PLAIN, L.MQ_W4A16_EPI_BIAS, 1e-5, 0
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def attn_args(**kw):
    from mobilequant_amd import _lib as L
    a = L.MqW4A16DecodeAttentionArgs()
    a.qkv, a.k_cache, a.v_cache, a.rope_row, a.pos, a.out, a.part, a.ticket = P, 2 * P, 3 * P, 4 * P, 5 * P, 6 * P, 7 * P, 8 * P
    a.heads, a.kv_heads, a.head_dim, a.cache_len, a.rot_dim, a.nsplit = 8, 2, 64, 96, 64, 1
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def status(lib, fn, a):
    rc = getattr(lib, fn)(ctypes.byref(a), None)
    return rc, lib.mq_last_error().decode()


def test_entries_are_declared_exported_and_the_structs_match_the_header(lib):
    from mobilequant_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "mobilequant_amd.h")).read()
    for fn in ("mq_w4a16_decode_gemv", "mq_w4a16_decode_attention", "mq_w4a16_decode_supported"):
        assert fn in _lib.EXPORTED_SYMBOLS and hasattr(lib, fn)
    assert "mq_w4a16_decode.hip" in build.SOURCES
    assert int(re.search(r"#define MQ_VERSION (\d+)", hdr).group(1)) // 100 == _lib.HEADER_MAJOR == lib.mq_version() // 100     # the major stays
    for name in ("MQ_W4A16_PRO_PLAIN", "MQ_W4A16_PRO_RMSNORM", "MQ_W4A16_PRO_LAYERNORM", "MQ_W4A16_EPI_BIAS", "MQ_W4A16_EPI_RESID", "MQ_W4A16_EPI_GATED"):
        assert int(re.search(r"#define %s (\d+)" % name, hdr).group(1)) == getattr(_lib, name)
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "mobilequant_amd.h"', "int main(void) {"]
    want = []
    for S, c in ((_lib.MqW4A16DecodeGemvArgs, "mq_w4a16_decode_gemv_args"), (_lib.MqW4A16DecodeAttentionArgs, "mq_w4a16_decode_attention_args")):
        af = [f for f, _ in S._fields_]
        lines.append('  printf("%zu' + " %zu" * len(af) + '\\n", sizeof(' + c + "), " + ", ".join(f"offsetof({c}, {f})" for f in af) + ");")
        want += [ctypes.sizeof(S)] + [getattr(S, f).offset for f in af]
    lines += ["  return 0;", "}"]
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        open(c, "w").write("\n".join(lines))
        cc = next((x for x in ("cc", "gcc", "clang") if subprocess.run(["which", x], stdout=subprocess.PIPE).returncode == 0), "/opt/rocm/llvm/bin/clang")
        subprocess.run([cc, "-I" + os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        out = subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert [int(v) for v in out.split()] == want


def test_gemv_refuses_bad_argument_blocks_before_any_launch(lib):
    from mobilequant_amd import _lib as L
    fn = "mq_w4a16_decode_gemv"
    assert lib.mq_w4a16_decode_gemv(None, None) == EINVAL and b"null pointer" in lib.mq_last_error()
    for f in ("x", "w_packed", "scales", "zeros", "out"):
        rc, msg = status(lib, fn, gemv_args(**{f: None}))
        assert rc == EINVAL and msg.startswith(fn + ": null pointer"), (f, rc, msg)
    for f in ("x", "w_packed", "out", "bias", "resid", "norm_weight", "norm_bias"):
        rc, msg = status(lib, fn, gemv_args(**{f: P + 4}, epilogue=L.MQ_W4A16_EPI_RESID if f == "resid" else L.MQ_W4A16_EPI_BIAS))
        assert rc == EINVAL and "misaligned pointer" in msg, (f, rc, msg)
    for f in ("scales", "zeros"):                                                    # whole dwords of the fp16 grids are loaded
        for off in (1, 2):
            rc, msg = status(lib, fn, gemv_args(**{f: P + off}))
            assert rc == EINVAL and "misaligned pointer" in msg, (f, off, rc, msg)
    for kw, text in ((dict(prologue=3), "unknown prologue 3"), (dict(epilogue=-1), "epilogue -1"), (dict(prologue=1, eps=0.0), "eps > 0"),
                     (dict(epilogue=1), "needs resid"), (dict(epilogue=2, act=2), "act 2"), (dict(epilogue=2, bias=6 * P), "no bias"),
                     (dict(out=P), "out must not be x"), (dict(epilogue=1, resid=5 * P), "out must not be x or resid")):
        rc, msg = status(lib, fn, gemv_args(**kw))
        assert rc == EINVAL and text in msg, (kw, rc, msg)
    for kw, text in ((dict(N=24), "N % 16 == 0"), (dict(K=96), "K % 64 == 0"), (dict(group_size=48), "multiple of 32"), (dict(K=32832, group_size=64), "K <= 32768"),
                     (dict(N=48, epilogue=2), "gated: N % 32 == 0")):
        rc, msg = status(lib, fn, gemv_args(**kw))
        assert rc == EUNSUPPORTED and text in msg and "mq_w4a16_decode_supported" in msg, (kw, rc, msg)
    assert lib.mq_w4a16_decode_supported(2 * 16384, 2048, 128, 2) == 1 and lib.mq_w4a16_decode_supported(2048, 16384, 128, 1) == 1    # Gemma's FFN
    assert lib.mq_w4a16_decode_supported(48, 128, 64, 2) == 0 and lib.mq_w4a16_decode_supported(48, 128, 64, 0) == 1


def test_attention_refuses_bad_argument_blocks_before_any_launch(lib):
    from mobilequant_amd import _lib as L
    fn = "mq_w4a16_decode_attention"
    assert lib.mq_w4a16_decode_attention(None, None) == EINVAL and b"null pointer" in lib.mq_last_error()
    for f in ("qkv", "k_cache", "v_cache", "rope_row", "pos", "out"):
        rc, msg = status(lib, fn, attn_args(**{f: None}))
        assert rc == EINVAL and msg.startswith(fn + ": null pointer"), (f, rc, msg)
    for f, off in (("qkv", 4), ("k_cache", 8), ("v_cache", 4), ("out", 4), ("part", 8), ("rope_row", 2), ("pos", 1), ("ticket", 2)):
        rc, msg = status(lib, fn, attn_args(**{f: P + off}))
        assert rc == EINVAL and "misaligned pointer" in msg, (f, rc, msg)
    for kw, text in ((dict(cache_len=0), "cache_len=0 outside"), (dict(cache_len=(1 << 24) + 1), "outside 1 .. 2^24"), (dict(heads=0), "must be >= 1"),
                     (dict(nsplit=2, part=None), "needs part and ticket"), (dict(nsplit=2, ticket=None), "needs part and ticket")):
        rc, msg = status(lib, fn, attn_args(**kw))
        assert rc == EINVAL and text in msg, (kw, rc, msg)
    for kw, text in ((dict(head_dim=96), "head_dim 32, 64, 128 or 256"), (dict(heads=8, kv_heads=3), "heads % kv_heads == 0"), (dict(rot_dim=66), "rot_dim even"),
                     (dict(rot_dim=15), "rot_dim even"), (dict(nsplit=17), "1 <= nsplit <= 16"), (dict(cache_len=8193), "ceil(cache_len / nsplit) <= 8192")):
        rc, msg = status(lib, fn, attn_args(**kw))
        assert rc == EUNSUPPORTED and text in msg, (kw, rc, msg)


# ---- the engine's constructor on CPU models ----------------------------------------------------------------------------------------------
def packed_model(shape, g=64, seed=0, skip=()):
    """A LlamaForCausalLM on the CPU whose layer linears are WeightOnlyLinears packed by the ORACLE (tests/w4a16_ref.py: the device packer
    is not needed), except the names in `skip`."""
    import w4a16_ref as R
    import mobilequant_amd.quantization.qmodule as Q
    from mobilequant_amd.llama import LlamaForCausalLM
    m = LlamaForCausalLM(shape).eval()
    m.reset_parameters(0.08, seed=seed)
    for layer in m.layers:
        for parent in (layer.self_attn, layer.mlp):
            for name, lin in list(parent._modules.items()):
                if type(lin) is nn.Linear and name not in skip:
                    w = lin.weight.detach().numpy()
                    s, o = R.grid_from_minmax(w, False, g)
                    u, s16, z16 = R.stored(w, s, o, False, g)
                    wl = Q.WeightOnlyLinear(lin.in_features, lin.out_features, g, lin.bias is not None)
                    wl.qweight.copy_(torch.from_numpy(R.pack(u)))
                    wl.scales.copy_(torch.from_numpy(s16))
                    wl.zeros.copy_(torch.from_numpy(z16))
                    if lin.bias is not None:
                        wl.bias.copy_(lin.bias.detach())
                    parent._modules[name] = wl
    return m


def test_engine_refuses_what_it_does_not_serve_and_names_it(lib):
    from mobilequant_amd import WeightOnlyDecodeEngine
    from mobilequant_amd.llama import LlamaForCausalLM, LlamaShape
    import mobilequant_amd.quantization.qmodule as Q
    toy = LlamaShape.toy()
    with pytest.raises(ValueError, match=r"layers\.0\.self_attn\.q_proj: Linear is not a WeightOnlyLinear"):
        WeightOnlyDecodeEngine(LlamaForCausalLM(toy))                                     # a float model
    with pytest.raises(ValueError, match=r"layers\.0\.mlp\.w2: Linear is not a WeightOnlyLinear"):
        WeightOnlyDecodeEngine(packed_model(toy, skip=("w2",)))
    sim = Q.create_sim_qmodel(LlamaForCausalLM(toy), Q.QuantConfig(bitwidth=4, is_per_channel=True), Q.QuantConfig(bitwidth=8))
    with pytest.raises(ValueError, match=r"layers\.0\.self_attn\.q_proj: QLinear is not a WeightOnlyLinear"):
        WeightOnlyDecodeEngine(sim)                                                       # a sim (QLinear) model
    with pytest.raises(ValueError, match=r"cache_len: 129 outside 1 \.\. max_pos = 128"):
        WeightOnlyDecodeEngine(packed_model(toy), cache_len=129)
    with pytest.raises(ValueError, match="expected a LlamaForCausalLM"):
        WeightOnlyDecodeEngine(nn.Linear(4, 4))
    # shapes outside the kernels' rules: a head_dim the attention launch has no form for; an FFN whose interleaved image has N % 32 != 0
    with pytest.raises(ValueError, match="head_dim 16 is not served"):
        WeightOnlyDecodeEngine(packed_model(LlamaShape.toy(hidden=64, heads=4, kv_heads=2, head_dim=16, ffn=128), g=32))
    with pytest.raises(ValueError, match=r"attn_splits: 17"):
        WeightOnlyDecodeEngine(packed_model(toy), attn_splits=17)
    m = packed_model(toy)
    m.layers[1].mlp.act_fn = nn.GELU(approximate="tanh")
    with pytest.raises(ValueError, match=r"layers\.1\.mlp\.act_fn"):
        WeightOnlyDecodeEngine(m)
    # everything served: the refusal left is the missing device, not a ValueError
    for shape in (toy, LlamaShape.toy(norm="layernorm", qkv_bias=True, rotary_pct=0.25), LlamaShape.toy(hidden_act="gelu", embed_scale=True)):
        with pytest.raises(RuntimeError, match="ROCm device"):
            WeightOnlyDecodeEngine(packed_model(shape))


def test_images_round_trip_to_the_modules_weights():
    from mobilequant_amd import weight_only
    from mobilequant_amd.decode_weight_only import concat_rows, interleave_rows
    from mobilequant_amd.llama import LlamaShape
    m = packed_model(LlamaShape.toy(qkv_bias=True), g=32, seed=3)
    att, mlp = m.layers[1].self_attn, m.layers[1].mlp
    qw, qs, qz, qb = concat_rows((att.q_proj, att.k_proj, att.v_proj))
    w = weight_only.w4a16_dequantize(qw, qs, qz, 32)
    want = torch.cat([att.q_proj.dequantize(), att.k_proj.dequantize(), att.v_proj.dequantize()])
    assert w.shape == want.shape == (128 + 64 + 64, 128) and torch.equal(w.view(torch.int16), want.view(torch.int16))
    assert torch.equal(qb, torch.cat([att.q_proj.bias, att.k_proj.bias, att.v_proj.bias])) and len(set(qb.tolist())) > 200
    gw, gs, gz = interleave_rows(mlp.w1, mlp.w3)
    w = weight_only.w4a16_dequantize(gw, gs, gz, 32)
    a, b = mlp.w1.dequantize(), mlp.w3.dequantize()
    assert w.shape == (512, 128) and not torch.equal(a, b)
    assert torch.equal(w[0::2].contiguous().view(torch.int16), a.view(torch.int16)) and torch.equal(w[1::2].contiguous().view(torch.int16), b.view(torch.int16))
    for t in (qw, qs, qz, qb, gw, gs, gz):
        assert t.is_contiguous()
    # a bias on one of the three only: the others contribute zeros
    att.k_proj.bias = None
    qb2 = concat_rows((att.q_proj, att.k_proj, att.v_proj))[3]
    assert torch.equal(qb2[:128], qb[:128]) and not qb2[128:192].any() and torch.equal(qb2[192:], qb[192:])


def test_oracle_chain_agrees_with_the_module_chain_on_the_cpu():
    """tests/w4a16_decode_ref.py against llama.py itself: the float64 chain on the modules' dequantised weights equals the float model built
    from those weights (to_float) run in float64, step by step with a cache -- the oracle restates the graph correctly."""
    import w4a16_decode_ref as D
    from mobilequant_amd.llama import LlamaShape
    for shape in (LlamaShape.toy(), LlamaShape.toy(norm="layernorm", qkv_bias=True, rotary_pct=0.25), LlamaShape.toy(hidden_act="gelu", embed_scale=True)):
        m = packed_model(shape, seed=5)
        chain = D.Chain.from_packed(m)
        for layer in m.layers:
            for parent in (layer.self_attn, layer.mlp):
                for name, mod in list(parent._modules.items()):
                    if type(mod).__name__ == "WeightOnlyLinear":
                        parent._modules[name] = HalfInput(mod.to_float())
        m = m.double()
        ids = np.random.default_rng(2).integers(0, shape.vocab, size=6)
        got, _ = chain.run(ids, D.F64, T=8)
        cache = m.new_cache(1, 8, dtype=torch.float64)
        with torch.no_grad():
            want = np.stack([m(torch.tensor([[int(t)]]), cache=cache, pos=p)[0, 0].numpy() for p, t in enumerate(ids)])
        # HFRMSNorm computes in fp32 whatever its input's dtype, and a late fp32 bit of a norm's output flips fp16 roundings of the next
        # linear's input (3e-4 seen): the LayerNorm family pins the graph to float64's accuracy, the other two to 1e-3 (a wrong activation,
        # scale or residual moves the logits by 0.1 and more)
        tol = 1e-9 if shape.norm == "layernorm" else 1e-3
        assert np.abs(got - want).max() < tol * max(1.0, np.abs(want).max()), (shape, np.abs(got - want).max())


class HalfInput(nn.Module):
    """x -> linear(fp16(x)): the contract's x16 in front of a float linear."""

    def __init__(self, lin):
        super().__init__()
        self.lin = lin

    def forward(self, x):
        return self.lin(x.to(torch.float16).to(x.dtype))
