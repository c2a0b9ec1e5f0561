"""Batched decode entries without a GPU: argument blocks are rejected with MQ_EINVAL and a message before any HIP call, and the
barriers of mq_decode_batch.hip have no LDS traffic in flight.  Pointers are fake, aligned and never dereferenced."""
import ctypes
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x10000          # a fake, 16-byte aligned device address


@pytest.fixture(scope="module")
def lib():
    from mobilequant_amd import _lib, build
    build.build()
    return _lib.load()


def _grid(on=True, qmax=255.0):
    from mobilequant_amd._lib import MqGrid
    return MqGrid(P, P, 0.0, qmax) if on else MqGrid(None, None, 0.0, 0.0)


def _gemv(batch=2, K=2048, N=256, **kw):
    from mobilequant_amd._lib import MqDecodeGemvArgs, MqDecodeGemvBatchArgs
    g = MqDecodeGemvArgs()
    g.x, g.K, g.N, g.norm_w, g.a_grid, g.norm_in = P, K, N, P, _grid(), _grid(qmax=65535.0)
    g.w, g.alpha, g.w_zp, g.col_term, g.y, g.consts = P, P, P, P, P, P
    g.seg_end[0] = g.seg_end[1] = N
    for k, v in kw.items():
        setattr(g, k, v)
    a = MqDecodeGemvBatchArgs()
    a.g, a.batch, a.x_stride, a.y_stride, a.gate_stride = g, batch, K, N, 0
    return a


def _attn(batch=2, **kw):
    from mobilequant_amd._lib import MqDecodeAttentionArgs, MqDecodeAttentionBatchArgs
    a = MqDecodeAttentionArgs()
    a.qkv, a.k_cache, a.v_cache, a.cos, a.sin, a.pos, a.consts, a.out_q = P, P, P, P, P, P, P, P
    a.heads, a.kv_heads, a.head_dim, a.cache_len, a.rot_dim, a.nsplit = 8, 2, 64, 256, 64, 1
    a.qk_a, a.qk_b, a.pv_b, a.o_in = _grid(), _grid(), _grid(), _grid()
    a.pv_a, a.qk_out, a.pv_out = _grid(qmax=65535.0), _grid(qmax=65535.0), _grid()
    for k, v in kw.items():
        setattr(a, k, v)
    b = MqDecodeAttentionBatchArgs()
    b.a, b.batch, b.split_from, b.qkv_stride = a, batch, 768, (8 + 4) * 64
    return b


def _head(batch=2, K=2048, V=1000, **kw):
    from mobilequant_amd._lib import MqDecodeHeadBatchArgs
    h = MqDecodeHeadBatchArgs()
    h.x, h.x_stride, h.norm_weight, h.w, h.K, h.V, h.batch, h.logits, h.logits_stride = P, K, P, P, K, V, batch, P, V
    h.eps = 1e-5
    for k, v in kw.items():
        setattr(h, k, v)
    return h


def _rejects(lib, name, args, text):
    rc = getattr(lib, name)(ctypes.byref(args), None)
    msg = lib.mq_last_error()
    assert rc == 1, (name, rc, msg)
    assert text.encode() in msg, (name, msg)


def test_gemv_batch_rejects_bad_argument_blocks(lib):
    assert lib.mq_decode_gemv_batch(None, None) == 1 and b"null argument block" in lib.mq_last_error()
    _rejects(lib, "mq_decode_gemv_batch", _gemv(w=None), "null pointer")
    _rejects(lib, "mq_decode_gemv_batch", _gemv(consts=None), "consts")
    for b in (0, 9, -1):
        _rejects(lib, "mq_decode_gemv_batch", _gemv(batch=b), "outside 1..8")
    # B * K over the 128 KiB of images: Gemma's w2 (K = 16 384) fits at B = 8, K = 32 768 only at B <= 4
    a = _gemv(batch=8, K=16384 * 2, x=None, xq=P, norm_w=None)
    _rejects(lib, "mq_decode_gemv_batch", a, "exceeds the 131072 bytes")
    _rejects(lib, "mq_decode_gemv_batch", _gemv(batch=5, K=32768, x=None, xq=P, norm_w=None), "exceeds the 131072 bytes")
    _rejects(lib, "mq_decode_gemv_batch", _gemv(K=1000), "multiple of 256")
    _rejects(lib, "mq_decode_gemv_batch", _gemv(K=16384), "8192")                      # fp32 rows beyond the prologue's reach
    _rejects(lib, "mq_decode_gemv_batch", _gemv(x=P + 4), "16-byte aligned")
    a = _gemv()
    a.x_stride = 100
    _rejects(lib, "mq_decode_gemv_batch", a, "x_stride")
    _rejects(lib, "mq_decode_gemv_batch", _gemv(zero_acc=P, zero_n=4), "zero_acc / o_acc")
    _rejects(lib, "mq_decode_gemv_batch", _gemv(o_acc=P), "zero_acc / o_acc")
    a = _gemv()
    a.y_stride = 10
    _rejects(lib, "mq_decode_gemv_batch", a, "y_stride")


def test_attention_batch_rejects_bad_argument_blocks(lib):
    assert lib.mq_decode_attention_batch(None, None) == 1 and b"null argument block" in lib.mq_last_error()
    _rejects(lib, "mq_decode_attention_batch", _attn(pos=None), "null pointer")
    _rejects(lib, "mq_decode_attention_batch", _attn(k_cache=None), "null pointer")
    for b in (0, 9):
        _rejects(lib, "mq_decode_attention_batch", _attn(batch=b), "outside 1..8")
    _rejects(lib, "mq_decode_attention_batch", _attn(head_dim=48), "head_dim=48")
    _rejects(lib, "mq_decode_attention_batch", _attn(cache_len=40000), "cache_len=40000")
    _rejects(lib, "mq_decode_attention_batch", _attn(nsplit=4), "needs part and ticket")
    _rejects(lib, "mq_decode_attention_batch", _attn(k_cache=P + 8), "16-byte aligned")
    _rejects(lib, "mq_decode_attention_batch", _attn(prefetch_wgs=4), "prefetch")
    b = _attn()
    b.qkv_stride = 64
    _rejects(lib, "mq_decode_attention_batch", b, "qkv_stride")


def test_head_batch_rejects_bad_argument_blocks(lib):
    assert lib.mq_decode_head_batch(None, None) == 1 and b"null argument block" in lib.mq_last_error()
    _rejects(lib, "mq_decode_head_batch", _head(x=None), "null pointer")
    _rejects(lib, "mq_decode_head_batch", _head(logits=None), "null pointer")
    for b in (0, 9):
        _rejects(lib, "mq_decode_head_batch", _head(batch=b), "outside 1..8")
    _rejects(lib, "mq_decode_head_batch", _head(batch=8, K=8192, x_stride=8192), "exceeds the 32768")
    _rejects(lib, "mq_decode_head_batch", _head(K=1001), "K % 4 == 0")
    _rejects(lib, "mq_decode_head_batch", _head(w=P + 4), "16-byte aligned")
    _rejects(lib, "mq_decode_head_batch", _head(logits_stride=10), "logits_stride")
    _rejects(lib, "mq_decode_head_batch", _head(pos=P, cache_len=0), "cache_len")


def test_engine_refuses_batches_outside_the_limits_without_a_gpu():
    """The Python engine checks B before it allocates anything."""
    from mobilequant_amd.decode_batch import BatchDecodeEngine
    from mobilequant_amd.llama import LlamaForCausalLM, LlamaShape
    m = LlamaForCausalLM(LlamaShape(hidden=64, layers=1, heads=2, kv_heads=1, head_dim=32, ffn=128, vocab=16, max_pos=32))
    for b in (0, 9):
        with pytest.raises(ValueError, match="outside 1..8"):
            BatchDecodeEngine(m, b, cache_len=16)


def test_no_barrier_with_lds_traffic_in_flight_in_the_batched_kernels(tmp_path):
    """tools/barrier_audit.py (tests/test_cabi.py) on mq_decode_batch.hip: no s_barrier with an LDS operation possibly in flight."""
    from mobilequant_amd import build
    flags = [f for f in build.FLAGS if f != "-fPIC"]
    src = "mq_decode_batch.hip"
    asm = str(tmp_path / "mq_decode_batch.s")
    cmd = [build.HIPCC, *flags, *build.PER_FILE_FLAGS.get(src, ()), "-w", "--cuda-device-only", "-S", os.path.join(ROOT, "mobilequant_amd", "csrc", src), "-o", asm]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    rep = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "barrier_audit.py"), asm], stdout=subprocess.PIPE, text=True).stdout
    assert "PENDING" not in rep and "possibly in flight 0" in rep, rep
