"""Host side of the decode-cache <-> image-cache bridge: the two entry points exist on both sides of the C ABI and
refuse bad arguments before any device is touched.  No GPU needed."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mq_attention_cache_import", "mq_attention_cache_export")


@pytest.fixture(scope="module")
def lib():
    from mobilequant_amd import _lib, build
    build.build()
    return _lib.load()


def test_symbols_are_exported_and_declared(lib):
    from mobilequant_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mobilequant_amd.h")).read(), flags=re.S)
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS
        assert re.search(r"\bint " + name + r"\(const mq_attention_cache_args\* args, mq_stream_t stream\);", hdr), name


def test_entry_points_validate_before_any_hip_call(lib):
    """Fake, aligned pointers that are never dereferenced: every refusal is MQ_EINVAL with a message."""
    from mobilequant_amd import _lib as L
    p = 0x10000

    def args(**kw):
        a = L.MqAttentionCacheArgs()
        base = dict(k=p, v=p, k_head_stride=256 * 64, v_head_stride=256 * 64, v_chunked=0, kv_heads=2, head_dim=64, cache_len=256, p0=0, n=128,
                    cache_seq=256, k_i8=p, vt_i8=p, k_rowsum=p)
        base.update(kw)
        for name, val in base.items():
            setattr(a, name, val)
        a.qk_a = L.MqGrid(p, p, 0.0, 255.0)
        a.qk_b = L.MqGrid(p, p, 0.0, 255.0)
        return a

    def refused(fn, text, **kw):
        assert getattr(lib, fn)(ctypes.byref(args(**kw)), None) == 1, (fn, kw)
        assert text in lib.mq_last_error().decode(), (lib.mq_last_error(), text)

    for fn in NAMES:
        assert getattr(lib, fn)(None, None) == 1 and b"null argument block" in lib.mq_last_error()
        refused(fn, "head_dim 64, 128 or 256", head_dim=96)
        refused(fn, "cache_seq", cache_seq=200)
        refused(fn, "exceeds", n=320, cache_seq=320, cache_len=256)
        refused(fn, "exceeds", n=192, cache_seq=128)
        refused(fn, "null pointer", vt_i8=None)
        refused(fn, "head strides", k_head_stride=100)
        refused(fn, "16-byte aligned", k=p + 4)
        refused(fn, "multiple of 16 with v_chunked", v_chunked=1, cache_len=250, k_head_stride=250 * 64, v_head_stride=250 * 64)
    refused(NAMES[0], "n % 64 == 0", n=100)
    refused(NAMES[0], "n % 64 == 0", p0=64, n=64)
    refused(NAMES[0], "v_prefix", head_dim=128, k_head_stride=256 * 128, v_head_stride=256 * 128)
    refused(NAMES[0], "v_prefix", v_prefix=p)
    refused(NAMES[0], "k_f16", head_dim=128, k_head_stride=256 * 128, v_head_stride=256 * 128, v_prefix=p, k_f16=p)
    refused(NAMES[1], "n > 0", n=0)
    refused(NAMES[1], "p0 >= 0", p0=-1)


def test_ops_refuse_on_the_host():
    from mobilequant_amd import ops
    c = ops.attention_image_cache(2, 64, 256, "cpu")
    k, v = torch.zeros(2, 256, 64, dtype=torch.int8), torch.zeros(2, 256, 64, dtype=torch.int8)
    one = torch.ones(1)
    grids = {"qk_a": (one, one * 128, 0.0, 255.0), "qk_b": (one, one * 128, 0.0, 255.0)}
    with pytest.raises(RuntimeError, match="n % 64 == 0"):
        ops.attention_cache_import(c, k, v, 100, grids)
    bad = ops.attention_image_cache(2, 96, 256, "cpu")
    with pytest.raises(RuntimeError, match="head_dim 64, 128 and 256"):
        ops.attention_cache_import(bad, k, v, 128, grids)
    with pytest.raises(RuntimeError, match="head_dim 64, 128 and 256"):
        ops.attention_cache_export(bad, k, v, 64, 37)
    for wrong_v, chunked in ((torch.zeros(2, 256, 32, dtype=torch.int8), False), (v, True), (torch.zeros(2, 16, 64, 16, dtype=torch.int8), False),
                             (v.float(), False), (v[:, ::2], False)):
        with pytest.raises(RuntimeError, match="shape mismatch|int8 decode caches"):
            ops.attention_cache_import(c, k, wrong_v, 128, grids, v_chunked=chunked)
        with pytest.raises(RuntimeError, match="shape mismatch|int8 decode caches"):
            ops.attention_cache_export(c, k, wrong_v, 64, 37, v_chunked=chunked)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        ops.attention_cache_export(c, k[:, :64], v[:, :64], 64, 37)              # the decode caches end before the rows
    with pytest.raises(RuntimeError, match="outside the image cache"):
        ops.attention_cache_export(c, k, v, 250, 37)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.attention_cache_import(c, k, v, 128, grids)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.attention_cache_export(c, k, torch.zeros(2, 16, 64, 16, dtype=torch.int8), 64, 37, v_chunked=True)


def test_engines_take_the_append_argument():
    import inspect
    from mobilequant_amd.decode import DecodeEngine
    from mobilequant_amd.decode_batch import BatchDecodeEngine
    assert inspect.signature(DecodeEngine.prefill).parameters["append"].default is False
    assert inspect.signature(BatchDecodeEngine.prefill).parameters["append"].default is False
    assert DecodeEngine.APPEND_MIN_TOKENS % 8 == 0 and BatchDecodeEngine.APPEND_MIN_TOKENS == DecodeEngine.APPEND_MIN_TOKENS
