"""CPU: the decode-step attention oracle (oracle.decode_attention_step) is row `pos` of attention_sim(..., exact_int=True), and the
decode engine's cache-length limits (which chain serves a cache_len, where it refuses) sit where the kernels' LDS puts them."""
import ctypes

import numpy as np
import pytest

from oracle import mq_oracle as O

F32 = np.float32


def _grid(bits, lo, hi):
    g = O.QuantizerOracle(bitwidth=bits)
    g.set_from_minmax(F32(lo), F32(hi))
    return g


def _rope(S, rot):
    inv = 1.0 / (10000.0 ** (np.arange(0, rot, 2, dtype=F32) / rot))
    ang = np.outer(np.arange(S, dtype=F32), inv).astype(F32)
    ang = np.concatenate((ang, ang), -1)
    return np.cos(ang).astype(F32), np.sin(ang).astype(F32)


@pytest.mark.parametrize("D,H,KV,rot,pv_bits", [(32, 8, 2, 32, 16), (64, 4, 4, 16, 12), (128, 4, 1, 128, 8), (256, 2, 1, 256, 16)])
def test_decode_attention_step_is_row_pos_of_attention_sim(D, H, KV, rot, pv_bits):
    rng = np.random.default_rng(D + pv_bits)
    S = 200
    q, k, v = (rng.standard_normal((S, n * D), dtype=np.float32) * F32(1.5) for n in (H, KV, KV))
    k[77] = np.tile(q[77, :D], KV)                     # (one position whose score stands out)
    cos, sin = _rope(S, rot)
    qk = (_grid(8, -4.0, 4.0), _grid(8, -4.5, 4.5), _grid(16, -40.0, 40.0))
    pv = (_grid(pv_bits, 0.0, 1.0), _grid(8, -4.0, 4.0), _grid(8, -1.5, 1.5))
    # the cache of int8 indices - 128 the engine holds: RoPE'd keys on qk.input2, values on pv.input2
    kr = O.rope_partial(k.reshape(S, KV, D).transpose(1, 0, 2), cos, sin)
    k_cache = (O._index(kr, qk[1]).astype(np.int64) - 128).astype(np.int8)
    v_cache = (O._index(v.reshape(S, KV, D).transpose(1, 0, 2), pv[1]).astype(np.int64) - 128).astype(np.int8)
    n_diff = 0
    for pos in (0, 1, 63, 64, 77, 130, S - 1):
        want = O.attention_sim(q[:pos + 1], k[:pos + 1], v[:pos + 1], cos[:pos + 1], sin[:pos + 1], H, KV, qk, pv, exact_int=True)[pos]
        got = O.decode_attention_step(q[pos], k[pos], v[pos], k_cache, v_cache, pos, cos[pos], sin[pos], H, KV, qk, pv)
        assert np.array_equal(got["y"].view(np.uint32), want.view(np.uint32)), (pos, np.abs(got["y"] - want).max())
        assert np.array_equal(got["k_new"], k_cache[:, pos]) and np.array_equal(got["v_new"], v_cache[:, pos]), pos
        assert np.array_equal(got["out_q"], (O._index(want, pv[2]).astype(np.int64) - 128).astype(np.int8)), pos
        # the float64 softmax rounds to the fp32 one's index everywhere but at a few boundary cases, and only by one step
        d = np.abs(got["p_idx"] - got["p_idx64"])
        assert d.max() <= 1, pos
        n_diff += int((d > 0).sum())
    assert n_diff <= 8, n_diff


def test_oproj_int_sums_is_the_integer_matmul():
    rng = np.random.default_rng(3)
    w = rng.integers(-128, 128, (48, 64)).astype(np.int8)
    zp = rng.integers(-20, 20, 48).astype(np.int32)
    a8 = rng.integers(-128, 128, 64).astype(np.int8)
    want = [sum(int(w[n, j]) * int(a8[j]) for j in range(64)) - int(zp[n]) * int(a8.astype(np.int64).sum()) for n in range(48)]
    assert O.oproj_int_sums(w, zp, a8).tolist() == want


# -- cache-length limits -----------------------------------------------------------------------------------------------------------
LIMITS_4 = {256: {32: 23072, 64: 23056, 128: 23024, 256: 22944}, 1024: {32: 22176, 64: 22160, 128: 22128, 256: 22048}}


def _shape(D):
    from mobilequant_amd.llama import LlamaShape
    return LlamaShape(hidden=256, layers=1, heads=4, kv_heads=2, head_dim=D, ffn=512, vocab=64, max_pos=64)


@pytest.mark.parametrize("D", [32, 64, 128, 256])
def test_cache_length_limits_follow_the_static_lds(D):
    """7 bytes of LDS per cached position (four launches) or 4 (five) on top of the kernel's static LDS, 160 KiB per workgroup."""
    from mobilequant_amd.decode import DecodeEngine as E
    for t in (256, 1024):
        n = E.max_cache_len(4, D, t)
        assert n == LIMITS_4[t][D] and n % 16 == 0
        assert 7 * n + E.AO_STATIC_LDS[t][D] <= 160 * 1024 < 7 * (n + 16) + E.AO_STATIC_LDS[t][D]
    assert E.max_cache_len(4, D) == LIMITS_4[1024][D]            # an engine replays both variants
    assert E.max_cache_len(5, D) == 32768 and 4 * 32768 + 9008 <= 160 * 1024


@pytest.mark.parametrize("D", [32, 64, 128, 256])
def test_engine_chooses_the_chain_on_both_sides_of_each_limit(D):
    from mobilequant_amd.decode import DecodeEngine as E
    s = _shape(D)
    lim4 = E.max_cache_len(4, D)
    geom = E._oproj_geometry(s, D)
    assert geom is not None
    assert E._chain_geometry(s, D, lim4, 4) == geom                  # four launches up to their limit
    assert E._chain_geometry(s, D, lim4 + 16, 4) is None             # five beyond it
    assert E._chain_geometry(s, D, lim4, 5) is None                  # (five when asked for)
    assert E._chain_geometry(s, D, 32768, 4) is None
    assert E._chain_geometry(s, D, 1000, 4) is None                  # (not a multiple of 16: the transposed value cache)
    for launches in (4, 5):
        for bad in (32768 + 16, 32769, 0):
            with pytest.raises(RuntimeError, match="cache_len"):
                E._chain_geometry(s, D, bad, launches)


def test_the_c_entries_refuse_a_cache_beyond_their_lds():
    """Host-side checks only: argument blocks that fail them return before anything reaches a device."""
    from mobilequant_amd import _lib
    from mobilequant_amd._lib import MqDecodeAttentionArgs, MqDecodeAttentionOprojArgs, MqGrid
    from mobilequant_amd.decode import DecodeEngine as E
    fake = 1 << 20                                                   # non-null, aligned: never dereferenced on the host
    g8, g16 = MqGrid(fake, fake, 0.0, 255.0), MqGrid(fake, fake, 0.0, 65535.0)
    for D in (32, 64, 128, 256):
        for threads in (256, 1024):
            a = MqDecodeAttentionOprojArgs()
            a.qkv = a.k_cache = a.v_cache = a.rope_row = a.pos = a.consts = a.o_w = a.o_wzp = a.o_acc = fake
            a.heads, a.kv_heads, a.head_dim, a.rot_dim = 4, 2, D, D
            a.qk_a = a.qk_b = a.pv_b = a.o_in = g8
            a.qk_out = a.pv_out = g16
            a.pv_a = g16
            a.N, a.slices, a.tpr, a.threads, a.lg_slices = 256, (2 if D == 256 else 1), (2 if D == 256 else 1), threads, -1
            a.cache_len = E.max_cache_len(4, D, threads) + 16
            with pytest.raises(_lib.MobileQuantLibraryError, match=f"cache_len={a.cache_len} exceeds {a.cache_len - 16}"):
                _lib.call("mq_decode_attention_oproj", ctypes.byref(a), None)
        b = MqDecodeAttentionArgs()
        b.qkv = b.k_cache = b.v_cache = b.cos = b.sin = b.pos = b.consts = b.out_q = fake
        b.heads, b.kv_heads, b.head_dim, b.rot_dim, b.nsplit = 4, 2, D, D, 1
        b.qk_a = b.qk_b = b.pv_b = b.o_in = g8
        b.pv_a = g16
        b.cache_len = E.max_cache_len(5, D) + 16
        with pytest.raises(_lib.MobileQuantLibraryError, match="cache_len=32784"):
            _lib.call("mq_decode_attention", ctypes.byref(b), None)
