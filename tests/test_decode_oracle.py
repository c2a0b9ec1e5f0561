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


# -- mq_decode_gemv / mq_decode_head oracle ---------------------------------------------------------------------------------------
def _epilogue_vectors(qw, zw, shift, a_grid, w_grid_scale):
    """w_zp / col_term / alpha that turn the kernel's tt = sum_k wb a8 - zp rs + ct into sum_k (qa - za)(qw - zw): wb = qw - shift the
    stored weight byte, a8 = qa - 128 the image byte."""
    K = qw.shape[1]
    c, d = 128 - int(a_grid.offset), shift - zw.astype(np.int64)
    wb_sum = (qw.astype(np.int64) - shift).sum(1)
    return (F32(a_grid.scale) * w_grid_scale).astype(F32), (-d).astype(np.int32), (c * wb_sum + K * c * d).astype(np.int32)


@pytest.mark.parametrize("layernorm,w4,act", [(0, False, 0), (1, True, 1), (1, False, 0), (0, True, 1)])
def test_decode_gemv_oracle_is_the_module_chain(layernorm, w4, act):
    """In division form the launch oracle is Qnorm -> qlinear_int_exact -> Qout (segments) and, gated, Qout -> QSiLU / QGELU -> product
    -> w2's input quantizer, element for element; its image is Qnorm's index wherever the float64 norm is not near a tie."""
    rng = np.random.default_rng(10 * layernorm + 2 * w4 + act)
    K, N = 512, 96
    x = (rng.standard_normal(K) * 2).astype(F32)
    nin, ag = _grid(16, -8.0, 8.0), _grid(8, -3.0, 3.5)
    nw = O.fake_quant(rng.uniform(0.5, 1.5, K).astype(F32), *O.scale_offset_from_min_max(0.0, 1.5, 16, False))
    nb = (rng.standard_normal(K) * 0.1).astype(F32) if layernorm else None
    norm = O.qlayernorm if layernorm else O.qrmsnorm
    h = norm(x, nw, nb, 1e-5, nin, None, None)
    qa = O.quantize_index(h, ag.scale, ag.offset, 0, 255)
    bits = 4 if w4 else 8
    qw = rng.integers(0, 2 ** bits, (N, K))
    zw = rng.integers(0, 2 ** bits, N)
    sw = rng.uniform(0.001, 0.01, N).astype(F32)
    shift = 0 if w4 else 128
    w = O.pack_w4(qw, 0) if w4 else (qw - 128).astype(np.int8)
    alpha, zp, ct = _epilogue_vectors(qw, zw, shift, ag, sw)
    bias = (rng.standard_normal(N) * 0.2).astype(F32)
    outs = [_grid(8, -2.0, 2.0), _grid(16, -3.0, 3.0), _grid(8, -1.0, 1.5)]
    pro = dict(x=x, norm_w=nw, norm_bias=nb, layernorm=layernorm, norm_in=nin, eps=1e-5, a_grid=ag)
    acc, lin = O.qlinear_int_exact(qa, ag.offset, ag.scale, qw, zw, sw, bias)
    # plain launch, three segments with ragged ends
    got = O.decode_gemv_launch(K, N, w, alpha, zp, ct, w4=w4, bias=bias, seg_end=(37, 61), out_grid=outs, **pro)
    ok = ~got["tie_image"]
    assert np.array_equal(got["image"][ok].astype(np.int64) + 128, qa[ok].astype(np.int64)), "image"
    assert not got["tie_image"].any()               # (seeds chosen so: the exact comparisons below need the same image)
    assert np.array_equal(got["tt"].astype(np.int64), acc.astype(np.int64))
    for k, (lo, hi) in enumerate(((0, 37), (37, 61), (61, N))):
        want = O.fake_quant(lin[lo:hi], outs[k].scale, outs[k].offset, outs[k].qmin, outs[k].qmax)
        assert np.array_equal(got["y_div"][lo:hi].view(np.uint32), want.view(np.uint32)), k
    # the reciprocal form the kernels evaluate: the same to one step
    d = np.abs(got["y"] - got["y_div"])
    assert np.all(d <= np.array([outs[0 if n < 37 else 1 if n < 61 else 2].scale for n in range(N)], np.float64) * 1.0001)
    # gated launch: rows 2i / 2i+1 = w1 / w3 row i
    g_mid, g_act, g_out = _grid(16, 0.0, 1.0), _grid(16, -1.0, 4.0), _grid(8, -2.0, 2.0)
    gate = O.decode_gemv_launch(K, N, w, alpha, zp, ct, w4=w4, gate=True, bias=bias, out_grid=outs, gate_act=act,
                                gate_mid=g_mid if act == 0 else None, gate_actout=g_act, gate_out=g_out, **pro)
    fa = O.fake_quant(lin[0::2], outs[0].scale, outs[0].offset, 0, outs[0].qmax)
    fb = O.fake_quant(lin[1::2], outs[1].scale, outs[1].offset, 0, outs[1].qmax)
    r = O.qsilu(fa, None, g_mid, g_act) if act == 0 else O.qgelu(fa, None, g_act)
    q = O.quantize_index((r * fb).astype(F32), g_out.scale, g_out.offset, 0, 255).astype(np.int64) - 128
    assert np.array_equal(gate["gate_q_div"].astype(np.int64), q)
    assert np.abs(gate["gate_q"].astype(np.int64) - q).max() <= 2


def test_decode_gemv_oracle_wraps_int32_and_reads_xq():
    """tt wraps like the kernel's unsigned arithmetic; XM_I8 contracts the given image; XM_F32 quantises the row itself."""
    K = 256
    xq = np.full(K, 127, np.int8)
    w = np.full((2, K), -128, np.int8)
    zp = np.array([2 ** 30, -(2 ** 30)], np.int32)
    ct = np.array([2 ** 31 - 1, 5], np.int32)
    got = O.decode_gemv_launch(K, 2, w, np.ones(2, F32), zp, ct, xq=xq)
    s = -128 * 127 * K
    want = [(s - int(z) * 127 * K + int(c)) for z, c in zip(zp, ct)]
    want = [((v + 2 ** 31) % 2 ** 32) - 2 ** 31 for v in want]
    assert got["rs"] == 127 * K and got["tt"].tolist() == want and got["y"].tolist() == [float(F32(v)) for v in want]
    x = np.linspace(-4, 4, K).astype(F32)
    ag = _grid(8, -3.0, 3.0)
    f = O.decode_gemv_prologue(K, x=x, a_grid=ag)
    ok = ~f["tie"]
    assert np.array_equal(f["image"][ok].astype(np.int64) + 128, O.quantize_index(x, ag.scale, ag.offset, 0, 255)[ok].astype(np.int64))


def test_packed_w4_round_trips_and_contracts_as_unpacked():
    rng = np.random.default_rng(4)
    q = rng.integers(0, 16, (5, 256))
    q[0, :] = 15
    q[1, :] = 0
    p = O.pack_w4(q, 0)
    assert np.array_equal(O.unpack_w4(p, 0), q)
    assert p[2, 3] == (q[2, 3] | (q[2, 19] << 4)) and p[2, 16 + 3] == (q[2, 35] | (q[2, 51] << 4))
    a = rng.integers(-128, 128, 256).astype(np.int8)
    assert np.array_equal(O.decode_gemv_sums(a, p, w4=True), q @ a.astype(np.int64))


@pytest.mark.parametrize("mode", ["rms", "rms_now", "ln", "ln_nob", "ln_now", "none"])
@pytest.mark.parametrize("K", [256, 260, 2052])
def test_decode_head_oracle_is_the_float64_reference(mode, K):
    """decode_head_norm / decode_head_logits against torch in float64; the bound covers the fp32 evaluation in the kernel's order."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(K)
    V = 37
    x = (rng.standard_normal(K) * 3 + 0.5).astype(F32)
    nw = rng.uniform(0.5, 1.5, K).astype(F32)
    nb = (rng.standard_normal(K) * 0.1).astype(F32)
    w = (rng.standard_normal((V, K)) * 0.05).astype(F32)
    b = (rng.standard_normal(V) * 0.1).astype(F32)
    ln = mode.startswith("ln")
    wt = None if mode in ("rms_now", "ln_now", "none") else nw
    bt = nb if mode == "ln" or mode == "ln_now" else None
    X = torch.from_numpy(x).double()
    if ln:
        h = torch.nn.functional.layer_norm(X, (K,), None if wt is None else torch.from_numpy(wt).double(),
                                           None if bt is None else torch.from_numpy(bt).double(), eps=float(F32(1e-5)))
    elif wt is not None:
        h = torch.from_numpy(wt).double() * (X * torch.rsqrt((X * X).mean() + float(F32(1e-5))))
    else:
        h = X
    want = torch.from_numpy(w).double() @ h + torch.from_numpy(b).double()
    s64, err = O.decode_head_norm(x, wt, bt, int(ln), 1e-5)
    lg, bound = O.decode_head_logits(w.astype(np.float64), s64, err, b.astype(np.float64))
    assert np.allclose(s64, h.numpy(), rtol=1e-12, atol=1e-12) and np.allclose(lg, want.numpy(), rtol=1e-12, atol=1e-12)
    # an fp32 evaluation in the kernel's order stays inside the bound
    xs = x.copy()
    if ln:
        mu = F32(np.float32(x.astype(np.float64).sum()) / F32(K))
        var = F32(np.float32(((x - mu).astype(F32) ** 2).astype(np.float64).sum()) / F32(K))
        r = F32(F32(1) / np.sqrt(F32(var + F32(1e-5))))
        xs = ((x * r).astype(F32) + F32(-r * mu)).astype(F32)
        if wt is not None:
            xs = (xs * wt).astype(F32)
        if bt is not None:
            xs = (xs + bt).astype(F32)
    elif wt is not None:
        r = F32(F32(1) / np.sqrt(F32(F32((x * x).astype(F32).sum(dtype=F32)) / F32(K)) + F32(1e-5)))
        xs = (wt * (x * r).astype(F32)).astype(F32)
    lg32 = ((w * xs).astype(F32).sum(axis=1, dtype=F32) + b).astype(F32)
    assert np.all(np.abs(lg32 - lg) <= bound), float((np.abs(lg32 - lg) / bound).max())
    assert np.all(bound < 1e-3 * np.abs(w).sum(1))


def test_decode_gemv_c_entry_refuses_k_beyond_its_limits():
    """The K limits the C entry states: fp32 rows up to 8192, OPRE up to 4096, xq up to 32768, K % 256 == 0 (host checks only)."""
    from mobilequant_amd import _lib
    from mobilequant_amd._lib import MqDecodeGemvArgs, MqGrid
    fake = 1 << 20
    g8 = MqGrid(fake, fake, 0.0, 255.0)

    def args(K, **f):
        a = MqDecodeGemvArgs()
        a.w = a.alpha = a.w_zp = a.col_term = a.consts = a.y = fake
        a.K, a.N, a.a_grid = K, 8, g8
        for k, v in f.items():
            setattr(a, k, v)
        return a

    for a, msg in ((args(8192 + 256, x=fake), "8192"), (args(32768 + 256, xq=fake), "32768"), (args(2304 + 4, xq=fake), "multiple of 256"),
                   (args(4096 + 256, x=fake, norm_w=fake, gate_q=fake, out_grid=(MqGrid * 3)(g8, g8, g8), gate_out=g8, o_acc=fake, o_alpha=fake,
                         o_ct=fake, x_mid=fake), "K <= 4096")):
        with pytest.raises(_lib.MobileQuantLibraryError, match=msg):
            _lib.call("mq_decode_gemv", ctypes.byref(a), None)
