"""The decode-cache <-> image-cache bridge (mq_attention_cache_import / mq_attention_cache_export) restated element by element from the
layout statement above mq_attention_args / mq_attention_cache_args in include/mobilequant_amd.h.  numpy, no GPU.

Every array is built by writing value(h, t, d) at the FLAT index the header gives for (h, t, d): no view / permute / transpose anywhere,
so this is a second statement next to the permute-based helpers of test_gpu_prefill_append.py and the view-based ones of
test_gpu_prefill_attention.py, not a copy of either.  Everything is exact integer arithmetic or data movement.

  import_images(k, v_logical, n, zq, zk, D, want_f16, rows=None, before=None) -> dict of flat arrays laid out for `rows` image rows
  export_caches(images, k_before, v_before, p0, n, chunked)                 -> (k, v), whole
  to_chunked(v_logical, chunks=None, before=None) / from_chunked(v_chunked, positions): the chunked value layout"""
import numpy as np

F16_WINDOW = (-256.0, 511.0)       # zk inside: k_f16 holds fp16(index - zk) exactly; outside: every half is NAN_HALF
NAN_HALF = 0x7E00


def _htd(KV, n, D):
    """Index grids h, t, d over [KV, n, D]."""
    return np.meshgrid(np.arange(KV, dtype=np.int64), np.arange(n, dtype=np.int64), np.arange(D, dtype=np.int64), indexing="ij")


def kappa(r):
    """Where key r = 16 j + 4 tq + e of a 64-key block sits in a vT row: 16 tq + 4 j + e."""
    j, tq, e = r // 16, (r % 16) // 4, r % 4
    return 16 * tq + 4 * j + e


def vt_index(h, t, d, blocks, D):
    """vt_i8[h][t / 64][d][kappa]"""
    return ((h * blocks + t // 64) * D + d) * 64 + kappa(t % 64)


def k_f16_index(h, t, d, blocks):
    """The fragment-blocked half index of k_f16 (head_dim 64), as the header gives it."""
    b, r = t // 64, t % 64
    return ((h * blocks + b) * 8 + 2 * (r // 16) + (d % 16) // 8) * 512 + ((r % 16) + 16 * (d // 16)) * 8 + d % 8


def chunked_index(h, t, d, chunks, D):
    """v[h][t / 16][d][t % 16] of the chunked value layout [kv][chunks][D][16]."""
    return ((h * chunks + t // 16) * D + d) * 16 + t % 16


def to_chunked(v_logical, chunks=None, before=None):
    """v [KV, L, D] -> [KV, chunks, D, 16] (chunks >= L / 16; chunks past the positions keep `before`, or zero)."""
    KV, L, D = v_logical.shape
    assert L % 16 == 0
    chunks = L // 16 if chunks is None else chunks
    out = np.zeros((KV, chunks, D, 16), np.int8) if before is None else np.array(before, dtype=np.int8).reshape(KV, chunks, D, 16)
    h, t, d = _htd(KV, L, D)
    out.reshape(-1)[chunked_index(h, t, d, chunks, D)] = v_logical[h, t, d]
    return out


def from_chunked(v_chunked, positions):
    """[KV, chunks, D, 16] -> v [KV, positions, D]."""
    KV, chunks, D, _ = v_chunked.shape
    h, t, d = _htd(KV, positions, D)
    return np.ascontiguousarray(v_chunked).reshape(-1)[chunked_index(h, t, d, chunks, D)].astype(np.int8)


def import_images(k, v_logical, n, zq, zk, D, want_f16, rows=None, before=None):
    """The images of positions 0 .. n - 1 of k / v_logical [KV, >= n, D] int8 (stored bytes = index - 128), laid out for `rows` image rows
    (default n).  zq / zk: the offsets of qk_a / qk_b.  Returns flat arrays: k_i8, vt_i8 (int8), k_rs (int64: the caller checks that it
    fits int32), v_pre (int64; None at head_dim 64), k_f16 (uint16 bit patterns; None unless head_dim 64 and want_f16), and rows.
    Elements of rows >= n keep `before` (a dict of flat arrays of the same sizes), or zero."""
    KV = k.shape[0]
    assert k.shape[2] == D and v_logical.shape[2] == D and n % 64 == 0 and 0 < n <= k.shape[1] and n <= v_logical.shape[1]
    rows = n if rows is None else rows
    assert rows % 64 == 0 and n <= rows
    blocks = rows // 64

    def start(name, size, dtype):
        return np.zeros(size, dtype) if before is None or before.get(name) is None else np.array(before[name]).reshape(-1).astype(dtype)

    out = {"rows": rows, "v_pre": None, "k_f16": None}
    h, t, d = _htd(KV, n, D)
    kv, vv = k[h, t, d].astype(np.int64), v_logical[h, t, d].astype(np.int64)

    out["k_i8"] = start("k_i8", KV * rows * D, np.int8)
    out["k_i8"][(h * rows + t) * D + d] = kv

    zq = int(zq)
    out["k_rs"] = start("k_rs", KV * rows, np.int64)
    row = np.zeros((KV, n), np.int64)
    for dd in range(D):
        row += kv[:, :, dd]
    out["k_rs"][h[:, :, 0] * rows + t[:, :, 0]] = -(zq - 128) * row

    out["vt_i8"] = start("vt_i8", KV * rows * D, np.int8)
    out["vt_i8"][vt_index(h, t, d, blocks, D)] = vv

    if D != 64:
        out["v_pre"] = start("v_pre", KV * blocks * D, np.int64)
        run = np.zeros((KV, D), np.int64)
        for b in range(n // 64):
            for tt in range(64 * b, 64 * b + 64):
                run += vv[:, tt]
            out["v_pre"][(h[:, 0] * blocks + b) * D + d[:, 0]] = run

    if D == 64 and want_f16:
        out["k_f16"] = start("k_f16", KV * rows * D, np.uint16)
        if F16_WINDOW[0] <= float(zk) <= F16_WINDOW[1]:
            c = (kv + 128).astype(np.float32) - np.float32(zk)
            half = c.astype(np.float16)
            assert np.array_equal(half.astype(np.float32), c), "fp16(index - zk) must be exact inside the window"
            bits = half.view(np.uint16)
        else:
            bits = np.full(kv.shape, NAN_HALF, np.uint16)
        out["k_f16"][k_f16_index(h, t, d, blocks)] = bits
    return out


def export_caches(images, k_before, v_before, p0, n, chunked):
    """Rows p0 .. p0 + n - 1 of images["k_i8"] / images["vt_i8"] (flat, images["rows"] rows) written into copies of the decode caches
    k_before [KV, positions, D] and v_before ([KV, positions, D], or chunked [KV, chunks, D, 16]): the allocation as a whole, pad rows /
    chunks behind the cache's positions included.  No other byte changes."""
    KV, _, D = k_before.shape
    rows = images["rows"]
    blocks = rows // 64
    assert n > 0 and p0 >= 0 and p0 + n <= rows and p0 + n <= k_before.shape[1]
    k, v = np.array(k_before, dtype=np.int8), np.array(v_before, dtype=np.int8)
    h, t, d = _htd(KV, n, D)
    t = t + p0
    k.reshape(-1)[(h * k.shape[1] + t) * D + d] = images["k_i8"][(h * rows + t) * D + d]
    val = images["vt_i8"][vt_index(h, t, d, blocks, D)]
    if chunked:
        assert v.shape[2:] == (D, 16) and p0 + n <= 16 * v.shape[1]
        v.reshape(-1)[chunked_index(h, t, d, v.shape[1], D)] = val
    else:
        assert v.shape[2] == D and p0 + n <= v.shape[1]
        v.reshape(-1)[(h * v.shape[1] + t) * D + d] = val
    return k, v
