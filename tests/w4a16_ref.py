"""numpy oracle of the W4A16 contract, float64 where the contract says "exact".

For a weight W [N, K] with a 4-bit per-(row, group) grid (scale s, offset z, fp32, [N, G], G = K / g):
    index   q   = clamp(rint(w / s) + z, qmin, qmax)       oracle.mq_oracle.quantize_index (Quantizer.forward)
    nibble  u   = q - qmin  (0..15);  zero z' = z - qmin (an integer, |z'| <= 1024);  s16 = fp16(s)
    w16         = fp16(s16 * (u - z'))                      the product is exact in float64: one rounding
    x16         = fp16(x)
    y64         = sum_k x16 * w16 + bias                    float64
and the kernel's y within  2 K 2^-24 sum_k |x16 w16| + ulp_out(|y64|)  of y64 (any order of K fp32 additions of exact products, doubled
because the MFMA's internal accumulation rounding is not documented as round-to-nearest; the ulp covers the bias add and the final
rounding).  The packed layout is restated here from include/mobilequant_amd.h, independently of oracle.pack_w4.
"""
import numpy as np

from oracle import mq_oracle as O

F16, F32, F64 = np.float16, np.float32, np.float64
BITS = 4


def limits(is_symmetric):
    return O.qrange(BITS, is_symmetric)


def groups(K, g):
    g = K if g == -1 else g
    assert g > 0 and K % g == 0
    return g, K // g


def grid_from_minmax(w, is_symmetric, g):
    """(scale, offset) fp32 [N, G] of the per-group min / max grid (compute_min_max_from_tensor + compute_scale_offset_from_min_max)."""
    w = np.asarray(w, F32)
    N, K = w.shape
    g, G = groups(K, g)
    mn, mx = O.min_max_from_tensor(w, True, g)
    s, o, _, _ = O.scale_offset_from_min_max(mn, mx, BITS, is_symmetric)
    return s.reshape(N, G).astype(F32), o.reshape(N, G).astype(F32)


def index(w, scale, offset, is_symmetric, g):
    """q [N, K] as fp32 integers."""
    w = np.asarray(w, F32)
    N, K = w.shape
    g, G = groups(K, g)
    qmin, qmax = limits(is_symmetric)
    q = O.quantize_index(w.reshape(N * G, g), np.asarray(scale, F32).reshape(-1, 1), np.asarray(offset, F32).reshape(-1, 1), qmin, qmax)
    return q.reshape(N, K)


def stored(w, scale, offset, is_symmetric, g):
    """(u uint8 [N, K], s16 fp16 [N, G], z' fp16 [N, G])."""
    qmin, _ = limits(is_symmetric)
    q = index(w, scale, offset, is_symmetric, g)
    u = (q - F32(qmin)).astype(np.int32)
    assert u.min() >= 0 and u.max() <= 15
    N, K = q.shape
    _, G = groups(K, g)
    zp = (np.asarray(offset, F32).reshape(N, G) - F32(qmin)).astype(F32)
    assert np.all(zp == np.rint(zp)) and np.all(np.abs(zp) <= 1024)
    return u.astype(np.uint8), np.asarray(scale, F32).reshape(N, G).astype(F16), zp.astype(F16)


def dequant_f32(u, scale, zp, g):
    """(u - z') * s in fp32 with the fp32 scale: the reference's fake-quant value (q - z) * s, since u - z' = q - z exactly."""
    N, K = u.shape
    g, G = groups(K, g)
    d = (u.astype(F32).reshape(N, G, g) - np.asarray(zp, F32).reshape(N, G, 1)).astype(F32)
    return (d * np.asarray(scale, F32).reshape(N, G, 1)).astype(F32).reshape(N, K)


def pack(u):
    """mq_pack_w4: byte j (0..15) of each 16-byte group holds element j (low nibble) and element j + 16 (high nibble) of a 32-wide
    k block."""
    u = np.asarray(u, np.uint8)
    N, K = u.shape
    assert K % 32 == 0
    out = np.zeros((N, K // 2), np.uint8)
    for kb in range(K // 32):
        for j in range(16):
            out[:, kb * 16 + j] = u[:, kb * 32 + j] | (u[:, kb * 32 + 16 + j] << 4)
    return out


def unpack(p):
    p = np.asarray(p, np.uint8)
    N, half = p.shape
    u = np.zeros((N, half * 2), np.uint8)
    for kb in range(half // 16):
        for j in range(16):
            u[:, kb * 32 + j] = p[:, kb * 16 + j] & 15
            u[:, kb * 32 + 16 + j] = p[:, kb * 16 + j] >> 4
    return u


def w16(u, s16, zp16, g):
    """fp16 [N, K]: one rounding of the exact product."""
    N, K = u.shape
    g, G = groups(K, g)
    d = u.astype(F64).reshape(N, G, g) - np.asarray(zp16, F16).astype(F64).reshape(N, G, 1)
    return (np.asarray(s16, F16).astype(F64).reshape(N, G, 1) * d).reshape(N, K).astype(F16)


def x16(x):
    return np.asarray(x).astype(F16)


def linear64(x, w16_, bias=None):
    """(y64 [M, N], sum_k |x16 w16| [M, N]) in float64."""
    a, b = x16(x).astype(F64), np.asarray(w16_, F16).astype(F64)
    y = a @ b.T
    if bias is not None:
        y = y + np.asarray(bias, F32).astype(F64)[None, :]
    return y, np.abs(a) @ np.abs(b).T


def ulp_out(y64, out_dtype):
    """one ulp of the output dtype at |y64|: 2^-23 (fp32) or 2^-10 (fp16) relative, with the fp16 subnormal spacing as the floor."""
    a = np.abs(y64)
    if out_dtype == F32:
        return np.maximum(a * 2.0 ** -23, 2.0 ** -149)
    return np.maximum(a * 2.0 ** -10, 2.0 ** -24)


def bound(K, sumabs, y64, out_dtype):
    return 2.0 * K * 2.0 ** -24 * sumabs + ulp_out(y64, out_dtype)
