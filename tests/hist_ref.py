"""numpy reference of the bit-pattern histogram and of the percentile range read from it, written from the rule's text (DESIGN.md
4.1h), not from the implementation.

Bins.  mantissa_bits m in 0..6, NB = 256 << m magnitude keys, 2 NB bins.  For an element x (fp16 converted to fp32 first: exact),
u = bits(x): -0 counts as +0; a NaN goes to a separate nan_count and to no bin; otherwise mag = (u & 0x7fffffff) >> (23 - m),
bin = NB + mag for x >= 0 and NB - 1 - mag for x < 0.  With f(k) = float_from_bits(min(k, 255 << m) << (23 - m)) a non-negative bin of
key k holds [f(k), f(k + 1)), a negative one (-f(k + 1), -f(k)].

Range.  counts c[0 .. 2 NB), N = sum c, the observed exact mn / mx, a coverage p in (0, 1]: tail = floor((1.0 - p) * 0.5 * N) in
IEEE double in exactly this order; lo = the lowest bin with sum_{i <= lo} c[i] > tail, hi = the highest bin with
sum_{i >= hi} c[i] > tail; min = max(lower bound of lo, mn), max = min(upper bound of hi, mx), both fp32."""
import math

import numpy as np


def nb_of(m):
    return 256 << m


def bin_index(x, m):
    """(bin of every element as int64, NaN mask); the bin of a NaN is meaningless."""
    x = np.ascontiguousarray(np.asarray(x).astype(np.float32).reshape(-1))
    u = x.view(np.uint32).astype(np.int64)
    a = u & 0x7FFFFFFF
    nan = a > 0x7F800000
    mag = a >> (23 - m)
    neg = ((u >> 31) == 1) & (a != 0)                   # -0 counts as +0
    nb = nb_of(m)
    return np.where(neg, nb - 1 - mag, nb + mag), nan


def histogram(x, m):
    """(counts int64 [2 NB], nan_count)."""
    b, nan = bin_index(x, m)
    return np.bincount(b[~nan], minlength=2 * nb_of(m)).astype(np.int64), int(nan.sum())


def minmax(x):
    """torch.min / torch.max semantics on the fp32 values: NaN if any, zeros compare equal (returned as +0)."""
    x = np.asarray(x).astype(np.float32).reshape(-1)
    if np.isnan(x).any():
        return np.float32(np.nan), np.float32(np.nan)
    return np.float32(x.min() + np.float32(0)), np.float32(x.max() + np.float32(0))


def _f(k, m):
    k = np.minimum(np.asarray(k, dtype=np.int64), 255 << m)
    return (k << (23 - m)).astype(np.uint32).view(np.float32)


def bin_bounds(m):
    """fp32 (lo[2 NB], hi[2 NB]): lo inclusive / hi exclusive for the non-negative bins, lo exclusive / hi inclusive for the negative."""
    nb = nb_of(m)
    lo, hi = np.empty(2 * nb, np.float32), np.empty(2 * nb, np.float32)
    k = np.arange(nb)
    lo[nb + k], hi[nb + k] = _f(k, m), _f(k + 1, m)
    lo[nb - 1 - k], hi[nb - 1 - k] = -_f(k + 1, m), -_f(k, m)
    return lo, hi


def percentile_bins(counts, p):
    c = [int(v) for v in counts]
    n = sum(c)
    tail = math.floor((1.0 - p) * 0.5 * n)
    acc, lo = 0, None
    for i in range(len(c)):
        acc += c[i]
        if acc > tail:
            lo = i
            break
    acc, hi = 0, None
    for i in range(len(c) - 1, -1, -1):
        acc += c[i]
        if acc > tail:
            hi = i
            break
    return lo, hi, tail, n


def percentile_range(counts, mn, mx, p, m):
    """(min, max) as np.float32."""
    lo, hi, _, _ = percentile_bins(counts, p)
    blo, bhi = bin_bounds(m)
    return max(blo[lo], np.float32(mn)), min(bhi[hi], np.float32(mx))


def planted_data(n, seed, fp16=False):
    """N(0, 1) with the awkward values planted at fixed places (as many as fit into n): +-0, fp32 and fp16 denormals, +-inf, NaNs,
    +-max finite, values exactly on bin bounds (powers of two, 1 + k * 2^-m for m = 3, 5, 6) and the nextafter neighbour on each side."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n).astype(np.float32)
    f32max = np.finfo(np.float32).max
    special = [0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 6e-8, -6e-8, 5.96e-8, np.inf, -np.inf, np.nan, np.nan, -np.nan, f32max, -f32max,
               65504.0, -65504.0]
    edges = [2.0 ** e for e in (-20, -3, -1, 0, 1, 2, 10)] + [1.0 + k * 2.0 ** -mm for mm in (3, 5, 6) for k in (1, 3, 2 ** mm - 1)]
    dt = np.float16 if fp16 else np.float32
    with np.errstate(over="ignore"):
        special = list(np.array(special, dtype=np.float32).astype(dt))      # (fp16: fp32 extremes become +-inf, tiny ones 0 or fp16 denormals)
    for e in edges:
        e = dt(e)
        for s in (dt(1.0), dt(-1.0)):
            special += [s * e, s * np.nextafter(e, dt(np.inf)), s * np.nextafter(e, dt(0))]
    special = np.array(special, dtype=dt)
    x = x.astype(dt)
    k = min(n, special.size)
    pos = rng.permutation(n)[:k]
    x[pos] = special[rng.permutation(special.size)[:k]]
    return x
