"""Inputs and case list of the mq_w8a8_linear_grouped pin, built once for the CPU checks (test_qmatmul_oracle.py) and the GPU comparison
(test_gpu_gemm_grouped.py): both files take every operand and vector from here.

The kernel (csrc/mq_gemm_grouped.hip) has two instantiations -- 128 bytes of K per LDS buffer when group_size % 128 == 0, else 64
(kernel_of) -- and one fixed sequence of operations per output (oracle.grouped_linear).  Content:
  random   int8 operands over the whole range, true per-group activation sums, cw within +-383, t within +-2^20
  ties     rows and columns of saturated operands at group_size >= 2048 and a chosen t: brackets beyond 2^24 that are EXACT ties of the
           int32 -> fp32 conversion, of both parities and both signs, in [2^24, 2^25), [2^25, 2^26) and [2^30, 2^31)
  mul24    cw = +-(2^23 - 1), the edge of the 24-bit multiply, against |a_gsum| <= 250 (the product fits int32)
  big      group_size 32768, with a saturated row and column: P = 2^29, a_gsum = -2^22
Every case's brackets are asserted inside int32 in int64 arithmetic (oracle.grouped_linear does it)."""
import functools
import zlib
from collections import namedtuple

import numpy as np

from oracle import mq_oracle as O

F32 = np.float32

GCase = namedtuple("GCase", "id M N gs G bias content", defaults=(True, "random"))
CASES = [
    # 64 bytes of K per buffer: group_size % 128 != 0
    GCase("g64-G1-M1", 1, 128, 64, 1),
    GCase("g64-G2", 127, 384, 64, 2, False),
    GCase("g192-G3", 128, 128, 192, 3),
    GCase("g320-G5", 129, 128, 320, 5, False),
    GCase("g192-G2-M300", 300, 384, 192, 2),
    GCase("g64-G7", 129, 128, 64, 7),
    # 128 bytes per buffer
    GCase("g128-G1", 129, 128, 128, 1, False),
    GCase("g128-G2-M1", 1, 384, 128, 2),
    GCase("g256-G3", 127, 128, 256, 3),
    GCase("g384-G5-M300", 300, 128, 384, 5, False),
    GCase("g256-G6", 128, 384, 256, 6),
    GCase("g128-G3-M300", 300, 128, 128, 3),
    # brackets beyond 2^24 on exact conversion ties
    GCase("ties-g2048-G3", 20, 128, 2048, 3, True, "ties"),
    GCase("ties-g2112-G2", 20, 128, 2112, 2, False, "ties"),
    # the 24-bit multiply's edge
    GCase("mul24-g64-G3", 129, 128, 64, 3, True, "mul24"),
    GCase("mul24-g128-G2", 127, 128, 128, 2, False, "mul24"),
    # the largest group
    GCase("big-g32768-G2", 16, 128, 32768, 2, True, "big"),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
ALL_KERNELS = ["bks128", "bks64"]
SAT_ROWS = 10         # "ties": rows 0 .. 9 hold -128 throughout


def kernel_of(c):
    """The instantiation mq_w8a8_linear_grouped launches: gemm_i8_grouped_kernel<128> when group_size % 128 == 0, else <64>."""
    return "bks128" if c.gs % 128 == 0 else "bks64"


def tie_targets(G, N):
    """int64 [G, N]: brackets that are exact ties of the int32 -> fp32 conversion.  Column class n % 3: 2^24 + 2 j + 1 (spacing 2),
    2^25 + 4 j + 2 (spacing 4), 2^31 - 2^28 - 192 - 128 j (spacing 128: 64 mod 128); j = n // 3 runs through both parities of the kept mantissa;
    the sign alternates with g + n."""
    n = np.arange(N, dtype=np.int64)[None, :]
    g = np.arange(G, dtype=np.int64)[:, None]
    j = n // 3
    mag = np.where(n % 3 == 0, 2 ** 24 + 2 * j + 1, np.where(n % 3 == 1, 2 ** 25 + 4 * j + 2, 2 ** 31 - 2 ** 28 - 192 - 128 * j))
    return np.where((g + n) % 2 == 0, mag, -mag)


def is_conversion_tie(v):
    """v int64: fl32(v) is a tie (v lies exactly between two neighbouring fp32 values)."""
    v = np.abs(np.asarray(v, np.int64))
    e = np.floor(np.log2(np.maximum(v, 1).astype(np.float64))).astype(np.int64)
    step = np.where(e >= 24, 2 ** np.maximum(e - 23, 0), 1)
    return (e >= 24) & (v % step == step // 2)


@functools.lru_cache(maxsize=None)
def problem(cid):
    """dict(a int8 [M, K], w int8 [N, K], a_gsum int32 [G, M], alpha fp32 [G, N], cw / t int32 [G, N], bias fp32 [N] | None), read-only."""
    c = BY_ID[cid]
    M, N, gs, G = c.M, c.N, c.gs, c.G
    K = gs * G
    rng = np.random.default_rng(zlib.crc32(repr(tuple(c)).encode()))
    a = rng.integers(-128, 128, (M, K), dtype=np.int64).astype(np.int8)
    w = rng.integers(-128, 128, (N, K), dtype=np.int64).astype(np.int8)
    alpha = (F32(0.031) * (F32(1e-3) + F32(4e-3) * rng.random((G, N)).astype(F32))).astype(F32)
    cw = rng.integers(-383, 384, (G, N), dtype=np.int64)
    t = rng.integers(-2 ** 20, 2 ** 20, (G, N), dtype=np.int64)
    if c.content == "ties":
        a[:SAT_ROWS] = -128
        w[::2] = -128                                         # even columns saturated as well: P = 2^14 group_size in those
    elif c.content == "big":
        a[0] = -128
        w[0] = -128
        cw = rng.integers(-255, 256, (G, N), dtype=np.int64)
    ag = a.astype(np.int64).reshape(M, G, gs).sum(axis=2).T.copy()            # [G, M], the true sums
    if c.content == "ties":
        wsum = w.astype(np.int64).reshape(N, G, gs).sum(axis=2).T            # [G, N]
        # in a saturated row P = -128 W_g[n] and a_gsum = -128 group_size: t makes the bracket the chosen tie
        t = tie_targets(G, N) + 128 * wsum + cw * 128 * gs
    elif c.content == "mul24":
        cw = np.where((np.arange(G)[:, None] + np.arange(N)[None, :]) % 2 == 0, 2 ** 23 - 1, -(2 ** 23 - 1)).astype(np.int64)
        ag = rng.integers(-250, 251, (G, M), dtype=np.int64)                  # given, not the sums of a: the kernel takes the vector as it is
        ag[:, 0] = 250
        ag[:, -1] = -250
    assert np.abs(t).max() < 2 ** 31
    bias = (rng.standard_normal(N) * 0.2).astype(F32) if c.bias else None
    p = dict(a=a, w=w, a_gsum=ag.astype(np.int32), alpha=alpha, cw=cw.astype(np.int32), t=t.astype(np.int32), bias=bias)
    for v in p.values():
        if v is not None:
            v.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def expect(cid, mutation=None):
    c, p = BY_ID[cid], problem(cid)
    return O.grouped_linear(p["a"], p["w"], c.gs, p["a_gsum"], p["alpha"], p["cw"], p["t"], p["bias"], mutation)
