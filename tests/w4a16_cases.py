"""Case table of the W4A16 launch-branch pin (numpy only: no torch, no GPU): tests/test_w4a16_oracle.py checks the table on the host,
tests/test_gpu_w4a16_oracle.py runs it through mq_w4a16_linear.  The oracle is tests/w4a16_ref.py; nothing of the contract is restated.

plan() mirrors the launch arithmetic of mq_w4a16_linear (csrc/mq_w4a16.hip): which kernel, which instantiation, how many rows a
workgroup and a wave take, how many chunk passes a row needs, how much LDS, which arm of group_of.  Its constants stand once, below; the
host test reads the same constants out of the source and compares.  Every shape that depends on the CU count is an expression of `cus`.

Exact cases: integer x in [-4, 4], random nibbles, scales 2^e drawn per (row, group), integer zeros, a bias that is a multiple of the
smallest scale 2^emin and differs in every row.  Every product and the bias are multiples of 2^emin, so every partial sum of any order
is one too, of magnitude at most sum_k |x16 w16| + |bias|; the builder asserts  max(sum_k |x16 w16| + |bias|) / 2^emin < 2^24  on the
oracle's own output, and then every partial sum is an fp32 number: the result is the float64 oracle bit for bit whatever the order."""
import functools
from collections import namedtuple

import numpy as np

import w4a16_ref as R

F16, F32, F64 = np.float16, np.float32, np.float64

# ---- the launch constants of csrc/mq_w4a16.hip (audited against the source by tests/test_w4a16_oracle.py) ---------------------------------
WV_THREADS, WV_WAVES = 1024, 16
WV_MAX_LDS = 128 * 1024
WV_INFLIGHT = {1: 8, 2: 8, 4: 8, 8: 4}        # chunks in flight per lane, by MT
LDS_ATTR_ABOVE = 32768                        # dynamic LDS above this: the hipFuncSetAttribute branch
WV_MAX_SLOTS = 64                             # row slots per wave (rows_per_wg <= WV_WAVES * WV_MAX_SLOTS)
GM_BM, GM_BN, GM_BK = 64, 64, 128
CU_COUNTS = (64, 256, 304)                    # the host test's; the GPU test passes the device's own


def _cdiv(a, b):
    return -(-a // b)


def variant(M, N, K, g):
    """w4a16_variant of the source (0: not served, 1: GEMV, 2: GEMM), g already resolved."""
    if not (1 <= M <= 1 << 30) or N < 16 or N % 16 or N > 65535 * GM_BN or K < 64 or K % 64 or K > 1 << 24 or g < 32 or g % 32 or K % g:
        return 0
    return 1 if M <= 8 and M * K * 2 <= WV_MAX_LDS else 2


def plan(M, N, K, g, cus):
    """The launch mq_w4a16_linear makes for x [M, K] and weights [N, K] with groups of g (-1: K) on a part with `cus` CUs."""
    g = K if g == -1 else g
    g32 = g // 32
    p = dict(M=M, N=N, K=K, g=g, cus=cus, variant=variant(M, N, K, g), group_div=g32 & (g32 - 1) != 0)
    if p["variant"] == 1:
        MT = 1 if M == 1 else 2 if M == 2 else 4 if M <= 4 else 8
        rows_per_wg = min(_cdiv(N, cus), WV_WAVES * WV_MAX_SLOTS)
        grid = _cdiv(N, rows_per_wg)
        kchunks = K // 32
        cpl = _cdiv(kchunks, 64)
        last = N - (grid - 1) * rows_per_wg                       # rows of the last workgroup
        first = min(rows_per_wg, N)
        nslots_max = _cdiv(first, WV_WAVES)                       # wave 0 of the first workgroup
        nslots_min = _cdiv(max(first - (WV_WAVES - 1), 0), WV_WAVES)                               # its wave 15
        lds = M * K * 2
        p.update(MT=MT, m_guard=M < MT, inflight=WV_INFLIGHT[MT], rows_per_wg=rows_per_wg, grid=grid, last_wg_rows=last,
                 nslots_max=nslots_max, nslots_min=nslots_min, kchunks=kchunks, cpl=cpl, clamped_lanes=cpl * 64 - kchunks, lds=lds,
                 lds_attr=lds > LDS_ATTR_ABOVE, passes=_cdiv(nslots_max * cpl, WV_INFLIGHT[MT]))
        # a refill that starts inside a row: the chunks of a pass are not a whole number of rows
        p["midrow_refill"] = p["passes"] >= 2 and WV_INFLIGHT[MT] % cpl != 0
    elif p["variant"] == 2:
        NT = 2 if N > GM_BN else 1
        p.update(NT=NT, grid=(_cdiv(M, GM_BM), _cdiv(N, GM_BN * NT)), nchunks=_cdiv(K, GM_BK), ktail=K % GM_BK, groups_per_chunk=GM_BK / g,
                 group_wide=g > GM_BK, group_splits_chunk=any(b % GM_BK for b in range(g, K, g)))
    return p


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def exact_x(rng, M, K):
    x = rng.integers(-4, 5, size=(M, K)).astype(F32)
    x[:, 0] = 3.0                                             # (no all-zero row even at K = 64)
    return x


def one_hot_x(rng, M, K):
    """Row m reads out weight column k_m (value 1), and -- from the second row on -- a second column with weight -2."""
    x = np.zeros((M, K), F32)
    for m in range(M):
        x[m, rng.integers(0, K)] = 1.0
        if m:
            x[m, (7 * m + 3) % K] += -2.0
    return x


ZLIM = (-1024, -1023, 0, 1009, 1023, 1024)

# id, M, N(cus), K, g, scale exponents (lo, hi inclusive), zeros (None: integers in [-3, 18]), x dtypes, one-hot too,
# reaches: the plan fields the case is there for (asserted one by one in tests/test_w4a16_oracle.py)
Case = namedtuple("Case", "id M N K g e zeros xdts one_hot reaches")


def _c(id, M, N, K, g, reaches, e=(-6, -1), zeros=None, xdts=(F32, F16), one_hot=False):
    return Case(id, M, N, K, g, e, zeros, xdts, one_hot, tuple(reaches.split()))


def slots3_n(cus):
    """Three row slots in the first waves and a short last workgroup: N = 32 cus + 16 + 16 r with the smallest r >= 1 for which N is no
    multiple of rows_per_wg = ceil(N / cus) (33 .. 48)."""
    for r in range(1, 64):
        N = 32 * cus + 16 + 16 * r
        rows = _cdiv(N, cus)
        if rows <= 48 and N % rows:
            return N
    raise AssertionError("no ragged three-slot N at %d CUs" % cus)


def exact_cases(cus):
    """The table of the issue, at the smallest shapes that still reach each branch (x dtypes: both unless noted)."""
    n2 = 16 * cus + 16
    out = [_c("slots2-m%d" % M, M, n2, 128, 64, "slots2 ragged_slots", one_hot=M == 3) for M in (1, 3, 8)]
    out += [
        _c("slots3-ragged", 2, slots3_n(cus), 64, 32, "slots3 short_last_wg"),
        _c("slotsxpasses", 8, n2, 4160, 64, "slots2 cpl3 passes2 midrow_refill clamped mt8", e=(-3, -1)),
        _c("slotsxpasses-m2", 2, 32 * cus + 16, 2112, -1, "slots3 cpl2 clamped62 group_div", e=(-3, -1)),
        _c("longrow", 1, 16, 16448, 64, "cpl9 passes2 lds_attr lds_first", e=(-2, -1), xdts=(F32,), one_hot=True),     # fp32 x only
        _c("lds-max-m1", 1, 16, 65536, 128, "lds_max cpl32 lds_attr", e=(-2, -1), xdts=(F16,)),                         # fp16 x only
        _c("lds-max-m8", 8, 48, 8192, 128, "lds_max lds_attr inflight_exact mt8", e=(-2, -1), xdts=(F32,)),             # fp32 x only
        _c("seam-m8", 8, 48, 8256, 96, "gemm_small_m group_div group_splits_chunk ktail", e=(-2, -1)),
        _c("seam-m1", 1, 16, 65600, 64, "gemm_small_m ktail", e=(-2, -1)),
        _c("cap", 2, 1024 * cus + 16, 64, 32, "cap", xdts=(F16,)),                                           # fp16 x only
    ]
    for M in (3, 17):
        out += [_c("gdiv-m%d-k%d" % (M, K), M, 48, K, g, "group_div" + (" group_splits_chunk" if M > 8 and g == 96 else ""), one_hot=True)
                for K, g in ((192, 96), (320, 160), (384, -1))]
    out += [_c("gwide-g%s" % g, 17, 80, 512, g, "group_wide") for g in (256, -1)]
    out += [_c("mt-m%d" % M, M, 48, 128, 64, "mt%d" % (M if M in (2, 4) else 8) + (" m_guard" if M in (5, 6, 7) else ""))
            for M in (2, 4, 5, 6, 7)]
    out += [_c("zlim-m%d" % M, M, 48, 128, 64, "zlim", e=(-2, -1), zeros=ZLIM) for M in (3, 17)]
    return out


def _seed(case):
    return [case.M, case.N % 65521, case.K, case.g % 97, sum(map(ord, case.id))]


Built = namedtuple("Built", "case u s16 z16 packed w16 bias emin x x_hot bits_needed")


@functools.lru_cache(maxsize=2)
def build_exact(case):
    """Weights, bias and x of an exact case (read-only arrays).  `bits_needed`: log2 of max(sum |x16 w16| + |bias|) / 2^emin over every x the
    case runs -- asserted below 24."""
    rng = np.random.default_rng(_seed(case))
    M, N, K = case.M, case.N, case.K
    gs, G = R.groups(K, case.g)
    u = rng.integers(0, 16, size=(N, K), dtype=np.uint8)
    u[0, :16] = np.arange(16)                                    # all 16 nibbles for sure
    if case.zeros is None:
        z16 = rng.integers(-3, 19, size=(N, G)).astype(F16)
    else:
        z = rng.choice(case.zeros, size=(N, G))
        z.reshape(-1)[:len(case.zeros)] = case.zeros              # each of them present
        z16 = z.astype(F16)
    s16 = (2.0 ** rng.integers(case.e[0], case.e[1] + 1, size=(N, G))).astype(F16)
    emin = case.e[0]
    bias = ((rng.permutation(N) - N // 2) * 2.0 ** emin).astype(F32)          # another bias in every row
    assert len(np.unique(bias)) == N and np.all(bias[16:] != bias[:-16])
    packed, w16 = R.pack(u), R.w16(u, s16, z16, case.g)
    x = exact_x(rng, M, K)
    x_hot = one_hot_x(rng, M, K) if case.one_hot else None
    worst = 0.0
    for xv in (x, x_hot):
        if xv is not None:
            y64, sumabs = R.linear64(xv, w16, bias)
            worst = max(worst, float((sumabs + np.abs(bias.astype(F64))[None, :]).max()))
            assert np.array_equal(y64.astype(F32).astype(F64), y64)
    bits_needed = float(np.log2(worst / 2.0 ** emin))
    assert worst / 2.0 ** emin < 2.0 ** 24, "%s is not order independent: %.1f bits" % (case.id, bits_needed)
    for a in (u, s16, z16, packed, w16, bias, x) + ((x_hot,) if x_hot is not None else ()):
        a.setflags(write=False)
    return Built(case, u, s16, z16, packed, w16, bias, emin, x, x_hot, bits_needed)


def want_f32(b, x, bias):
    """fp32 bits the kernel must give for x (of the dtype it is launched with) -- the float64 oracle, which IS an fp32 number."""
    y64, _ = R.linear64(x, b.w16, bias)
    want = y64.astype(F32)
    assert np.array_equal(want.astype(F64), y64)
    return want


# ---- fp16-out edges --------------------------------------------------------------------------------------------------------------------
# column n of the output is W[n] + bias[n] for every row (one-hot x with a 1), W = s16 (u - z') an fp16 number, bias an fp32 number, the
# sum an fp32 number: the kernel's fp32 value is exact and the fp16 rounding is the only rounding.
_B = 2.0 ** 16 - 2.0 ** 4          # 65520: half way between 65504 and 2^16
EDGE_TARGETS = [65504.0, _B - 2.0 ** -8, _B, -_B, -65504.0, -(_B - 2.0 ** -8),
                1 * 2.0 ** -24, 3 * 2.0 ** -24, 1023 * 2.0 ** -24, 1024 * 2.0 ** -24, -5 * 2.0 ** -24,
                2.0 ** -25, 3 * 2.0 ** -25, -(2.0 ** -25), -3 * 2.0 ** -25, 5 * 2.0 ** -25]
EDGE_N, EDGE_K, EDGE_G = 16, 64, 32

Edge = namedtuple("Edge", "M x packed s16 z16 bias y64 want")


def build_edges(M):
    assert len(EDGE_TARGETS) == EDGE_N
    rng = np.random.default_rng(900 + M)
    N, K, g = EDGE_N, EDGE_K, EDGE_G
    G = K // g
    u = rng.integers(0, 16, size=(N, K), dtype=np.uint8)
    z16, s16 = np.empty((N, G), F16), np.empty((N, G), F16)
    ks = rng.permutation(K)[:M]                                              # row m reads out column ks[m]
    x = np.zeros((M, K), F32)
    x[np.arange(M), ks] = 1.0
    bias = np.zeros(N, F32)
    for n, t in enumerate(EDGE_TARGETS):
        big = abs(t) > 1.0
        s16[n] = F16(32.0) if big else F16(2.0 ** -24)                       # the small columns: an fp16-subnormal scale
        d = (15 if big else 1) * (1 if t > 0 else -1)                        # u - z' at the read-out columns
        z = rng.integers(max(-3, -d), min(18, 15 - d) + 1, size=G)           # 0 <= z + d <= 15
        z16[n] = z
        u[n, ks] = (z[ks // g] + d).astype(np.uint8)
        b = F64(t) - F64(s16[n, 0]) * d
        assert F64(F32(b)) == b                                              # the bias is an fp32 number
        bias[n] = F32(b)
    w16 = R.w16(u, s16, z16, g)
    y64, _ = R.linear64(x, w16, bias)
    assert np.array_equal(y64.astype(F32).astype(F64), y64)                  # sum + bias is exact in fp32: one rounding to fp16
    assert np.array_equal(y64, np.broadcast_to(np.array(EDGE_TARGETS, F64), (M, N)))
    with np.errstate(over="ignore"):
        want = y64.astype(F16)
    return Edge(M, x, R.pack(u), s16, z16, bias, y64, want)


# ---- tolerance cases -------------------------------------------------------------------------------------------------------------------
def tolerance_shapes(cus):
    return [(2, 64, 4160, -1), (1, 32, 16448, 64), (8, 48, 8192, 128), (8, 48, 8256, 96), (5, 16 * cus + 16, 128, 64)]


Gauss = namedtuple("Gauss", "x packed s16 z16 w16 bias")


def build_gaussian(M, N, K, g, xdt):
    """Gaussian w and x on the project's own min / max grid (R.grid_from_minmax); symmetric and asymmetric grids alternate."""
    sym = (M + K // 64) % 2 == 0
    rng = np.random.default_rng([M, N % 65521, K, g % 97])
    w = rng.standard_normal((N, K)).astype(F32)
    x = rng.standard_normal((M, K)).astype(xdt)
    bias = rng.standard_normal(N).astype(F32)
    s, o = R.grid_from_minmax(w, sym, g)
    u, s16, z16 = R.stored(w, s, o, sym, g)
    return Gauss(x, R.pack(u), s16, z16, R.w16(u, s16, z16, g), bias)
