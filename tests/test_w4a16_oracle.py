"""Host side of the W4A16 launch-branch pin (no GPU): tests/w4a16_cases.py against the source it mirrors and the oracle it trusts.

- the launch constants of the case table are the ones in csrc/mq_w4a16.hip, csrc/mq_w4a16_stream.h (the walk) and csrc/mq_common.h (the
  launch geometry and the LDS opt-in), read out of the source;
- at 64, 256 and 304 CUs every case reaches the branch it is in the table for, said by plan(), and the table as a whole reaches every
  branch class of both kernels;
- plan().variant is mq_w4a16_supported, for the table and around both sides of the GEMV / GEMM seam;
- every exact case is independent of the summation order (the builder's own assertion), all 16 nibbles and every zero of the limit list
  occur;
- tests/w4a16_ref.py's w16 and linear64 equal a slow scalar evaluation -- a Python loop over k, the group by integer division, the
  nibbles from the packed bytes through the layout of include/mobilequant_amd.h -- bit for bit on two division-group shapes."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import w4a16_cases as C  # noqa: E402
import w4a16_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mobilequant_amd", "csrc")
SRC = open(os.path.join(CSRC, "mq_w4a16.hip")).read()
STREAM = open(os.path.join(CSRC, "mq_w4a16_stream.h")).read()         # the weight-stream walk both W4A16 GEMVs run
COMMON = open(os.path.join(CSRC, "mq_common.h")).read()               # the launch geometry and the LDS opt-in every fat GEMV shares
F16, F32, F64 = np.float16, np.float32, np.float64


def _one(pattern, text=None, where="mq_w4a16.hip"):
    m = re.findall(pattern, SRC if text is None else text)
    assert len(m) == 1, "%r: %d matches in %s" % (pattern, len(m), where)
    return m[0]


def test_the_constants_of_the_mirror_are_the_sources():
    t, w = _one(r"constexpr int WV_THREADS = (\d+), WV_WAVES = (\d+);")
    assert (int(t), int(w)) == (C.WV_THREADS, C.WV_WAVES) and C.WV_THREADS == 64 * C.WV_WAVES
    a, b = _one(r"constexpr size_t WV_MAX_LDS = (\d+) \* (\d+);")
    assert int(a) * int(b) == C.WV_MAX_LDS
    mt, yes, no = _one(r"constexpr int WV_INFLIGHT = MT == (\d+) \? (\d+) : (\d+);")
    assert C.WV_INFLIGHT == {1: int(no), 2: int(no), 4: int(no), int(mt): int(yes)}
    # the walk takes the kernel's count as INFLIGHT: one set of request registers, one issue loop and one consume loop over it
    _one(r"w4_stream_walk<WV_INFLIGHT, false, MT>\(")
    _one(r"template <int INFLIGHT, bool SZ_DWORDS, int MT, class SlotRow, class Stage, class RowDone>", STREAM, "mq_w4a16_stream.h")
    assert len(re.findall(r"\bbuf\[INFLIGHT\]", STREAM)) == 1 and len(re.findall(r"u < INFLIGHT", STREAM)) == 2
    # the LDS opt-in: above LDS_ATTR_ABOVE bytes, once, for the kernel's maximum
    assert int(_one(r"if \(lds > (\d+) && cache\[dev\]", COMMON, "mq_common.h")) == C.LDS_ATTR_ABOVE
    _one(r"hipFuncSetAttribute\(fn, hipFuncAttributeMaxDynamicSharedMemorySize, \(int\)ceiling\)", COMMON, "mq_common.h")
    assert _one(r"set_lds\(fn, lds_set\[ki\], lds, \"mq_w4a16_linear\", (\w+)\)") == "WV_MAX_LDS"
    # the launch geometry: rows over the CUs, capped at one bias per lane of a wave
    assert int(_one(r"fat_row_geometry\(a\.g\.N, WV_WAVES \* (\d+), &rows_per_wg, &grid\);")) == C.WV_MAX_SLOTS == 64
    _one(r"int rpw = \(rows \+ cus - 1\) / cus;", COMMON, "mq_common.h")
    _one(r"if \(rpw > max_rows_per_wg\) rpw = max_rows_per_wg;", COMMON, "mq_common.h")
    _one(r"\*grid = \(unsigned\)\(\(rows \+ rpw - 1\) / rpw\);", COMMON, "mq_common.h")
    _one(r"const size_t lds = \(size_t\)a\.M \* a\.g\.K \* 2;")
    _one(r"const int cpl = \(kchunks \+ 63\) >> 6;", STREAM, "mq_w4a16_stream.h")
    _one(r"const int ki = a\.M == 1 \? 0 : a\.M == 2 \? 1 : a\.M <= 4 \? 2 : 3;")
    _one(r"return \(M <= 8 && \(size_t\)M \* K \* 2 <= WV_MAX_LDS\) \? 1 : 2;")
    bm, bn, bk = _one(r"constexpr int GM_BM = (\d+), GM_BN = (\d+), GM_BK = (\d+),")
    assert (int(bm), int(bn), int(bk)) == (C.GM_BM, C.GM_BN, C.GM_BK)
    _one(r"const int nt = a\.g\.N > GM_BN \? 2 : 1;")


# what each tag of a case's `reaches` says about plan()
REACHES = {
    "slots2": lambda p: p["variant"] == 1 and p["nslots_max"] >= 2,
    "slots3": lambda p: p["variant"] == 1 and p["nslots_max"] >= 3,
    "ragged_slots": lambda p: 1 <= p["nslots_min"] < p["nslots_max"],                       # waves with one slot more than others
    "short_last_wg": lambda p: 0 < p["last_wg_rows"] < p["rows_per_wg"] and p["grid"] >= 2,
    "cpl2": lambda p: p["cpl"] == 2,
    "cpl3": lambda p: p["cpl"] == 3,
    "cpl9": lambda p: p["cpl"] == 9 and p["cpl"] > p["inflight"],
    "cpl32": lambda p: p["cpl"] == 32,
    "clamped": lambda p: p["cpl"] >= 2 and p["clamped_lanes"] > 0,
    "clamped62": lambda p: p["cpl"] >= 2 and p["clamped_lanes"] == 62,
    "passes2": lambda p: p["passes"] >= 2,
    "midrow_refill": lambda p: p["midrow_refill"],
    "inflight_exact": lambda p: p["nslots_max"] * p["cpl"] == p["inflight"] and p["passes"] == 1,
    "lds_attr": lambda p: p["lds_attr"],
    "lds_first": lambda p: p["lds_attr"] and p["lds"] - 128 * p["M"] <= C.LDS_ATTR_ABOVE,   # K steps by 64: the first size above
    "lds_max": lambda p: p["variant"] == 1 and p["lds"] == C.WV_MAX_LDS,
    "gemm_small_m": lambda p: p["variant"] == 2 and p["M"] <= 8 and p["M"] * (p["K"] - 64) * 2 <= C.WV_MAX_LDS,   # just past the seam
    "ktail": lambda p: p["variant"] == 2 and p["ktail"] == 64,
    "cap": lambda p: p["rows_per_wg"] == 1024 and p["grid"] == p["cus"] + 1 and p["nslots_max"] == p["nslots_min"] == 64 and p["last_wg_rows"] == 16,
    "group_div": lambda p: p["group_div"],
    "group_splits_chunk": lambda p: p["variant"] == 2 and p["group_splits_chunk"],
    "group_wide": lambda p: p["variant"] == 2 and p["group_wide"],
    "mt2": lambda p: p["MT"] == 2 and not p["m_guard"],
    "mt4": lambda p: p["MT"] == 4 and not p["m_guard"],
    "mt8": lambda p: p["MT"] == 8,
    "m_guard": lambda p: p["MT"] == 8 and p["m_guard"],
    "zlim": lambda p: p["variant"] in (1, 2),                                               # (the zeros: test_exact_cases_... below)
}


@pytest.mark.parametrize("cus", C.CU_COUNTS)
def test_every_case_reaches_its_branch(cus):
    cases = C.exact_cases(cus)
    assert len({c.id for c in cases}) == len(cases)
    hit = {1: set(), 2: set()}
    for c in cases:
        p = C.plan(c.M, c.N, c.K, c.g, cus)
        assert p["variant"] in (1, 2), c.id
        assert c.reaches, c.id
        for tag in c.reaches:
            assert REACHES[tag](p), "%s at %d CUs does not reach %r: %r" % (c.id, cus, tag, p)
        for tag, holds in REACHES.items():
            try:
                if holds(p):
                    hit[p["variant"]].add(tag)
            except KeyError:                                                                  # a field of the other kernel
                pass
        if p["variant"] == 1:                                                                 # the launch stays inside the kernel's limits
            assert p["lds"] <= C.WV_MAX_LDS and p["nslots_max"] <= C.WV_MAX_SLOTS and p["grid"] * p["rows_per_wg"] >= c.N
        assert c.N * c.K // 2 <= 11 << 20, c.id                                               # packed weights: 8.4 MB at 256 CUs at the most
    gemv = {t for t in REACHES if t not in ("gemm_small_m", "ktail", "group_splits_chunk", "group_wide")}
    assert hit[1] >= gemv, "GEMV branch classes no case reaches at %d CUs: %s" % (cus, sorted(gemv - hit[1]))
    gemm = {"gemm_small_m", "ktail", "group_splits_chunk", "group_wide", "group_div", "zlim"}
    assert hit[2] >= gemm, "GEMM branch classes no case reaches at %d CUs: %s" % (cus, sorted(gemm - hit[2]))
    # both kernels, every MT instantiation, both NT instantiations
    plans = [C.plan(c.M, c.N, c.K, c.g, cus) for c in cases]
    assert {p["MT"] for p in plans if p["variant"] == 1} == {1, 2, 4, 8} and {p["NT"] for p in plans if p["variant"] == 2} == {1, 2}
    for M, N, K, g in C.tolerance_shapes(cus):
        assert C.plan(M, N, K, g, cus)["variant"] in (1, 2)


def test_plan_variant_is_the_entrys_rule():
    from mobilequant_amd import _lib
    lib = _lib.load()

    def both(M, N, K, g):
        g = K if g == -1 else g
        return C.plan(M, N, K, g, 256)["variant"], int(lib.mq_w4a16_supported(M, N, K, g))

    for cus in C.CU_COUNTS:
        for c in C.exact_cases(cus):
            mine, theirs = both(c.M, c.N, c.K, c.g)
            assert mine == theirs, (c.id, mine, theirs)
        for shape in C.tolerance_shapes(cus):
            mine, theirs = both(*shape)
            assert mine == theirs, shape
    # both sides of the seam M * K * 2 <= WV_MAX_LDS, at every M the GEMV serves and at M = 9
    seen = set()
    for M in range(1, 10):
        kmax = C.WV_MAX_LDS // (2 * M) // 64 * 64
        for K in (kmax - 64, kmax, kmax + 64):
            mine, theirs = both(M, 48, K, 64)
            assert mine == theirs == (1 if M <= 8 and M * K * 2 <= C.WV_MAX_LDS else 2), (M, K, mine, theirs)
            seen.add((M, M * K * 2 - C.WV_MAX_LDS))
    assert {(8, -128 * 8), (8, 0), (8, 128 * 8), (1, -128), (1, 0), (1, 128)} <= seen
    for K in (C.WV_MAX_LDS // 16 - 64, C.WV_MAX_LDS // 16, C.WV_MAX_LDS // 16 + 64):
        assert both(9, 48, K, 64) == (2, 2)
    # unserved shapes are 0 on both sides
    for M, N, K, g in ((1, 24, 128, 64), (1, 48, 96, 32), (1, 48, 192, 128), (1, 48, 128, 48), (0, 48, 128, 64)):
        assert both(M, N, K, g) == (0, 0)


@pytest.mark.parametrize("i", range(len(C.exact_cases(256))), ids=[c.id for c in C.exact_cases(256)])
def test_exact_cases_are_independent_of_the_summation_order(i):
    """build_exact asserts max(sum |x16 w16| + |bias|) / 2^emin < 2^24 from the oracle's output; here it runs for the 256-CU table."""
    c = C.exact_cases(256)[i]
    b = C.build_exact(c)
    print("%s: %.1f bits" % (c.id, b.bits_needed))
    assert b.bits_needed < 24 and len(np.unique(b.u)) == 16
    assert np.all(np.log2(b.s16.astype(F64)) == np.rint(np.log2(b.s16.astype(F64)))) and b.s16.astype(F64).min() >= 2.0 ** b.emin
    assert np.all(b.bias.astype(F64) / 2.0 ** b.emin == np.rint(b.bias.astype(F64) / 2.0 ** b.emin))
    assert len(np.unique(b.bias)) == c.N and np.all(b.bias[16:] != b.bias[:-16])
    assert np.all(b.x == np.rint(b.x)) and np.abs(b.x).max() <= 4
    if c.zeros is not None:
        assert set(np.unique(b.z16.astype(F64))) == set(float(z) for z in C.ZLIM) and np.abs(b.z16.astype(F64)).max() == 1024
        d = R.unpack(b.packed).astype(F64).reshape(c.N, -1, 64) - b.z16.astype(F64)[:, :, None]
        assert d.max() == 1039 and d.min() == -1024                                           # u - z' needs all 11 significand bits
    if c.id == "cap":
        assert np.all(b.bias[1024:] != b.bias[:-1024])


def test_the_small_cu_tables_are_exact_too():
    """The shapes that change with the CU count, at 64 CUs (the cheapest): the same assertion."""
    for c in C.exact_cases(64):
        if c.N != dict((d.id, d.N) for d in C.exact_cases(256))[c.id]:
            assert C.build_exact(c).bits_needed < 24, c.id


def test_fp16_edge_columns_are_what_they_claim():
    for M in (2, 17):
        e = C.build_edges(M)
        w = e.want.astype(F64)[0]
        assert np.array_equal(e.want, np.broadcast_to(e.want[0], e.want.shape))
        assert w[0] == 65504 and w[1] == 65504 and w[2] == np.inf and w[3] == -np.inf and w[4] == -65504 and w[5] == -65504
        assert list(w[6:11] * 2.0 ** 24) == [1, 3, 1023, 1024, -5]                           # subnormals and the first normal
        assert list(w[11:] * 2.0 ** 24) == [0, 2, 0, -2, 2] and np.signbit(e.want[0, 13])   # ties to even: 2^-25 -> 0, 3 2^-25 -> 2^-23
        assert e.y64[0, 1] == 65520 - 2.0 ** -8 and float(F32(e.y64[0, 1])) == e.y64[0, 1]


def _slow(packed, s16, z16, g, x, bias):
    """w16 and y element by element: Python floats (float64), the group by integer division, the nibble from the packed byte."""
    N, K = packed.shape[0], packed.shape[1] * 2
    w = np.zeros((N, K), F16)
    for n in range(N):
        for k in range(K):
            kb, r = divmod(k, 32)
            byte = int(packed[n, 16 * kb + r % 16])                     # byte j of the 16-byte group: element j low, element j + 16 high
            nib = byte >> 4 if r >= 16 else byte & 15
            G = k // g
            w[n, k] = F16(float(s16[n, G]) * (nib - float(z16[n, G])))  # the product is exact in float64: one rounding
    x16 = x.astype(F16)
    y = np.zeros((x.shape[0], N), F64)
    for m in range(x.shape[0]):
        for n in range(N):
            acc = 0.0
            for k in range(K):
                acc += float(x16[m, k]) * float(w[n, k])
            y[m, n] = acc + float(bias[n])
    return w, y


@pytest.mark.parametrize("id", ["gdiv-m3-k192", "gdiv-m17-k320"])
def test_the_oracle_equals_a_slow_scalar_evaluation(id):
    c = next(c for c in C.exact_cases(256) if c.id == id)
    b = C.build_exact(c)
    gs, _ = R.groups(c.K, c.g)
    assert (gs // 32) & (gs // 32 - 1)                                   # a division-group shape
    w, y = _slow(b.packed, b.s16, b.z16, gs, b.x, b.bias)
    assert np.array_equal(w.view(np.uint16), R.w16(b.u, b.s16, b.z16, c.g).view(np.uint16)) and np.array_equal(w.view(np.uint16), b.w16.view(np.uint16))
    y64, _ = R.linear64(b.x, b.w16, b.bias)
    assert np.array_equal(y.view(np.uint64), y64.view(np.uint64))
    assert np.array_equal(C.want_f32(b, b.x, b.bias).astype(F64), y)
