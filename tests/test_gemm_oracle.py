"""CPU: the oracle of the prefill GEMM epilogues (oracle.fma_f32, prefill_gemm_acc, prefill_gemm_epilogue, prefill_gemm_gated) and the
case lists of gemm_cases.py, held to what test_gpu_gemm_epilogue.py relies on -- without a GPU.

  * fma_f32 against exact rational arithmetic, on random triples and on constructed ones whose float64 sum lies exactly on an fp32
    midpoint with a residual of either sign (where float32(a64 * b64 + c64) rounds twice and is wrong);
  * the epilogue oracle against the existing ones: bit for bit qlinear_int_exact without a grid, within one index of the division
    form quantize_index with one;
  * every case: ties of both parities, both clamps, the steps around them, accumulators beyond 2^24 whose conversion rounds, no wrap;
  * the dispatch predicates reach every kernel with every grid class it accepts; the tile map is a bijection on every grid the cases
    launch, block counts that are no multiple of 8 and a short last group included."""
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gemm_cases as C  # noqa: E402
from oracle import mq_oracle as O  # noqa: E402
from test_gpu_parity import _int_problem  # noqa: E402

F32 = np.float32


def _round_f32_exact(x: Fraction) -> float:
    """The fp32 nearest to the rational x, ties to even (normal range), by integer arithmetic alone."""
    if x == 0:
        return 0.0
    s, x = (-1 if x < 0 else 1), abs(x)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1                                                      # 2^e <= x < 2^(e + 1)
    assert -126 <= e <= 127
    m = x / Fraction(2) ** (e - 23)                                 # in [2^23, 2^24)
    fl = m.numerator // m.denominator
    rem = m - fl
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and fl & 1):
        fl += 1
    return s * float(fl) * 2.0 ** (e - 23)


def _exact_fma(a, b, c):
    return np.array([_round_f32_exact(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)], F32)


def _midpoint_triples():
    """(a, b, c) with a * b + c = (the midpoint of the fp32 neighbours m 2^e and (m + 1) 2^e) -+ 2^(e - 47): the product is
    +-(1 + 2^-23)(1 - 2^-23) 2^(e - 1) = +-(1 - 2^-46) 2^(e - 1), half an ulp of c short of 2^-46 of itself, 70 bits below the sum's
    leading bit, so the float64 sum IS the midpoint.  c = m 2^e with the product added lands just below it (the result is m whatever
    its parity), c = (m + 1) 2^e with the product subtracted just above (the result is m + 1); mirrored for negative sums."""
    a, b, c = [], [], []
    for m in (2 ** 23 + 1, 2 ** 23 + 2, 2 ** 24 - 3, 2 ** 24 - 2, 12345677, 12345678):
        for sign in (1, -1):
            for e in (0, 5, -7):
                for above in (False, True):
                    a.append(sign * (-1 if above else 1) * (1.0 + 2.0 ** -23))
                    b.append((1.0 - 2.0 ** -23) * 2.0 ** (e - 1))
                    c.append(sign * (m + 1 if above else m) * 2.0 ** e)
    return np.array(a, F32), np.array(b, F32), np.array(c, F32)


def test_fma_f32_random_triples_against_rationals():
    rng = np.random.default_rng(11)
    n = 4000
    a = (rng.standard_normal(n) * 2.0 ** rng.integers(-10, 26, n)).astype(F32)
    b = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 4, n)).astype(F32)
    c = (rng.standard_normal(n) * 2.0 ** rng.integers(-10, 20, n)).astype(F32)
    c[::5] = (-(a[::5].astype(np.float64) * b[::5].astype(np.float64))).astype(F32)      # cancellation: the residual of the product is the result
    t = rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32).astype(F32)                  # converted accumulators
    for x, y, z in ((a, b, c), (t, b, c)):
        got, want = O.fma_f32(x, y, z), _exact_fma(x, y, z)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.flatnonzero(got != want)[:5]


def test_fma_f32_midpoints_where_double_rounding_is_wrong():
    a, b, c = _midpoint_triples()
    a64, b64, c64 = (v.astype(np.float64) for v in (a, b, c))
    s = a64 * b64 + c64
    want = _exact_fma(a, b, c)
    naive = s.astype(F32)
    other = np.nextafter(naive, np.where(s > naive, F32(np.inf), F32(-np.inf)).astype(F32))
    on_midpoint = (s != naive) & (s == (naive.astype(np.float64) + other.astype(np.float64)) / 2)
    assert on_midpoint.all(), "every constructed sum has to land on an fp32 midpoint in float64"
    wrong = naive != want
    assert wrong.sum() >= len(a) // 4, "float32(a64 * b64 + c64) has to be wrong on a good part of the set (%d of %d)" % (wrong.sum(), len(a))
    # the residual's sign: both have to occur among the triples the naive expression gets wrong
    signs = np.array([(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z)) > Fraction(float(v))) for x, y, z, v in zip(a, b, c, s)])
    assert signs[wrong].any() and (~signs[wrong]).any()
    got = O.fma_f32(a, b, c)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.flatnonzero(got != want)[:5]


@pytest.mark.parametrize("shape", [(16, 64, 128), (100, 180, 256), (257, 260, 384)])
@pytest.mark.parametrize("per_row", [False, True])
def test_epilogue_without_grid_is_qlinear_int_exact(shape, per_row):
    M, N, K = shape
    rng = np.random.default_rng(M * 7 + N)
    qa, qw, za, zw, sa, sw, bias = _int_problem(rng, M, N, K, per_row)
    _, want = O.qlinear_int_exact(qa, za, sa, qw, zw, sw, bias)
    a8, w8 = qa - 128, qw - 128                                     # storage with shift 128 on both sides, as _run_int8 passes it
    alpha, w_zp, ct = O.linear_epilogue_vectors(np.array([sa], F32), np.array([za], F32), 128, np.asarray(sw, F32), np.asarray(zw, F32), 128,
                                                w8.sum(axis=1), K)
    t = O.prefill_gemm_acc(a8, w8, a8.sum(axis=1), w_zp, ct)
    got, _, _ = O.prefill_gemm_epilogue(t, alpha, bias)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    half, _, _ = O.prefill_gemm_epilogue(t, alpha, bias, out_dtype="f16")
    assert np.array_equal(half.view(np.uint16), want.astype(np.float16).view(np.uint16))


@pytest.mark.parametrize("grid", ["u8", "s8", "u4", "u16", "i16"])
def test_epilogue_with_grid_is_within_one_index_of_the_division_form(grid):
    g = C.GRIDS[grid]
    rng = np.random.default_rng(5)
    qa, qw, za, zw, sa, sw, bias = _int_problem(rng, 100, 180, 256, True)
    acc, y = O.qlinear_int_exact(qa, za, sa, qw, zw, sw, bias)
    lo, hi = float(y.min()), float(y.max())
    scale = F32(0.9 * (hi - lo) / (g.qmax - g.qmin))                # the outputs span the grid and a little more: both clamps
    off = F32(round((g.qmin + g.qmax) / 2 - (lo + hi) / 2 / float(scale)))
    alpha = (F32(sa) * np.asarray(sw, F32)).astype(F32)
    stored, _, _ = O.prefill_gemm_epilogue(acc.astype(np.int32), alpha, bias, [(scale, off)], None, g.qmin, g.qmax, g.storage)
    want = O.quantize_index(y, scale, off, g.qmin, g.qmax).astype(np.int64)
    idx = stored.astype(np.int64)
    if grid == "u16":
        idx &= 0xFFFF
    assert np.abs(idx - want).max() <= 1
    assert (idx == want).mean() > 0.99 and idx.min() == g.qmin and idx.max() == g.qmax
    deq, _, _ = O.prefill_gemm_epilogue(acc.astype(np.int32), alpha, bias, [(scale, off)], None, g.qmin, g.qmax, "f32")
    assert np.array_equal(deq, O.dequantize_index(idx.astype(F32), scale, off))


def test_gated_oracle_is_the_table_and_the_layout_formula():
    rng = np.random.default_rng(3)
    ia, ib = rng.integers(0, 256, (37, 128)), rng.integers(0, 256, (37, 128))
    tb = C.gate_table()
    img, (image, real), rs = O.prefill_gemm_gated(ia, ib, tb)
    assert img[7, 9] == tb[ia[7, 9] * 256 + ib[7, 9]] and image[O.tiled_offset(7, 9, 128)] == img[7, 9]
    assert real.sum() == 37 * 128 and image.size == 48 * 128 and np.array_equal(rs, img.astype(np.int64).sum(axis=1))


# ---- the case lists -------------------------------------------------------------------------------------------------------------
def test_case_ids_are_unique_and_operands_respect_the_entry_points():
    assert len({c.id for c in C.ALL_CASES}) == len(C.ALL_CASES)
    for c in C.ALL_CASES:
        assert c.N % 4 == 0 and c.K % 128 == 0 and c.M > 8, c.id
        if c.segs:
            assert c.segs[-1] == c.N and all(s % 4 == 0 for s in c.segs) and c.grid in C.U8_FAST, c.id
        if not c.rowsum:
            assert not C.weights(c.N, c.K, c.w4, False, C._span(c), 0)[1].any(), c.id


def test_segment_ends_cover_unaligned_and_aligned_and_every_count():
    ends = [c.segs for c in C.ALL_CASES if c.segs]
    assert {len(s) for s in ends} == {1, 2, 3}
    inner = [e for s in ends for e in s[:-1]]
    assert any(all(e % b for b in (16, 128, 160, 176)) for e in inner), "an end off every tile and fragment boundary"
    assert any(e % 128 == 0 for e in inner), "a tile-aligned neighbour"
    for k in ("fr128", "fr160", "frw4x128"):                        # the per-column-grid kernels: both kinds arrive
        mine = [c.segs for c in C.ALL_CASES if c.segs and len(c.segs) > 1 and C.kernels_of(c)[0][0] == k]
        assert any(all(e % 16 for e in s[:-1]) for s in mine), k


@pytest.mark.parametrize("c", C.ALL_CASES, ids=lambda c: c.id)
def test_case_conditions(c):
    """What the GPU comparison relies on, from the oracle alone; the gated and pair cases for both of their linears."""
    g = C.GRIDS[c.grid]
    for which in range(2 if c.entry in ("pair", "gated") else 1):
        d = C.conditions(c, which)
        assert d["wraps"] == 0 and d["tmax"] < 2 ** 31, d
        assert d["big"] >= 64 and d["big_rounds"] >= 64, d          # |t| > 2^24, and the conversion to fp32 is inexact
        if g is None:
            continue
        assert d["tie_even"] >= 64 and d["tie_odd"] >= 64, d
        if c.bias:
            assert d["near_tie"] >= 8, d                            # B' moved by an ulp or two: just off a tie
        need = math.ceil(0.01 * c.M)
        assert d["sat_lo_min"] >= need and d["sat_hi_min"] >= need, d
        for k in C.SAT_STEPS:
            assert d[k] >= 1, (k, d)


def _mutant(c, kind):
    """A subtly wrong epilogue for the index / dequantised outputs of case c: the oracle's steps with ONE of them replaced."""
    p, g = C.problem(c), C.GRIDS[c.grid]
    N = c.N
    fold = g.qmax - g.qmin <= 255
    sc, oo = O.prefill_gemm_columns(N, p.grids, p.seg_end)
    tf = p.t.astype(F32)
    if kind == "cvt_truncates":                                     # int32 -> fp32 toward zero
        t64 = p.t.astype(np.int64)
        over = tf.astype(np.int64)
        tf = np.where(np.abs(over) > np.abs(t64), np.nextafter(tf, F32(0)), tf).astype(F32)
    inv = (F32(1.0) / sc).astype(F32)
    bs = np.zeros(N, F32) if p.bias is None else p.bias
    a1 = (p.alpha / sc).astype(F32) if kind == "division_form" else (p.alpha * inv).astype(F32)
    b1 = (bs * inv).astype(F32)
    if fold:
        b1 = (b1 + oo).astype(F32)
    if kind == "mul_then_add":
        q = ((tf * a1[None, :]).astype(F32) + b1[None, :]).astype(F32)
    else:
        q = O.fma_f32(tf, np.broadcast_to(a1, tf.shape), np.broadcast_to(b1, tf.shape))
    if kind == "offset_before_rint" and not fold:
        r = np.rint((q + oo[None, :]).astype(F32)).astype(F32)
    else:
        r = np.floor(q.astype(np.float64) + 0.5).astype(F32) if kind == "half_up" else np.rint(q).astype(F32)
        if not fold:
            r = (r + oo[None, :]).astype(F32)
    lo = F32(g.qmin + (kind == "low_clamp_off_by_one"))
    hi = F32(g.qmax - (kind == "high_clamp_off_by_one"))
    return np.minimum(np.maximum(r, lo), hi).astype(np.int64)


MUTANTS = ("half_up", "mul_then_add", "cvt_truncates", "division_form", "offset_before_rint", "low_clamp_off_by_one", "high_clamp_off_by_one")


@pytest.mark.parametrize("c", [c for c in C.ALL_CASES if c.M <= 400 and C.GRIDS[c.grid] is not None], ids=lambda c: c.id)
def test_cases_tell_the_oracle_from_subtly_wrong_epilogues(c):
    """Every small case with a grid separates the oracle from: ties rounded half up, a multiply and an add for the fma, a truncating
    int -> float conversion, alpha / scale for alpha * fl(1 / scale) (scales that are no power of two), the offset of a 16-bit grid added
    in front of the rounding, and either clamp off by one.  The unmutated restatement is the oracle itself."""
    g = C.GRIDS[c.grid]
    e = C.expect(c)
    _, oo = O.prefill_gemm_columns(c.N, C.problem(c).grids, C.problem(c).seg_end)
    fold = g.qmax - g.qmin <= 255
    want = np.minimum(np.maximum(np.rint(e.q) + (0 if fold else oo.astype(np.float64)[None, :]), g.qmin), g.qmax).astype(np.int64)
    assert np.array_equal(_mutant(c, "none"), want)
    for kind in MUTANTS:
        if (kind == "offset_before_rint" and fold) or (kind == "division_form" and c.p2):
            continue
        # without a bias B' is the bare offset: nothing cancels the big columns' t A' (they clamp), where an ulp of A' or of
        # float(t) is worth an index; a multiply and an add then differ from the fma by one rounding at 2^-17 of an index
        if kind in ("mul_then_add", "cvt_truncates", "division_form") and not c.bias:
            continue
        assert (_mutant(c, kind) != want).sum() >= 1, kind


def test_zero_points_hold_both_extremes_and_stay_in_the_24_bit_multiply():
    for c in C.ALL_CASES:
        if not c.rowsum or c.M > 400:
            continue
        p = C.problem(c)
        assert p.w_zp.max() == 255 and p.w_zp.min() == -255, c.id
        assert np.abs(p.a_rowsum).max() < 2 ** 23
        assert p.a.min() == -128 and p.a.max() == 127 and not p.a[C.ZERO_ROW].any()
        if c.w4:
            assert p.w.min() == 0 and p.w.max() == 15
        else:
            assert p.w.min() == -128 and p.w.max() == 127


def test_every_kernel_is_reached_with_every_grid_class_it_accepts():
    reached = {}
    for c in C.ALL_CASES:
        ks = C.kernels_of(c)
        assert all(k is not None for k, _ in ks), "%s: the entry point would answer MQ_EUNSUPPORTED" % c.id
        for k, _ in ks:
            reached.setdefault(k, set()).add(c.grid)
    for k, grids in C.REACH.items():
        assert k in reached, "no case reaches %s" % k
        assert grids <= reached[k], "%s is not reached with %s" % (k, sorted(grids - reached[k]))
    want = {"cpp_v%d" % v for v in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10)} | {
        "fr", "fr_pair", "fr_pair_persistent", "fr128", "fr160", "fr128r", "fr128r8", "frg176", "frg128", "frw4x176", "frw4x128", "frw4r",
        "frgw4x176", "frgw4x128"}
    assert want == set(C.REACH) and want <= set(reached)
    # packed weights reach the C++ kernel too, and the entry points beside mq_w8a8_linear are all present
    assert any(c.w4 and C.kernels_of(c)[0][0].startswith("cpp_") for c in C.ALL_CASES)
    assert {c.entry for c in C.ALL_CASES} == {"linear", "linear_residual", "segmented", "tiled", "tiled_w4", "tiled_segmented", "tiled_residual",
                                              "pair", "gated"}
    assert {(c.entry, c.w4) for c in C.ALL_CASES} >= {("segmented", True), ("segmented", False), ("tiled_residual", True), ("gated", True)}


def test_pick_variant_by_shape_is_exercised():
    """Unforced row-major cases take the variant pick_variant names; the restated thresholds at their edges."""
    assert C.pick_variant(2048, 5632, False) == 7 and C.pick_variant(2048, 5632, True) == 10
    assert C.pick_variant(300, 260, False) == 8 and C.pick_variant(2048, 2560, False) == 5 and C.pick_variant(4096, 16384, True) == 2
    assert any(c.variant < 0 and c.entry in ("linear", "linear_residual", "segmented") for c in C.ALL_CASES)


def test_tile_map_is_a_bijection_on_every_launched_grid():
    grids = set()
    for c in C.ALL_CASES:
        for _, (bm, bn) in C.kernels_of(c):
            grids.add((-(-c.M // bm), -(-c.N // bn)))
    short_group = not_mult_8 = False
    for gm, gn in sorted(grids):
        nblk = gm * gn
        tiles = [C.tile_of_block(b, nblk, gm, gn) for b in range(nblk)]
        assert sorted(tiles) == [(m, n) for m in range(gm) for n in range(gn)], (gm, gn)
        not_mult_8 |= nblk % 8 != 0
        short_group |= gm % 4 != 0 and gm > 4
    assert not_mult_8 and short_group and (3, 3) in grids and (9, 22) in grids and (8, 24) in grids
