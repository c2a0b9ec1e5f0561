"""GPU: the calibration statistics of csrc/mq_reduce.hip -- mq_minmax_tensor (running), mq_minmax_tensor_fresh, mq_minmax_rows, mq_minmax_cols
and the fused passes mq_calib_attention_probs(_causal), mq_calib_norm, mq_calib_gated, mq_calib_rope(_qkv) -- against plain numpy oracles at
every dispatch branch and on every grid-stride trip.  No sibling kernel and no torch GPU op is a reference.

Bars.  Min/max of inputs (all four entry points, fp32 and fp16; the raw-score, h, delta, a, b, q / k / v-linear statistics), h, the RoPE
outputs, repeat_kv and the rotated statistics: EXACT (zeros compare with ==, NaN is a NaN).  Statistics of tensors a kernel writes
(probabilities, y, product, act(a)): exactly numpy's min / max of the bytes it wrote, and within the value bar of the float64 extremes.
y: bit for bit under the replay search (oracle.calib_norm_replay: some fp32 (mu, r) within gamma_n of the float64 row statistic reproduces
the whole row through the kernel's own expression), every element inside oracle.calib_norm_rows' err.  Probabilities: float64 softmax of
the op-for-op fp32 x (oracle.calib_probs).
  PROBS_ULP / PROBS_ABS: the project's bar was 8 ulp and 1.2e-7 against torch's GPU softmax (test_gpu_round5.py), which shares the fp32
  rounding of x - max and a row sum of the same length with the kernel.  Against float64 neither cancels: fl(x - max) alone is
  |x - max| 2^-24 relative -- 13 ulp at x - max = -27 -- and the sum of up to 4096 terms moves every entry of a row by the same few
  ulp, 6e-8 each for the entries above 1/2.  Worst observed over all cases of this file on an MI355X: 18.77 ulp and 2.50e-7 absolute;
  the bars are restated at twice that (the project's rule, tools/observe_bars.py): 38 ulp and 5.0e-7.
Product: rtol 2e-6 / atol 1e-7 against float64 -- unchanged for SiLU.  GELU is the reference's fp32 0.5 a (1 + erf(a / sqrt 2)): for
a < 0 the sum 1 + erf cancels and erff's ABSOLUTE error (a fraction of an ulp of 1) enters the product at full size, 0.5 |a b| E -- the
float64 value needs that third term (the torch fp32 chain the bar was set against has the same cancellation).  Worst observed
E = 2.26e-8 (0.38 ulp of 1); GELU_ERF_ABS is twice that.  With the term, the worst product deviation is 0.09 of the bar.
act(a) extremes: 1e-6 max(1, |min|) / 2e-6 |max| (unchanged; worst observed 0.026 of it).

Every call goes through ops._lib.call on buffers this file allocates: 64 canary bytes in front of and behind every output and every
statistic slot (pointer offsets included), and they have to survive.  Every case comes from calib_cases.py, whose lists
test_calib_oracle.py holds to the launch code on the CPU.  A failure names the entry point, the case, the first differing (row, column),
got, want and the input's bit pattern.

Measured wall time of the whole file on an MI355X: 8.5 s for its 329 tests (the slowest, the causal chain at S = 2052 x 7 blocks --
118 MB, six runs, one float64 softmax --, 2.1 s; S = 1028 x 16 1.1 s; everything else under 0.3 s)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import calib_cases as C  # noqa: E402
from gpu_buffers import CB, PAD, Buf, Slots, _bits, check_bits, same  # noqa: E402,F401
from oracle import mq_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F16 = np.float32, np.float16
MQ = {"f32": 0, "f16": 1}
TORCH = {"f32": torch.float32, "f16": torch.float16}
PROBS_ULP, PROBS_ABS = 38.0, 5.0e-7
PROD_RTOL, PROD_ATOL = 2e-6, 1e-7
GELU_ERF_ABS = 4.6e-8                      # erff's absolute error allowance in 1 + erf: twice the worst observed 2.26e-8
WORST = {"ulp": 0.0, "abs": 0.0, "prod": 0.0, "act": 0.0, "erf": 0.0}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    import mobilequant_amd._lib as L
    assert L.device_info()["arch"].startswith("gfx950")
    yield torch.device("cuda:0")
    print("\ntest_gpu_calib worst observed: %r" % (WORST,))


def _call(name, *args):
    from mobilequant_amd import ops
    ops._lib.call(name, *args)
    torch.cuda.synchronize()


def _refused(status, name, *args):
    from mobilequant_amd import ops
    with pytest.raises(ops._lib.MobileQuantLibraryError, match=r"status %d" % status):
        ops._lib.call(name, *args)
    torch.cuda.synchronize()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _inp(dev, a, off_bytes=0):
    return Buf(dev, a.nbytes, off_bytes, a)


def minmax_slots(dev, pairs=1):
    """`pairs` (min, max) slot pairs at the identity +inf / -inf: slot 2 i is a minimum, 2 i + 1 its maximum."""
    return Slots(dev, 2 * pairs, np.tile(np.array([np.inf, -np.inf], F32), pairs))


def check_stat(got, want, what):
    got, want = np.atleast_1d(got), np.atleast_1d(np.asarray(want, F32))
    bad = np.flatnonzero(~same(got, want))
    if len(bad):
        i = int(bad[0])
        pytest.fail("%s: statistic %d of %d differs: got %r (%s) want %r (%s)" % (what, i, got.size, float(got[i]), _bits(F32(got[i])), float(want[i]), _bits(want[i])))


def np_min(x, axis=None):
    return np.min(np.asarray(x, F32) if x.dtype != F32 else x, axis=axis)       # np.min / np.max propagate NaN


def np_max(x, axis=None):
    return np.max(np.asarray(x, F32) if x.dtype != F32 else x, axis=axis)


# ---- per-tensor ---------------------------------------------------------------------------------------------------------------------------
def run_tensor(dev, entry, xb, dtype, numel, slots, i, scratch):
    if entry == "running":
        _call("mq_minmax_tensor", xb.ptr if numel else None, MQ[dtype], numel, slots.ptr(2 * i), slots.ptr(2 * i + 1), _stream())
    else:
        _call("mq_minmax_tensor_fresh", xb.ptr, MQ[dtype], numel, slots.ptr(2 * i), slots.ptr(2 * i + 1), scratch.ptr, 1024, _stream())


@pytest.mark.parametrize("size_i", range(12))
@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("entry", ["running", "fresh"])
def test_minmax_tensor_planted_extremes(dev, entry, dtype, size_i):
    """mq_minmax_tensor (atomic commit behind the relaxed filter: the kernel calibration uses) and mq_minmax_tensor_fresh (partials + fold)
    at every size class and every start offset, the unique maximum and minimum planted in turn at every head scalar, the ends of the first
    and last vector, every tail scalar and either side of the first three grid-stride boundaries.  The fresh path has to WRITE its slots
    (they start at 7)."""
    numel = C.tensor_sizes(dtype)[size_i]
    base = C.base_values(numel, dtype, "tensor")
    hi, lo = C.NP[dtype](2), C.NP[dtype](-2)
    for off in C.tensor_offsets(dtype):
        plants = C.tensor_plants(numel, off, dtype)
        xb = _inp(dev, base, off * C.SIZE[dtype])
        xv = xb.dev_view(TORCH[dtype])
        slots = minmax_slots(dev, len(plants)) if entry == "running" else Slots(dev, 2 * len(plants), F32(7))
        scratch = Buf(dev, 1024 * 4)
        for i, (pmax, pmin) in enumerate(plants):
            xv[pmin] = float(lo)
            xv[pmax] = float(hi)
            run_tensor(dev, entry, xb, dtype, numel, slots, i, scratch)
            xv[pmin] = float(base[pmin])
            xv[pmax] = float(base[pmax])
        got = slots.take("%s %s numel %d off %d" % (entry, dtype, numel, off)).reshape(-1, 2)
        scratch.take(F32, "scratch")
        assert np.array_equal(xb.take(C.NP[dtype], "x").view(np.uint8), base.view(np.uint8)), "x was written"
        pos = C.tensor_positions(numel, off, dtype)
        for i, (pmax, pmin) in enumerate(plants):
            want = (hi if pmin == pmax else lo, hi)
            if not (got[i, 0] == want[0] and got[i, 1] == want[1]):
                pytest.fail("mq_minmax_tensor%s %s numel %d off %d: maximum at %d (%s), minimum at %d (%s): got [%r, %r] want [%r, %r]; geometry %r"
                            % ("_fresh" if entry == "fresh" else "", dtype, numel, off, pmax, pos[pmax], pmin, pos[pmin], float(got[i, 0]),
                               float(got[i, 1]), float(want[0]), float(want[1]), C.tensor_geom(numel, off, dtype)))


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_minmax_tensor_running_semantics(dev, dtype):
    """Two calls widen the statistic, a third cannot narrow it, an empty tensor leaves it untouched (a fresh one: the identity)."""
    n = 1024 * 4 + 9
    x1 = C.base_values(n, dtype, "run1")
    x2 = (C.base_values(n, dtype, "run2") * C.NP[dtype](3)).astype(C.NP[dtype])
    x3 = (C.base_values(n, dtype, "run3") / C.NP[dtype](2)).astype(C.NP[dtype])
    slots = minmax_slots(dev)
    want = [np.inf, -np.inf]
    for k, x in enumerate((x1, x2, x3, x1[:0])):
        xb = _inp(dev, x, C.SIZE[dtype]) if x.size else None
        _call("mq_minmax_tensor", xb.ptr if xb else None, MQ[dtype], x.size, slots.ptr(0), slots.ptr(1), _stream())
        if x.size:
            want = [min(want[0], float(x.min())), max(want[1], float(x.max()))]
        check_stat(slots.take("running"), want, "mq_minmax_tensor %s call %d" % (dtype, k))
    assert want[0] == float(min(x1.min(), x2.min())) < float(x3.min()) and float(x2.min()) < float(x1.min())
    fresh, scratch = Slots(dev, 2, F32(7)), Buf(dev, 4096)
    _call("mq_minmax_tensor_fresh", None, MQ[dtype], 0, fresh.ptr(0), fresh.ptr(1), scratch.ptr, 1024, _stream())
    check_stat(fresh.take("fresh"), [np.inf, -np.inf], "mq_minmax_tensor_fresh %s empty" % dtype)


# ---- per-row / per-column -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", C.ROWS_CASES, ids=lambda c: c.id)
def test_minmax_rows_planted_extremes(dev, c):
    """minmax_rows_kernel<float | __half>, vector and scalar path (by shape and by pointer): over the launches every lane, the last vector
    and the last scalar hold a row's extreme; the statistics run on from launch to launch."""
    n = len(C.rows_launches(c))
    mn, mx = Buf(dev, 4 * c.rows, fill=F32(np.inf)), Buf(dev, 4 * c.rows, fill=F32(-np.inf))
    wmn, wmx = np.full(c.rows, np.inf, F32), np.full(c.rows, -np.inf, F32)
    for j in range(n):
        x = C.rows_input(c, j)
        xb = _inp(dev, x, c.off * C.SIZE[c.dtype])
        _call("mq_minmax_rows", xb.ptr, MQ[c.dtype], c.rows, c.cols, mn.ptr, mx.ptr, _stream())
        wmn, wmx = np.minimum(wmn, x.min(axis=1).astype(F32)), np.maximum(wmx, x.max(axis=1).astype(F32))
        gmn, gmx = mn.take(F32, "min"), mx.take(F32, "max")
        for name, g, w, k in (("min", gmn, wmn, 1), ("max", gmx, wmx, 0)):
            bad = np.flatnonzero(g != w)
            if len(bad):
                r = int(bad[0])
                col = C.rows_launches(c)[j][r][k]
                pytest.fail("mq_minmax_rows %s launch %d: %s of row %d: got %r want %r; planted at column %d (lane %d), x = %r (%s)"
                            % (c.id, j, name, r, float(g[r]), float(w[r]), col, C.rows_lane(col, c), float(x[r, col]), _bits(x[r, col])))


@pytest.mark.parametrize("c", C.COLS_CASES, ids=lambda c: c.id)
def test_minmax_cols_planted_extremes(dev, c):
    """minmax_cols_kernel<float | __half> and the scalar fallback (by shape and by pointer), one to five row chunks with a ragged last one:
    over two launches every row holds some column's extreme; the statistics run on."""
    mn, mx = Buf(dev, 4 * c.cols, fill=F32(np.inf)), Buf(dev, 4 * c.cols, fill=F32(-np.inf))
    wmn, wmx = np.full(c.cols, np.inf, F32), np.full(c.cols, -np.inf, F32)
    for j in (0, 1):
        x = C.cols_input(c, j)
        xb = _inp(dev, x, c.off * C.SIZE[c.dtype])
        _call("mq_minmax_cols", xb.ptr, MQ[c.dtype], c.rows, c.cols, mn.ptr, mx.ptr, _stream())
        wmn, wmx = np.minimum(wmn, x.min(axis=0).astype(F32)), np.maximum(wmx, x.max(axis=0).astype(F32))
        gmn, gmx = mn.take(F32, "min"), mx.take(F32, "max")
        rows = C.cols_plants(c, j)
        for name, g, w, k in (("min", gmn, wmn, 1), ("max", gmx, wmx, 0)):
            bad = np.flatnonzero(g != w)
            if len(bad):
                col = int(bad[0])
                r = int(rows[k][col])
                pytest.fail("mq_minmax_cols %s launch %d: %s of column %d: got %r want %r; planted in row %d, x = %r (%s); geometry %r"
                            % (c.id, j, name, col, float(g[col]), float(w[col]), r, float(x[r, col]), _bits(x[r, col]),
                               C.cols_geom(c.rows, c.cols, c.off, c.dtype)))


# ---- non-finite values and zeros ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_minmax_nonfinite_and_zeros(dev, dtype):
    """One NaN at each class of position makes exactly that statistic NaN and a later finite, +-inf or +-huge update leaves it NaN (running
    paths); +-inf are ordinary values; zeros of both signs compare equal."""
    dt, n = C.NP[dtype], 1024 * 4 + 9
    off = 1
    pos = C.tensor_positions(n, off, dtype)
    picks = [next(p for p, k in pos.items() if k == cls) for cls in ("head", "vec0_first", "vecN_last", "tail")] + [max(pos)]
    scratch = Buf(dev, 4096)
    for entry in ("running", "fresh"):
        for p in picks:
            x = C.base_values(n, dtype, "nan")
            x[p] = np.nan
            slots = minmax_slots(dev)
            run_tensor(dev, entry, _inp(dev, x, off * C.SIZE[dtype]), dtype, n, slots, 0, scratch)
            check_stat(slots.take("nan"), [np.nan, np.nan], "%s %s NaN at %d (%s)" % (entry, dtype, p, pos[p]))
            if entry == "running":
                for k, u in enumerate(C.later_updates(dtype, 100)):
                    run_tensor(dev, entry, _inp(dev, u), dtype, u.size, slots, 0, scratch)
                    check_stat(slots.take("nan"), [np.nan, np.nan], "running %s update %d after a NaN" % (dtype, k))
        x = C.base_values(n, dtype, "inf")
        x[picks[0]], x[picks[3]] = np.inf, -np.inf
        slots = minmax_slots(dev)
        run_tensor(dev, entry, _inp(dev, x, off * C.SIZE[dtype]), dtype, n, slots, 0, scratch)
        check_stat(slots.take("inf"), [-np.inf, np.inf], "%s %s +-inf" % (entry, dtype))
        slots = minmax_slots(dev)
        run_tensor(dev, entry, _inp(dev, C.zeros_input(n, dtype), off * C.SIZE[dtype]), dtype, n, slots, 0, scratch)
        check_stat(slots.take("zeros"), [0.0, 0.0], "%s %s zeros of both signs" % (entry, dtype))
    # rows: the NaN sits in one lane of one row; cols: in one column, once on the vector and once on the scalar path
    nv = C.VEC[dtype]
    for cols, col in ((64 * nv + nv, 64 * nv + 1), (64 * nv + 3, 64 * nv + 2)):
        rows = 7
        x = C.base_values(rows * cols, dtype, "nanrows", cols).reshape(rows, cols)
        x[3, col], x[5, 0], x[5, 1] = np.nan, np.inf, -np.inf
        mn, mx = Buf(dev, 4 * rows, fill=F32(np.inf)), Buf(dev, 4 * rows, fill=F32(-np.inf))
        _call("mq_minmax_rows", _inp(dev, x).ptr, MQ[dtype], rows, cols, mn.ptr, mx.ptr, _stream())
        for u in (None, np.full((rows, cols), 0.5, dt)):
            if u is not None:
                _call("mq_minmax_rows", _inp(dev, u).ptr, MQ[dtype], rows, cols, mn.ptr, mx.ptr, _stream())
            g0, g1 = mn.take(F32, "min"), mx.take(F32, "max")
            assert np.isnan(g0[3]) and np.isnan(g1[3]) and not np.isnan(np.delete(g0, 3)).any() and not np.isnan(np.delete(g1, 3)).any(), (dtype, cols, g0, g1)
            assert g0[5] == -np.inf and g1[5] == np.inf
    for cols, col in ((64 * nv + nv, 64 * nv + 1), (257, 256)):
        rows = 65
        x = C.base_values(rows * cols, dtype, "nancols", cols).reshape(rows, cols)
        x[64, col], x[0, 2], x[63, 2] = np.nan, np.inf, -np.inf
        mn, mx = Buf(dev, 4 * cols, fill=F32(np.inf)), Buf(dev, 4 * cols, fill=F32(-np.inf))
        for u in (x, np.full((rows, cols), 0.5, dt), np.full((rows, cols), np.inf, dt)):
            _call("mq_minmax_cols", _inp(dev, u).ptr, MQ[dtype], rows, cols, mn.ptr, mx.ptr, _stream())
            g0, g1 = mn.take(F32, "min"), mx.take(F32, "max")
            assert np.isnan(g0[col]) and np.isnan(g1[col]) and not np.isnan(np.delete(g0, col)).any() and not np.isnan(np.delete(g1, col)).any(), (dtype, cols)
            assert g0[2] == -np.inf and g1[2] == np.inf
        z = C.zeros_input(rows * cols, dtype).reshape(rows, cols)
        mn, mx = Buf(dev, 4 * cols, fill=F32(np.inf)), Buf(dev, 4 * cols, fill=F32(-np.inf))
        _call("mq_minmax_cols", _inp(dev, z).ptr, MQ[dtype], rows, cols, mn.ptr, mx.ptr, _stream())
        assert np.all(mn.take(F32, "min") == 0) and np.all(mx.take(F32, "max") == 0)


# ---- score chain ----------------------------------------------------------------------------------------------------------------------
def compare_probs(got, raw, what, mask=None, causal=False, rows=None, chunk=2048):
    """got [rows, cols] against oracle.calib_probs of raw, chunk by chunk: NaN rows all NaN, finite rows finite, summing to 1 within
    n 2^-24, masked entries exactly 0, every entry inside the bar.  Updates WORST.  `rows`: only these."""
    n, cols = raw.shape
    sel = np.arange(n) if rows is None else np.asarray(sorted(rows))
    for s in range(0, len(sel), chunk):
        idx = sel[s:s + chunk]
        o = _oracle_rows(raw, idx, mask, causal)
        g = got[idx]
        nan_got = np.isnan(g)
        bad = np.flatnonzero(nan_got.all(axis=1) != o["nan_row"])
        bad = bad if len(bad) else np.flatnonzero(nan_got.any(axis=1) != o["nan_row"])
        if len(bad):
            r = int(idx[bad[0]])
            pytest.fail("%s: row %d: oracle says %s, kernel wrote %d NaN of %d" % (what, r, "NaN" if o["nan_row"][bad[0]] else "finite", nan_got[bad[0]].sum(), cols))
        fin = ~o["nan_row"]
        g, p, m, x = g[fin], o["p"][fin], o["masked"][fin], o["x"][fin]
        ridx = idx[fin]
        if not len(g):
            continue
        bad = np.argwhere(m & (g != 0))
        if len(bad):
            pytest.fail("%s: masked entry (row %d, col %d) is %r, not 0" % (what, ridx[bad[0][0]], bad[0][1], float(g[bad[0][0], bad[0][1]])))
        sums = np.abs(g.astype(np.float64).sum(axis=1) - 1)
        assert sums.max() <= cols * 2.0 ** -24, "%s: row %d sums to 1 %+g" % (what, ridx[int(sums.argmax())], sums.max())
        err = np.abs(g.astype(np.float64) - p)
        ulp = err / np.spacing(np.maximum(np.abs(p), 2.0 ** -126).astype(F32)).astype(np.float64)
        WORST["ulp"], WORST["abs"] = max(WORST["ulp"], float(ulp.max())), max(WORST["abs"], float(err.max()))
        bad = np.argwhere((ulp > PROBS_ULP) | (err > PROBS_ABS))
        if len(bad):
            r, c = (int(v) for v in bad[0])
            pytest.fail("%s: %d entries outside %g ulp / %g, first at (row %d, col %d): got %r (%s) want %r, %.2f ulp, x = %r (%s)"
                        % (what, len(bad), PROBS_ULP, PROBS_ABS, ridx[r], c, float(g[r, c]), _bits(g[r, c]), float(p[r, c]), ulp[r, c], float(x[r, c]), _bits(x[r, c])))


def _oracle_rows(raw, idx, mask, causal):
    """oracle.calib_probs for the rows idx of raw: the mask row / diagonal of row i is that of i % period, so each row is paired with it."""
    cols = raw.shape[1]
    sub = raw[idx]
    if causal:
        m = np.where(np.arange(cols)[None, :] > (idx % cols)[:, None], C.NINF, F32(0)).astype(F32)
        return O.calib_probs(sub, C.INV_SQRT_D, mask=m)
    if mask is not None:
        return O.calib_probs(sub, C.INV_SQRT_D, mask=mask[idx % mask.shape[0]])
    return O.calib_probs(sub, C.INV_SQRT_D)


def check_prob_stats(st, raw, got, what, full=None):
    """[raw min, raw max, p min, p max]: the raw pair exact, the probability pair exactly that of the written tensor."""
    check_stat(st[:2], [np_min(raw), np_max(raw)], what + " raw statistic")
    w = got if full is None else full
    check_stat(st[2:], [np_min(w), np_max(w)], what + " probability statistic")


def run_probs(dev, raw_b, out_b, rows, cols, mask_b, mask_rows, slots):
    _call("mq_calib_attention_probs", raw_b.ptr, out_b.ptr, rows, cols, mask_b.ptr if mask_b else None, mask_rows, C.SQRT_D,
          slots.ptr(0), slots.ptr(1), slots.ptr(2), slots.ptr(3), _stream())


def run_causal(dev, raw_b, out_b, rows, seq, store_masked, slots):
    _call("mq_calib_attention_probs_causal", raw_b.ptr, out_b.ptr, rows, seq, C.SQRT_D, int(store_masked), slots.ptr(0), slots.ptr(1),
          slots.ptr(2), slots.ptr(3), _stream())


@pytest.mark.parametrize("c", C.PROBS_CASES, ids=lambda c: c.id)
def test_calib_attention_probs(dev, c):
    """The explicit-mask / no-mask chain on either side of every VPT edge and, at 70 x 130 rows of 260 keys under a [130, 260] mask, on the
    second, ragged trip of the 2048-workgroup grid (row % mask_rows across trips).  The extremes move from plant row to plant row; the
    last variant runs in place, as calibration does."""
    vs = list(C.probs_variants(c))
    for v in vs:
        raw, mask = C.probs_input(c, v)
        what = "mq_calib_attention_probs %s variant %d" % (c.id, v)
        rb = _inp(dev, raw)
        ob = rb if v == vs[-1] else Buf(dev, raw.nbytes)
        mb = _inp(dev, mask) if mask is not None else None
        slots = minmax_slots(dev, 2)
        run_probs(dev, rb, ob, c.rows, c.cols, mb, c.mask_rows, slots)
        got = ob.take(F32, "probs").reshape(c.rows, c.cols)
        if ob is not rb:
            assert np.array_equal(rb.take(np.uint8, "raw"), raw.view(np.uint8).reshape(-1)), "raw was written"
        compare_probs(got, raw, what, mask=mask)
        check_prob_stats(slots.take(what), raw, got, what)
        r = C.plant_rows(c.rows, C.probs_geom(c.rows, c.cols)[2])[v]
        assert np_max(raw) == raw[r, 0] == 80 and np_min(raw) == raw[r, 1] == -80, what


def unwritten(seq, rows):
    """[rows, seq] bool: the quads that lie wholly above the diagonal of their row (store_masked = 0 leaves them alone)."""
    return (np.arange(seq)[None, :] // 4 * 4) > (np.arange(rows) % seq)[:, None]


@pytest.mark.parametrize("c", C.CAUSAL_CASES, ids=lambda c: c.id)
def test_calib_attention_probs_causal(dev, c):
    """The causal chain, single-trip and with an odd (bottom-up) and a partial last trip, store_masked 1 and 0.  Variant 0 with the masked
    stores is held to the float64 oracle entry by entry; every other (variant, store_masked) run has to equal it bit for bit outside the
    rows whose input moved (those against the oracle) and, without the masked stores, outside the quads above the diagonal, which keep
    what the buffer held (7 once, 0 otherwise).  At the multi-trip shapes the explicit-mask kernel has to agree bit for bit (a cross-check)."""
    S, rows = c.seq, c.seq * c.blocks
    base = C.causal_base(c)
    plants = C.causal_plants(c)
    rb = _inp(dev, base)
    rv = rb.dev_view(torch.float32).view(rows, S)
    skip = unwritten(S, rows)
    first = None
    for v, (prow, vals) in enumerate(plants):
        raw = base.copy()
        for (r, col), val in vals.items():
            raw[r, col] = val
            rv[r, col] = float(val)
        for sm in (1, 0):
            what = "mq_calib_attention_probs_causal %s variant %d store_masked %d" % (c.id, v, sm)
            fill = F32(7) if (v == 0 and not sm) else F32(0)
            ob = Buf(dev, raw.nbytes, fill=fill)
            slots = minmax_slots(dev, 2)
            run_causal(dev, rb, ob, rows, S, sm, slots)
            got = ob.take(F32, "probs").reshape(rows, S)
            full = got
            if not sm:
                assert np.all(got[skip] == fill), "%s: a quad above the diagonal was stored" % what
                full = np.where(skip, F32(0), got)
            if first is None:
                compare_probs(got, raw, what, causal=True)
                first, first_row = got, prow
            else:
                moved = {prow, first_row}
                compare_probs(full, raw, what, causal=True, rows=moved)
                keep = np.ones(rows, bool)
                keep[list(moved)] = False
                check_bits(full[keep], first[keep], raw[keep], what + " against variant 0")
            check_prob_stats(slots.take(what), raw, got, what, full=full)
            assert np_max(raw) == raw[prow, 0] == 80 and np_min(raw) == raw[prow, 1] == -80
        if v == len(plants) - 1 and len(C.causal_geom(rows, S)[3]) > 1:
            mb = _inp(dev, C.odd_mask(S))
            ob, slots = Buf(dev, raw.nbytes), minmax_slots(dev, 2)
            run_probs(dev, rb, ob, rows, S, mb, S, slots)
            other = ob.take(F32, "probs").reshape(rows, S)
            check_bits(other, full, raw, "mq_calib_attention_probs under the causal mask against %s" % what)
        for (r, col) in vals:
            rv[r, col] = float(base[r, col])


@pytest.mark.parametrize("seq", C.ODD_SEQ)
def test_calib_attention_probs_odd_rows(dev, seq):
    """Rows with a NaN or an infinity take the causal kernel's full pass: -inf on either side of the diagonal leaves an ordinary row, +inf
    on either side, a NaN on either side and an all -inf live region give an all-NaN row -- the causal and the explicit-mask kernel alike,
    against the op-for-op oracle; without the masked stores the quads above the diagonal keep the buffer's content on NaN rows too."""
    raw, marks = C.odd_input(seq)
    rows = raw.shape[0]
    o = O.calib_probs(raw, C.INV_SQRT_D, causal=True)
    for r, name, nan in marks:
        assert bool(o["nan_row"][r]) == nan, (r, name)
    rb = _inp(dev, raw)
    skip = unwritten(seq, rows)
    outs = {}
    for tag, fill in (("causal sm1", 0), ("causal sm0 zeros", 0), ("causal sm0 sevens", 7), ("mask", 0)):
        what = "odd rows S %d %s" % (seq, tag)
        ob, slots = Buf(dev, raw.nbytes, fill=F32(fill)), minmax_slots(dev, 2)
        if tag == "mask":
            run_probs(dev, rb, ob, rows, seq, _inp(dev, C.odd_mask(seq)), seq, slots)
        else:
            run_causal(dev, rb, ob, rows, seq, int("sm1" in tag), slots)
        got = ob.take(F32, "probs").reshape(rows, seq)
        if "sm0" in tag:                                                # the skipped quads keep the fill; the rest is the full pass
            assert np.all(got[skip] == fill), "%s: a quad above the diagonal was stored" % what
            got = np.where(skip, outs["causal sm1"], got)
        compare_probs(got, raw, what, causal=True)
        st = slots.take(what)
        assert np.isnan(st).all(), "%s: a NaN score makes all four statistics NaN, got %r" % (what, st)
        outs[tag] = got
    for tag in outs:
        check_bits(outs[tag], outs["causal sm1"], raw, "odd rows S %d: %s against the full causal pass" % (seq, tag))


def test_calib_attention_probs_all_ones_row_sum(dev):
    """Rows whose only live entries are 0 and -k 2^-23 (k = 1 .. 4): with expf correctly rounded there, k = 1 sums to l = 0x3fffffff, the
    divisor whose reciprocal form the kernel does not trust (`quick` false: the true divide).  The device's expf is not specified to the
    bit, so l is read back from the two stored probabilities (calib_cases.allones_table): every row has to hold the IEEE quotients of some
    ex = 1 - j 2^-24, and at least one row has to hold the pair of an all-ones l -- a coverage condition, not a tolerance."""
    raw, mask, info = C.allones_input()
    rb, mb, ob, slots = _inp(dev, raw), _inp(dev, mask), Buf(dev, raw.nbytes), minmax_slots(dev, 2)
    run_probs(dev, rb, ob, raw.shape[0], raw.shape[1], mb, raw.shape[0], slots)
    got = ob.take(F32, "probs").reshape(raw.shape)
    tab = C.allones_table()
    ones = 0
    for r, k, c0, c1 in info:
        key = (int(got[r, c0].view(np.uint32)), int(got[r, c1].view(np.uint32)))
        assert key in tab, "row %d (k = %d): stored (%s, %s) are not the IEEE quotients 1 / l, ex / l of any ex = 1 - j 2^-24" % (r, k, hex(key[0]), hex(key[1]))
        ones += any(l & 0x7fffff == 0x7fffff for _, l in tab[key])
        live = np.zeros(raw.shape[1], bool)
        live[[c0, c1]] = True
        assert np.all(got[r, ~live] == 0)
    assert ones >= 1, "no row formed a row sum with an all-ones significand on this device: the true-divide path did not run"
    compare_probs(got, raw, "all-ones rows", mask=mask)


# ---- mq_calib_norm ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", C.NORM_CASES, ids=lambda c: c.id)
def test_calib_norm(dev, c):
    """RMSNorm and LayerNorm on either side of every VPT edge, with and without the residual, its statistic slots and the bias, and at
    8192 + 37 rows (the capped grid's second trip, s_red reused row to row) with the extremes of h, y and delta moving through the first
    row, row 8191 and the last row.  h bit for bit; y inside the oracle's bound everywhere and bit for bit under the replay search (the
    wrap shape: on the rows around both ends of each trip and every 97th)."""
    x, d, w, b = C.norm_input(c)
    wrap = c.rows > 8192
    o = O.calib_norm_rows(x, d, w, b, C.NORM_EPS, c.ln, candidates=not wrap)
    xb, wb = _inp(dev, x), _inp(dev, w)
    db = _inp(dev, d) if d is not None else None
    bb = _inp(dev, b) if b is not None else None
    hb = Buf(dev, x.nbytes) if d is not None else None
    yb = Buf(dev, x.nbytes)
    slots = minmax_slots(dev, 3)
    _call("mq_calib_norm", xb.ptr, db.ptr if db else None, hb.ptr if hb else None, yb.ptr, c.rows, c.cols, wb.ptr, bb.ptr if bb else None,
          float(C.NORM_EPS), int(c.ln), slots.ptr(0), slots.ptr(1), slots.ptr(2), slots.ptr(3), slots.ptr(4) if c.slots else None,
          slots.ptr(5) if c.slots else None, _stream())
    what = "mq_calib_norm " + c.id
    y = yb.take(F32, "y").reshape(c.rows, c.cols)
    if hb:
        check_bits(hb.take(F32, "h").reshape(c.rows, c.cols), o["h"], x, what + " h")
    err = np.abs(y.astype(np.float64) - o["y64"])
    bad = np.argwhere(~(err <= o["err"]))
    if len(bad):
        r, k = (int(v) for v in bad[0])
        pytest.fail("%s: y outside the bound at (row %d, col %d): got %r (%s) want %r +- %g, h = %r (%s)"
                    % (what, r, k, float(y[r, k]), _bits(y[r, k]), o["y64"][r, k], o["err"][r, k], float(o["h"][r, k]), _bits(o["h"][r, k])))
    rows = range(c.rows) if not wrap else sorted(set(range(4)) | set(range(8188, 8196)) | set(range(c.rows - 4, c.rows)) | set(range(0, c.rows, 97)))
    for r in rows:
        cand = o["cand"][r] if not wrap else O.calib_norm_candidates(o["h"][r], C.NORM_EPS, c.ln)
        if not O.calib_norm_replay(y[r], o["h"][r], cand, w, b, c.ln):
            pytest.fail("%s: row %d: none of the %d fp32 row statistics within gamma_n of the float64 one reproduces y bit for bit (y[0] = %r (%s), h[0] = %r (%s))"
                        % (what, r, sum(len(rs) for _, rs in cand), float(y[r, 0]), _bits(y[r, 0]), float(o["h"][r, 0]), _bits(o["h"][r, 0])))
    st = slots.take(what)
    check_stat(st[:2], [np_min(o["h"]), np_max(o["h"])], what + " h statistic")
    check_stat(st[2:4], [np_min(y), np_max(y)], what + " y statistic")
    assert abs(float(st[2]) - o["y64"].min()) <= o["err"].max() and abs(float(st[3]) - o["y64"].max()) <= o["err"].max(), what
    check_stat(st[4:], [np_min(d), np_max(d)] if c.slots else [np.inf, -np.inf], what + " delta statistic")
    if wrap:
        assert {int(np.argmax(y.max(axis=1))), int(np.argmin(y.min(axis=1)))} <= set(C.NORM_WRAP_ROWS)


# ---- mq_calib_gated -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [0, 1], ids=["silu", "gelu"])
@pytest.mark.parametrize("numel", C.GATED_SIZES)
def test_calib_gated(dev, numel, act):
    """act(a) * b and its four statistic pairs up to the second trip of the 4096-workgroup grid; the extremes of a, b, act(a) and the product
    sit in the first quad, the last quad of the first trip and the last quad in turn."""
    import ctypes
    a0, b0 = C.gated_base(numel)
    ab, bb = _inp(dev, a0), _inp(dev, b0)
    av, bv = ab.dev_view(torch.float32), bb.dev_view(torch.float32)
    want_p, want_s = O.calib_gated(a0, b0, act)
    for quad in C.gated_quads(numel):
        what = "mq_calib_gated %s numel %d quad %d" % (("silu", "gelu")[act], numel, quad)
        plant = C.gated_plant(act, quad)
        a, b = a0.copy(), b0.copy()
        for i, (va, vb) in plant.items():
            a[i], b[i] = va, vb
            av[i], bv[i] = float(F32(va)), float(F32(vb))
        idx = sorted(plant)
        wp, ws = want_p.copy(), want_s.copy()
        wp[idx], ws[idx] = O.calib_gated(a[idx], b[idx], act)
        ob, slots = Buf(dev, a.nbytes), minmax_slots(dev, 4)
        arr = (ctypes.c_void_p * 8)(*[slots.ptr(k) for k in range(8)])
        _call("mq_calib_gated", ab.ptr, bb.ptr, ob.ptr, numel, act, arr, _stream())
        got = ob.take(F32, "product")
        err = np.abs(got.astype(np.float64) - wp)
        plain = PROD_ATOL + PROD_RTOL * np.abs(wp)
        lever = 0.5 * np.abs(a.astype(np.float64) * b.astype(np.float64))           # GELU: what erff's absolute error is multiplied by
        if act == 1:
            WORST["erf"] = max(WORST["erf"], float((np.maximum(err - plain, 0) / np.maximum(lever, 1e-30)).max()))
        ratio = err / (plain + (GELU_ERF_ABS * lever if act == 1 else 0))
        WORST["prod"] = max(WORST["prod"], float(ratio.max()))
        bad = np.flatnonzero(~(ratio <= 1))
        if len(bad):
            i = int(bad[0])
            pytest.fail("%s: %d products outside rtol %g / atol %g (GELU: + 0.5 |a b| erf term), first at %d (quad %d): got %r (%s) want %r, a = %r (%s), b = %r (%s)"
                        % (what, len(bad), PROD_RTOL, PROD_ATOL, i, i // 4, float(got[i]), _bits(got[i]), wp[i], float(a[i]), _bits(a[i]), float(b[i]), _bits(b[i])))
        st = slots.take(what)
        check_stat(st[0:2], [np_min(a), np_max(a)], what + " a statistic")
        check_stat(st[4:6], [np_min(b), np_max(b)], what + " b statistic")
        check_stat(st[6:8], [np_min(got), np_max(got)], what + " product statistic")
        assert np.all(np.abs(st[6:8].astype(np.float64) - [wp.min(), wp.max()]) <= PROD_ATOL + PROD_RTOL * np.abs([wp.min(), wp.max()])), what
        lo, hi = ws.min(), ws.max()
        r = max(abs(float(st[2]) - lo) / (1e-6 * max(1, abs(lo))), abs(float(st[3]) - hi) / (2e-6 * abs(hi)))
        WORST["act"] = max(WORST["act"], r)
        assert r <= 1, "%s: act(a) statistic [%r, %r] against float64 [%r, %r]" % (what, float(st[2]), float(st[3]), lo, hi)
        assert abs(hi - 9) < 1e-2 and int(np.argmax(ws)) == 4 * quad and int(np.argmax(wp)) == 4 * quad and int(np.argmin(wp)) == 4 * quad + 1
        for i in plant:
            av[i], bv[i] = float(a0[i]), float(b0[i])


# ---- mq_calib_rope / mq_calib_rope_qkv --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", C.ROPE_CASES, ids=lambda c: c.id)
def test_calib_rope(dev, c):
    """Rotated q / k (and v carried along with repeat_kv) bit for bit, every statistic exact: the project's geometries, the capped grid's
    second trip (8400 (b, s) rows), head_dim 1024 (one head per sweep) and head_dim 12 with 8 rotated dims (dq = 3: no shift, an idle
    partial head slot, pass-through lanes)."""
    import ctypes
    q, k, v, cos, sin = C.rope_input(c)
    rep = c.H // c.KV if c.qkv else 1
    want = [O.calib_rope(q, c.H, c.D, cos, sin), O.calib_rope(k, c.KV, c.D, cos, sin, True, rep)]
    ins = [q, k]
    if c.qkv:
        want.append(O.calib_rope(v, c.KV, c.D, cos, sin, False, rep))
        ins.append(v)
    inb = [_inp(dev, t) for t in ins]
    outb = [Buf(dev, t.nbytes) for t in want]
    cb, sb = _inp(dev, cos), _inp(dev, sin)
    nst = 5 if c.qkv else 4
    slots = minmax_slots(dev, nst)
    if c.qkv:
        arr = (ctypes.c_void_p * 12)(*([slots.ptr(i) for i in range(10)] + [None, None]))
        _call("mq_calib_rope_qkv", inb[0].ptr, inb[1].ptr, inb[2].ptr, outb[0].ptr, outb[1].ptr, outb[2].ptr, c.B, c.S, c.H, c.KV, c.D, c.rot,
              cb.ptr, sb.ptr, arr, _stream())
    else:
        arr = (ctypes.c_void_p * 8)(*[slots.ptr(i) for i in range(8)])
        _call("mq_calib_rope", inb[0].ptr, inb[1].ptr, outb[0].ptr, outb[1].ptr, c.B, c.S, c.H, c.KV, c.D, c.rot, cb.ptr, sb.ptr, arr, _stream())
    what = ("mq_calib_rope_qkv " if c.qkv else "mq_calib_rope ") + c.id
    st = slots.take(what)
    for i, name in enumerate("qkv"[:len(ins)]):
        got = outb[i].take(F32, name).reshape(want[i].shape)
        heads = want[i].shape[1]
        bad = np.argwhere(got.view(np.uint32) != want[i].view(np.uint32))
        if len(bad):
            bi, hi, si, di = (int(t) for t in bad[0])
            pytest.fail("%s: %s differs in %d of %d, first at (b %d, head %d, s %d, d %d) = (row %d, col %d): got %r (%s) want %r (%s)"
                        % (what, name, len(bad), got.size, bi, hi, si, di, bi * c.S + si, hi * c.D + di, float(got[bi, hi, si, di]),
                           _bits(got[bi, hi, si, di]), float(want[i][bi, hi, si, di]), _bits(want[i][bi, hi, si, di])))
        check_stat(st[4 * i:4 * i + 2], [np_min(ins[i]), np_max(ins[i])], "%s %s-linear statistic" % (what, name))
        if i < 2:
            check_stat(st[4 * i + 2:4 * i + 4], [np_min(want[i]), np_max(want[i])], "%s rotated %s statistic" % (what, name))
        assert heads == (c.H if (i == 0 or c.qkv) else c.KV)


# ---- argument checks --------------------------------------------------------------------------------------------------------------------
def test_calib_argument_checks(dev):
    """Every documented rejection returns its status and touches nothing: outputs and statistic slots keep their bytes, canaries included.
    MQ_EUNSUPPORTED (3): cols % 4, cols > 4096 (score chain) / > 8192 (norm), misaligned pointers; MQ_EINVAL (1): rows % seq, rows %
    mask_rows, store_masked = 0 in place.  Zero-sized inputs return MQ_OK and touch nothing."""
    import ctypes
    raw = C._scores(8, 8200, "args")
    rb, ob = _inp(dev, raw), Buf(dev, raw.nbytes, fill=F32(7))
    mb = _inp(dev, np.zeros((2, 8200), F32))
    w = _inp(dev, np.ones(8200, F32))
    slots = minmax_slots(dev, 4)
    s4 = [slots.ptr(i) for i in range(4)]
    st = _stream()
    for cols in (6, 4100):
        _refused(3, "mq_calib_attention_probs", rb.ptr, ob.ptr, 8, cols, None, 0, C.SQRT_D, *s4, st)
        _refused(3, "mq_calib_attention_probs_causal", rb.ptr, ob.ptr, cols * 2, cols, C.SQRT_D, 1, *s4, st)
    _refused(3, "mq_calib_attention_probs", rb.ptr + 4, ob.ptr, 8, 8, None, 0, C.SQRT_D, *s4, st)
    _refused(3, "mq_calib_attention_probs", rb.ptr, ob.ptr + 8, 8, 8, None, 0, C.SQRT_D, *s4, st)
    _refused(3, "mq_calib_attention_probs", rb.ptr, ob.ptr, 8, 8, mb.ptr + 4, 2, C.SQRT_D, *s4, st)
    _refused(3, "mq_calib_attention_probs_causal", rb.ptr + 4, ob.ptr, 8, 8, C.SQRT_D, 1, *s4, st)
    _refused(1, "mq_calib_attention_probs", rb.ptr, ob.ptr, 8, 8, mb.ptr, 3, C.SQRT_D, *s4, st)
    _refused(1, "mq_calib_attention_probs_causal", rb.ptr, ob.ptr, 12, 8, C.SQRT_D, 1, *s4, st)
    _refused(1, "mq_calib_attention_probs_causal", ob.ptr, ob.ptr, 8, 8, C.SQRT_D, 0, *s4, st)
    s6 = [slots.ptr(i) for i in range(6)]
    for cols in (6, 8196):
        _refused(3, "mq_calib_norm", rb.ptr, None, None, ob.ptr, 2, cols, w.ptr, None, 1e-5, 0, *s6[:4], None, None, st)
    _refused(3, "mq_calib_norm", rb.ptr + 4, None, None, ob.ptr, 2, 8, w.ptr, None, 1e-5, 0, *s6[:4], None, None, st)
    _refused(3, "mq_calib_norm", rb.ptr, None, None, ob.ptr, 2, 8, w.ptr + 4, None, 1e-5, 1, *s6[:4], None, None, st)
    _refused(1, "mq_calib_norm", rb.ptr, rb.ptr, None, ob.ptr, 2, 8, w.ptr, None, 1e-5, 0, *s6[:4], None, None, st)          # a residual needs h_out
    _refused(1, "mq_calib_norm", rb.ptr, None, None, ob.ptr, 2, 8, w.ptr, None, 1e-5, 0, *s6, st)                            # its slots need a residual
    arr = (ctypes.c_void_p * 8)(*[slots.ptr(k) for k in range(8)])
    _refused(3, "mq_calib_gated", rb.ptr, rb.ptr, ob.ptr, 6, 0, arr, st)
    _refused(3, "mq_calib_gated", rb.ptr + 4, rb.ptr, ob.ptr, 8, 0, arr, st)
    _refused(1, "mq_calib_gated", rb.ptr, rb.ptr, ob.ptr, 8, 2, arr, st)
    _refused(3, "mq_calib_rope", rb.ptr, rb.ptr, ob.ptr, ob.ptr, 1, 2, 2, 1, 6, 8, w.ptr, w.ptr, arr, st)                     # head_dim % 4
    _refused(3, "mq_calib_rope", rb.ptr, rb.ptr, ob.ptr, ob.ptr, 1, 2, 2, 1, 16, 12, w.ptr, w.ptr, arr, st)                   # rot_dim % 8
    _refused(1, "mq_calib_rope", rb.ptr, rb.ptr, ob.ptr, ob.ptr, 1, 2, 3, 2, 16, 8, w.ptr, w.ptr, arr, st)                    # heads % kv_heads
    # zero-sized inputs: MQ_OK, nothing touched
    _call("mq_calib_attention_probs", rb.ptr, ob.ptr, 0, 8, None, 0, C.SQRT_D, *s4, st)
    _call("mq_calib_attention_probs", rb.ptr, ob.ptr, 8, 0, None, 0, C.SQRT_D, *s4, st)
    _call("mq_calib_attention_probs_causal", rb.ptr, ob.ptr, 0, 8, C.SQRT_D, 1, *s4, st)
    _call("mq_calib_norm", rb.ptr, None, None, ob.ptr, 0, 8, w.ptr, None, 1e-5, 0, *s6[:4], None, None, st)
    _call("mq_calib_gated", rb.ptr, rb.ptr, ob.ptr, 0, 0, arr, st)
    _call("mq_calib_rope", rb.ptr, rb.ptr, ob.ptr, ob.ptr, 0, 2, 2, 1, 16, 8, w.ptr, w.ptr, arr, st)
    _call("mq_minmax_tensor", rb.ptr, 0, 0, s4[0], s4[1], st)
    _call("mq_minmax_rows", rb.ptr, 0, 0, 8, ob.ptr, ob.ptr, st)
    _call("mq_minmax_rows", rb.ptr, 0, 8, 0, ob.ptr, ob.ptr, st)
    _call("mq_minmax_cols", rb.ptr, 0, 0, 8, ob.ptr, ob.ptr, st)
    _refused(3, "mq_minmax_tensor", rb.ptr, 2, 8, s4[0], s4[1], st)                                                             # dtype
    assert np.all(ob.take(F32, "out") == 7), "a refused or empty call wrote its output"
    check_stat(slots.take("argument checks"), np.tile(np.array([np.inf, -np.inf], F32), 4), "statistic slots after refused and empty calls")
    assert np.array_equal(rb.take(np.uint8, "raw"), raw.view(np.uint8).reshape(-1))
