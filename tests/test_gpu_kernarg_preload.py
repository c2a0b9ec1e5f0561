"""GPU: the two kernels whose parameter lists were reordered for kernel-argument preload (csrc/mq_quantize.hip quantize_tiled8_kernel,
csrc/mq_gemm.hip gemm_i8_fr_kernel), at the smallest shapes where a moved or swapped argument shows: every pointer and scalar of
either list carries a value of its own (scale != offset, qmin != 0, out_scale != out_offset, N != M), so a swap changes the result.

mq_quantize_tiled: cols 1024 / 2048 / 4096 x rows 16 / 20 / 36 (full, ragged and padding workgroups of the lane-per-fragment kernel,
which serves rows < 64) and rows 64 / 66 / 68 (the same three kinds in the STAGED kernel, the one whose list changed: it takes
rows >= 64), with and without row sums, on two asymmetric grids (shift 128 and shift 0).  The image's real-row bytes and the row sums
are array_equal with oracle.quantize_storage / oracle.tiled_image_bytes, the oracle of test_gpu_quantize.py; canaries around both.

mq_w8a8_linear_tiled: the smallest launches the 176-column kernel accepts (192 tiles: N = 11264 at three row tiles), K = 768 and 1024,
M = 768 and 700 (the last row blocks clamped), u8 and i8 output, with and without row sums and bias.  Every output equals the int64
reference with the epilogue of test_gpu_round2.py (exact_u8).

Measured wall time of the file on an MI355X: 11.2 s for its 34 tests (the slowest 0.8 s; the float64 reference GEMMs are most of it)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import quantize_cases as C  # noqa: E402
from oracle import mq_oracle as O  # noqa: E402
from test_gpu_quantize import MQ, Buf, _call, _inp, _stream, check_sums, dev  # noqa: E402,F401
from test_gpu_round2 import T, exact_u8, tiled_image  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32

# (scale, offset, qmin, qmax, shift): asymmetric, qmin != 0, no two parameters equal; both fit int8 behind the shift
Q_GRIDS = [(0.027, 93.0, 3, 250, 128), (0.0043, -17.0, -100, 90, 0)]


def _quantize_input(rows, cols, grid):
    s, o, qmin, qmax, _ = grid
    rng = np.random.default_rng(rows * 8192 + cols + qmax)
    return C._fill(rows, cols, F32(s), F32(o), qmin, qmax, np.float32, False, rng)


@pytest.mark.parametrize("cols", [1024, 2048, 4096])
@pytest.mark.parametrize("rows", [16, 20, 36, 64, 66, 68])
def test_quantize_tiled_arguments(dev, rows, cols):  # noqa: F811
    staged = C.tiled_branch(C.TCase("k", rows, cols))["kernel"].startswith("staged")
    assert staged == (rows >= 64)
    for grid in Q_GRIDS:
        s, o, qmin, qmax, shift = grid
        x = _quantize_input(rows, cols, grid)
        sc, of = np.array([s], F32), np.array([o], F32)
        stored, want_rs = O.quantize_storage(x, sc, of, qmin, qmax, shift)
        want, real = O.tiled_image_bytes(stored, rows, cols)
        for row_sum in (True, False):
            what = "%dx%d grid %r%s" % (rows, cols, grid, " +row_sum" if row_sum else "")
            xb, sb, ob = _inp(dev, x), _inp(dev, sc), _inp(dev, of)
            q = Buf(dev, (rows + 15) // 16 * 16 * cols)
            rs = Buf(dev, rows * 4) if row_sum else None
            _call("mq_quantize_tiled", xb.ptr, MQ["f32"], rows, cols, sb.ptr, ob.ptr, float(qmin), float(qmax), int(shift), None, q.ptr,
                  rs.ptr if rs else None, _stream())
            torch.cuda.synchronize()
            got = q.take(np.int8, "q_tiled")
            assert np.array_equal(got[real], want[real]), "%s: %d image bytes differ" % (what, int((got[real] != want[real]).sum()))
            if row_sum:
                check_sums(rs.take(np.int32, "row_sum"), want_rs, what)
                assert np.array_equal(rs.take(np.int32, "row_sum"), want_rs), what


GEMM_N = 11264          # 64 column tiles of 176: with three row tiles the 192 tiles mq_gemm_tiled_supported asks for


@pytest.mark.parametrize("with_rowsum, with_bias", [(True, True), (False, False), (True, False), (False, True)])
@pytest.mark.parametrize("K", [768, 1024])
@pytest.mark.parametrize("M", [768, 700])
def test_w8a8_linear_tiled_arguments(dev, M, K, with_rowsum, with_bias):  # noqa: F811
    from mobilequant_amd import ops
    from mobilequant_amd._lib import MQ_I8, MQ_U8
    N = GEMM_N
    assert ops.gemm_tiled_supported(M, N, K) and not ops.gemm_tiled_supported(M, N - 176, K) and N != M
    rng = np.random.default_rng(M * 7 + K + 2 * with_rowsum + with_bias)
    qa = rng.integers(0, 256, size=(M, K))
    za, sa = int(rng.integers(1, 255)), F32(0.021)
    sw = rng.random(N, dtype=F32) * F32(1e-3) + F32(1e-4)
    if with_rowsum:                     # asymmetric weights: per-column zero points, stored with shift 128
        qw = rng.integers(0, 256, size=(N, K))
        zw, w_shift = rng.integers(0, 256, size=N), 128
    else:                               # a_rowsum = NULL needs w_zp == 0: symmetric weights, stored as they are
        qw = rng.integers(-128, 128, size=(N, K))
        zw, w_shift = np.zeros(N, np.int64), 0
    bias = rng.standard_normal(N, dtype=F32) if with_bias else None
    a8 = (qa - 128).astype(np.int8)
    w8 = (qw - w_shift).astype(np.int8)
    colsum = T(w8.astype(np.int64).sum(1).astype(np.int32), dev)
    alpha, wzp, ct = ops.linear_epilogue_prepare(T(np.array([sa], F32), dev), T(np.array([za], F32), dev), 128, T(sw, dev),
                                                 T(zw.astype(F32), dev), w_shift, colsum, K)
    _, pre = O.qlinear_int_exact(qa, za, sa, qw, zw, sw, bias, blas=True)
    so = F32((np.percentile(pre, 99.5) - np.percentile(pre, 0.5)) / 255.0)          # the clamp is reached at both ends
    oo = F32(np.rint(-np.percentile(pre, 0.5) / so))
    assert float(so) != float(oo)
    kernel, _ = exact_u8(qa, za, sa, qw, zw, sw, bias, so, oo)
    one = torch.ones(1, device=dev)
    kw = dict(out_scale=one * float(so), out_offset=one * float(oo), out_qmin=0.0, out_qmax=255.0, a_tiled_rows=M)
    a_t, w_t = T(tiled_image(a8), dev), T(w8, dev)
    rs = T(a8.astype(np.int64).sum(1).astype(np.int32), dev) if with_rowsum else None
    b = T(bias, dev) if with_bias else None
    canary = torch.full((M + 16, N), 77, dtype=torch.uint8, device=dev)
    ops.int8_linear(a_t, w_t, rs, alpha, wzp, ct, b, out_dtype=MQ_U8, out=canary[:M], **kw)
    got = canary[:M].cpu().numpy()
    assert np.array_equal(got, kernel), int((got != kernel).sum())
    assert bool((canary[M:] == 77).all())
    got_i8 = ops.int8_linear(a_t, w_t, rs, alpha, wzp, ct, b, out_dtype=MQ_I8, **kw).cpu().numpy()
    assert np.array_equal(got_i8.astype(np.int16) + 128, kernel.astype(np.int16))
