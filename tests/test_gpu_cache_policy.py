"""GPU: the headline step's two kernels (csrc/mq_quantize.hip quantize_tiled8_kernel, csrc/mq_gemm.hip gemm_i8_fr_kernel) at the
smallest shapes where a cache policy on their loads or stores could show: a policy moves no byte, so every image byte (padding rows
included), row sum and output is held EXACTLY to the oracles of quantize_cases.py / gemm_cases.py.

mq_quantize_tiled (staged kernel, u8 / shift 128 and symmetric / shift 0 grids, with and without row sums):
  [64, 1024], [80, 2048]  every workgroup on the full path (streaming x loads)
  [70, 2048]              rows 68..71 in a ragged workgroup, rows 72..79 in padding workgroups
The WHOLE image is compared: the padding rows of the last row block hold the last real row (the kernel's clamp).

mq_w8a8_linear_tiled, u8 and i8 storage.  The entry point serves the 176-column kernel from 192 tiles on (mq_gemm_tiled_supported), so
the two tile geometries run at N = 192 x 176 = 33 792, one row of tiles:
  M = 256, K = 768    whole tiles at the smallest K the kernel accepts
  M = 200, K = 1024   a ragged last row block (masked group stores) in every tile; the 176-byte rows of neighbouring column tiles share
                      cache lines
One more case runs quantize -> GEMM -> quantize (another input) -> GEMM on the same buffers without a synchronisation and checks the
second result: the image passes from one kernel's stores to the other's loads twice, the second time over lines the GEMM has read.

Measured wall time of the file on an MI355X: 5.9 s for its 11 tests (the slowest 1.0 s: the oracle of a 33 792-column GEMM)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gemm_cases as G  # noqa: E402
import quantize_cases as C  # noqa: E402
from oracle import mq_oracle as O  # noqa: E402
from test_gpu_gemm_epilogue import Linear, _report, _run_single, hooks  # noqa: E402
from test_gpu_quantize import MQ, Buf, _call, _inp, _stream, check_sums, dev  # noqa: E402,F401

pytestmark = pytest.mark.gpu
F32 = np.float32

QUANTIZE_CASES = [C.TCase("full-64x1024", 64, 1024), C.TCase("full-80x2048", 80, 2048), C.TCase("ragged-70x2048", 70, 2048)]
QUANTIZE_GRIDS = [g for g in C.TILED_GRIDS if g[0] in ("u8", "sym")]


def _padded_image(x, sc, of, qmin, qmax, shift):
    """(the whole image of x with the last row repeated up to a multiple of 16 rows, the real rows' sums)"""
    rows, cols = x.shape
    mp = (rows + 15) // 16 * 16
    xp = np.concatenate([x, np.repeat(x[-1:], mp - rows, axis=0)])
    stored, rs = O.quantize_storage(xp, sc, of, qmin, qmax, shift, None)
    want, real = O.tiled_image_bytes(stored, mp, cols)
    assert real.all()
    return want, rs[:rows]


@pytest.mark.parametrize("row_sum", [True, False], ids=["rowsum", "nosum"])
@pytest.mark.parametrize("c", QUANTIZE_CASES, ids=lambda c: c.id)
def test_quantize_tiled_image_and_sums(dev, c, row_sum):  # noqa: F811
    b = C.tiled_branch(c)
    assert b["kernel"] == "staged-V%d-rows4" % (c.cols // 1024)
    assert (c.rows % 16 == 0) == c.id.startswith("full")
    mp = (c.rows + 15) // 16 * 16
    for grid, shift in QUANTIZE_GRIDS:
        x, sc, of, qmin, qmax, cs = C.tiled_inputs(c, grid)
        assert cs is None
        want, want_rs = _padded_image(x, sc, of, qmin, qmax, shift)
        what = "%s %s%s" % (c.id, grid, " +row_sum" if row_sum else "")
        xb, sb, ob = _inp(dev, x), _inp(dev, sc), _inp(dev, of)
        q = Buf(dev, mp * c.cols)
        rs = Buf(dev, c.rows * 4) if row_sum else None
        _call("mq_quantize_tiled", xb.ptr, MQ["f32"], c.rows, c.cols, sb.ptr, ob.ptr, float(qmin), float(qmax), int(shift), None, q.ptr,
              rs.ptr if rs else None, _stream())
        torch.cuda.synchronize()
        got = q.take(np.int8, "q_tiled")
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, "%s: %d image bytes differ, first at byte %d (row block %d): got %d want %d" % (
            what, len(bad), bad[0], bad[0] // (16 * c.cols), got[bad[0]], want[bad[0]])
        if row_sum:
            check_sums(rs.take(np.int32, "row_sum"), want_rs, what)


GEMM_N = 192 * 176
GEMM_CASES = [G._case("tiled", (M, GEMM_N, K), grid) for M, K in ((256, 768), (200, 1024)) for grid in ("u8", "i8u")]


@pytest.mark.parametrize("c", GEMM_CASES, ids=lambda c: c.id)
def test_w8a8_linear_tiled_outputs(dev, c):  # noqa: F811
    (kernel, tile), = G.kernels_of(c)
    assert kernel == "fr" and tile == (256, 176) and (c.M + 255) // 256 == 1
    with hooks(c):
        got = _run_single(dev, c)
    e = G.expect(c)
    _report(c, kernel, tile, 0, got, e.stored, e, G.problem(c), "output")


def test_quantize_gemm_twice_on_the_same_buffers(dev):  # noqa: F811
    c = GEMM_CASES[2]                                       # M = 200 (ragged), K = 1024, u8
    M, N, K = c.M, c.N, c.K
    p = G.problem(c)
    g = G.GRIDS[c.grid]
    qc = C.TCase("chain-200x1024", M, K)
    assert C.tiled_branch(qc)["kernel"] == "staged-V1-rows4"
    x1, sc, of, qmin, qmax, _ = C.tiled_inputs(qc, "u8")
    x2 = np.ascontiguousarray(x1[::-1] * F32(0.5))
    assert not np.array_equal(x1, x2)
    stored2, rs2 = O.quantize_storage(x2, sc, of, qmin, qmax, 128, None)
    assert stored2.min() >= -128 and stored2.max() <= 127
    t = O.prefill_gemm_acc(stored2.astype(np.int8), p.w, rs2.astype(np.int32), p.w_zp, p.col_term)
    want, _, _ = O.prefill_gemm_epilogue(t, p.alpha, p.bias, p.grids, p.seg_end, g.qmin, g.qmax, G.storage_of(c), None)
    lin = Linear(dev, c, p)
    xb = [_inp(dev, x1), _inp(dev, x2)]
    sb, ob = _inp(dev, sc), _inp(dev, of)
    a = Buf(dev, (M + 15) // 16 * 16 * K)
    rs = Buf(dev, M * 4)
    out = Buf(dev, M * N)
    for i in range(2):
        _call("mq_quantize_tiled", xb[i].ptr, MQ["f32"], M, K, sb.ptr, ob.ptr, float(qmin), float(qmax), 128, None, a.ptr, rs.ptr, _stream())
        _call("mq_w8a8_linear_tiled", a.ptr, lin.w.ptr, M, N, K, rs.ptr, *lin.vectors(), lin.so, lin.oo, lin.qmin, lin.qmax, out.ptr,
              MQ[G.storage_of(c)], _stream())
    torch.cuda.synchronize()
    check_sums(rs.take(np.int32, "row_sum"), rs2, "second quantize")
    got = out.take(O.PREFILL_GEMM_STORAGE[G.storage_of(c)], "out").reshape(M, N)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "second GEMM: %d of %d outputs differ, first at %r: got %d want %d" % (
        len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])
