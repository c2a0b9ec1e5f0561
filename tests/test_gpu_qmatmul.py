"""GPU: mq_qmatmul (csrc/mq_qmatmul.hip) in all 28 instantiations and every epilogue route against oracle.qmatmul_launch, a plain numpy
restatement of the kernel's fixed sequence of operations.  EVERY element of every batch is compared on its stored bits, NaN exactly
where the oracle has NaN: no tolerance, no excluded share.  No sibling kernel and no torch operation is a reference.

Every operand, grid and case comes from qmatmul_cases.py, whose list test_qmatmul_oracle.py holds to its conditions on the CPU (the
dispatch predicate against the library's own mq_qmatmul_geometry, all instantiations and routes reached, planted ties, no saturation,
every oracle mutation detected).  Every call goes through the C ABI on buffers this file allocates (gpu_buffers.Buf): operands on the
base alignment the case names -- a base 4 bytes past a 16-byte boundary is real --, the output pre-filled with a pattern between 64
canary bytes that have to survive.  One launch per case.  A failure names the instantiation and the route the predicates expect, the
first differing (batch, row, column), its tile, wave and lane, the integer bracket, alpha, got, want and the oracle's distance to an
output tie.

Measured wall time of the whole file on an MI355X: 3.5 s for its 57 tests; the slowest, panel-kT-kc1-vec, 0.26 s (the first case: it
loads the library and pays the first launch), then the 11-MB cases of the 128-row tile kernel at 0.08 - 0.11 s each; most of that is
the numpy oracle, not the GPU.  Every kernel matched.  Against an oracle broken on purpose the file failed there in 5 of its 57 tests
(a float64 scale for 8-bit operands: exactly the cases whose brackets exceed 2^24), 47 (input ties rounded half up), 17 (output ties
rounded half up), 45 (NaN becomes qmax) and 51 (the zero-point term dropped from the row sums)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import qmatmul_cases as C  # noqa: E402
from gpu_buffers import Buf, check_bits  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
PATTERN = 0xA5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    import mobilequant_amd._lib as L
    assert L.device_info()["arch"].startswith("gfx950")
    return torch.device("cuda:0")


def _grid(dev, g, keep):
    """mq_grid of a (scale, offset, qmin, qmax) tuple; the two one-float device buffers are appended to `keep`."""
    import mobilequant_amd._lib as L
    s, o = Buf(dev, 4, data=np.array([g[0]], F32)), Buf(dev, 4, data=np.array([g[1]], F32))
    keep += [s, o]
    return L.MqGrid(s.ptr, o.ptr, g[2], g[3])


def _locate(c, k, b, r, n):
    """Where output (b, r, n) is computed: tile, wave and lane of the MFMA layout both kernels share (D[n][m]: a lane holds four consecutive
    columns of one row; wave w owns rows 16 w .. 16 w + 15 of every 64-row round)."""
    mt = 128 if k["panel"] else 64 * k["rf"]
    where = "tile (%d, %d) of batch element %d, row block %d, wave %d, lane %d (row %d of the fragment, columns %d + 0..3), element %d" % (
        r // mt, n // 64, b, (r % mt) // 64, (r % 64) // 16, r % 16 + 16 * ((n % 16) // 4), r % 16, 16 * ((n % 64) // 16) + 4 * ((n % 16) // 4), n % 4)
    if k["panel"]:
        where += ", column range %d of %d" % ((n // 64) // k["tiles_per_split"], k["nsplit"])
    return where


@pytest.mark.parametrize("c", C.CASES, ids=lambda c: c.id)
def test_qmatmul_every_output_bit(dev, c):
    import mobilequant_amd._lib as L
    k = C.kernel_of(c)
    plain, causes = C.epilogue_route(c)
    g1, g2, go = C.grids_of(c)
    x1, x2m = C.operands(c.id)
    e = C.expect(c.id)
    keep = []
    a = Buf(dev, x1.nbytes, c.a_off, x1)
    b = Buf(dev, x2m.nbytes, c.b_off, x2m)
    nout = c.batch * c.M * c.N * 4
    out = Buf(dev, nout, c.o_off, np.full(nout, PATTERN, np.uint8))
    assert a.ptr % 16 == c.a_off % 16 and b.ptr % 16 == c.b_off % 16 and out.ptr % 16 == c.o_off % 16
    m1, m2 = _grid(dev, g1, keep), _grid(dev, g2, keep)
    mo = _grid(dev, go, keep) if go is not None else None
    L.call("mq_qmatmul", a.ptr, b.ptr, out.ptr, c.batch, c.M, c.N, c.K, int(c.kcontig), ctypes.byref(m1), ctypes.byref(m2),
           ctypes.byref(mo) if mo is not None else None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = out.take(F32, "out of %s" % c.id).reshape(c.batch, c.M, c.N)
    want = e["out"]
    ng, nw = np.isnan(got), np.isnan(want)
    bad = np.argwhere((ng != nw) | (~ng & ~nw & (got.view(np.uint32) != want.view(np.uint32))))
    if len(bad):
        bi, r, n = (int(v) for v in bad[0])
        untouched = int((got.view(np.uint32)[tuple(bad.T)] == 0x01010101 * PATTERN).sum())
        pytest.fail("%s on %s, epilogue PLAIN %d (%s): %d of %d outputs differ (%d of them still hold the pre-fill pattern), first at (batch %d, row %d, "
                    "col %d) = %s: got %r (0x%08x) want %r (0x%08x); bracket t = %d, alpha = %r, v = %r, quotient %r, distance to an output tie %s"
                    % (c.id, k["name"], plain, ", ".join(sorted(causes)), len(bad), got.size, untouched, bi, r, n, _locate(c, k, bi, r, n),
                       float(got[bi, r, n]), int(got.view(np.uint32)[bi, r, n]), float(want[bi, r, n]), int(want.view(np.uint32)[bi, r, n]),
                       int(e["t"][bi, r, n]), float(e["alpha"]), float(e["v"][bi, r, n]), None if e["q"] is None else float(e["q"][bi, r, n]),
                       "-" if e["tie"] is None else "%.3g" % float(e["tie"][bi, r, n])))
    check_bits(got.reshape(-1, c.N), want.reshape(-1, c.N), None, "%s on %s" % (c.id, k["name"]))
