"""GPU: mq_w8a8_linear_grouped (csrc/mq_gemm_grouped.hip) in both instantiations against oracle.grouped_linear, a plain numpy restatement of
its fixed sequence of operations: per group, in group order, one int32 bracket, one int32 -> fp32 conversion and one fused multiply-add,
then one add of the bias.  EVERY output is compared on its stored bits: no tolerance, no excluded share.  No sibling kernel and no torch
operation is a reference.

Every operand, vector and case comes from grouped_gemm_cases.py, which test_qmatmul_oracle.py holds to its conditions on the CPU: both
instantiations reached, group sizes 64 ... 384 and 2048 / 2112 / 32768, 1 to 7 groups of both parities, M off and on the tile, with and
without a bias, brackets beyond 2^24 on exact ties of the conversion, cw at the edge of the 24-bit multiply, every bracket inside int32.
Every call goes through the C ABI on buffers this file allocates (gpu_buffers.Buf); the output is pre-filled with a pattern between 64
canary bytes that have to survive.  One launch per case.  A failure names the instantiation, the first differing (row, column), its
tile, wave and lane, the brackets of every group, their alphas, got and want.

Measured wall time of the whole file on an MI355X: 2.2 s for its 17 tests; the slowest, g64-G2, 0.09 s, and the 8-MB weight of
big-g32768-G2 no slower.  Every output matched.  Against an oracle broken on purpose the file failed there in 15 of its 17 tests (a
multiply and an add in place of the fma), 15 (groups folded in reverse order) and 5 (the bracket entering the fma as a float64: the
tie, mul24 and big cases, whose brackets exceed 2^24); the two single-group cases cannot tell the first two apart (fma(x, a, 0) is the
rounded product) and are there for K == group_size."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import grouped_gemm_cases as G  # noqa: E402
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


def _inp(dev, a):
    return Buf(dev, a.nbytes, 0, a)


@pytest.mark.parametrize("c", G.CASES, ids=lambda c: c.id)
def test_grouped_linear_every_output_bit(dev, c):
    import mobilequant_amd._lib as L
    p, e = G.problem(c.id), G.expect(c.id)
    K = c.gs * c.G
    a, w, ag, al, cw, t = (_inp(dev, p[n]) for n in ("a", "w", "a_gsum", "alpha", "cw", "t"))
    bias = _inp(dev, p["bias"]) if p["bias"] is not None else None
    nout = c.M * c.N * 4
    out = Buf(dev, nout, 0, np.full(nout, PATTERN, np.uint8))
    L.call("mq_w8a8_linear_grouped", a.ptr, w.ptr, c.M, c.N, K, c.gs, ag.ptr, al.ptr, cw.ptr, t.ptr, bias.ptr if bias is not None else None,
           out.ptr, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = out.take(F32, "out of %s" % c.id).reshape(c.M, c.N)
    want = e["out"]
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    if len(bad):
        r, n = (int(v) for v in bad[0])
        pytest.fail("%s on %s: %d of %d outputs differ, first at (row %d, col %d) = tile (%d, %d), wave %d (rows %d.., columns %d..), lane %d, "
                    "element %d: got %r (0x%08x) want %r (0x%08x); brackets per group %s, alpha %s, bias %r"
                    % (c.id, G.kernel_of(c), len(bad), got.size, r, n, r // 128, n // 128, 2 * ((r % 128) // 32) + (n % 128) // 64,
                       32 * ((r % 128) // 32), 64 * ((n % 128) // 64), r % 16 + 16 * ((n % 16) // 4), n % 4, float(got[r, n]),
                       int(got.view(np.uint32)[r, n]), float(want[r, n]), int(want.view(np.uint32)[r, n]), e["bracket"][:, r, n].tolist(),
                       p["alpha"][:, n].tolist(), None if p["bias"] is None else float(p["bias"][n])))
    check_bits(got, want, None, "%s on %s" % (c.id, G.kernel_of(c)))
