"""GPU: the quantize-to-integer kernels that feed every prefill GEMM -- mq_quantize, mq_quantize_tiled, mq_linear_epilogue_prepare,
mq_pack_w4 (csrc/mq_quantize.hip) -- and mq_fake_quant's forward (csrc/mq_fake_quant.hip) against plain numpy oracles, at every dispatch
branch, with nothing excluded: every index, every image byte of a real row, every row sum, every epilogue word and every fake-quantised
value is held EXACTLY, round-half-even ties and non-finite inputs included (integer storage: NaN, +-inf and an overflowing quotient
store qmin - shift; fake-quant keeps NaN).  No sibling kernel is a reference: the indices are oracle.quantize_storage (the reference's
IEEE expression), the image is oracle.tiled_image_bytes (the header's byte formula as index arithmetic), the epilogue vectors are
Python integers modulo 2^32.

Every call goes through ops._lib.call on buffers this file allocates: each output has 64 canary bytes in front of it and behind it
(pointer offsets included), and they have to survive.  Every case comes from quantize_cases.py, whose lists test_quantize_oracle.py
holds to the dispatch code on the CPU.  A failure names the first differing (row, column), got, want and the input's bit pattern.

Measured wall time of the whole file on an MI355X: 3.0 s for its 89 tests (the slowest, [16400, 256], 0.2 s)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import quantize_cases as C  # noqa: E402
from oracle import mq_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
CB, PAD = 0x55, 64                       # canary byte, canary bytes on either side
MQ = {"f32": 0, "f16": 1, "i8": 2, "u8": 3, "i16": 4, "u16": 5, "i32": 6}          # mq_dtype (include/mobilequant_amd.h)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    import mobilequant_amd._lib as L
    assert L.device_info()["arch"].startswith("gfx950")
    return torch.device("cuda:0")


def _call(name, *args):
    from mobilequant_amd import ops
    ops._lib.call(name, *args)


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Buf:
    """nbytes of device memory `off` bytes past a 64-byte boundary, canary bytes in front and behind; `data` (any array) fills it."""

    def __init__(self, dev, nbytes, off=0, data=None):
        self.n, self.a = nbytes, PAD + off
        h = np.full(self.a + nbytes + PAD, CB, np.uint8)
        if data is not None:
            raw = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
            assert raw.size == nbytes
            h[self.a:self.a + nbytes] = raw
        t = torch.empty(h.size + 64, dtype=torch.uint8, device=dev)
        skip = -t.data_ptr() % 64
        self.t = t[skip:skip + h.size]
        self.t.copy_(torch.from_numpy(h))
        assert self.t.data_ptr() % 64 == 0
        self.ptr = self.t.data_ptr() + self.a

    def take(self, dtype, what):
        h = self.t.cpu().numpy()
        assert np.all(h[:self.a] == CB), "canary in front of %s changed" % what
        assert np.all(h[self.a + self.n:] == CB), "canary behind %s changed" % what
        return h[self.a:self.a + self.n].copy().view(dtype)


def _inp(dev, a, off_bytes=0):
    return Buf(dev, a.nbytes, off_bytes, a)


def _bits(v):
    v = np.asarray(v)
    return "0x%0*x" % (2 * v.dtype.itemsize, int(v.view({2: np.uint16, 4: np.uint32}[v.dtype.itemsize])))


def check_ints(got, want, x, what):
    """Exact; the message names the first differing (row, column), got, want and the input's bit pattern."""
    got, want = np.asarray(got).astype(np.int64), np.asarray(want).astype(np.int64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    if len(bad):
        r, c = (int(v) for v in bad[0])
        pytest.fail("%s: %d of %d differ, first at (row %d, col %d): got %d want %d, x = %r (%s)"
                    % (what, len(bad), got.size, r, c, got[r, c], want[r, c], float(x[r, c]), _bits(x[r, c])))


def check_sums(got, want, what):
    got, want = np.asarray(got).astype(np.int64), np.asarray(want).astype(np.int64)
    bad = np.flatnonzero(got != want)
    if len(bad):
        pytest.fail("%s: row_sum differs in %d rows, first row %d: got %d want %d" % (what, len(bad), bad[0], got[bad[0]], want[bad[0]]))


def check_values(got, want, x, what):
    """Bit for bit, NaN exactly where the oracle has NaN."""
    u = {2: np.uint16, 4: np.uint32}[want.dtype.itemsize]
    assert got.shape == want.shape and got.dtype == want.dtype, what
    ng, nw = np.isnan(got), np.isnan(want)
    bad = np.argwhere((ng != nw) | (~nw & ~ng & (got.view(u) != want.view(u))))
    if len(bad):
        r, c = (int(v) for v in bad[0])
        pytest.fail("%s: %d of %d differ, first at (row %d, col %d): got %r (%s) want %r (%s), x = %r (%s)"
                    % (what, len(bad), got.size, r, c, float(got[r, c]), _bits(got[r, c]), float(want[r, c]), _bits(want[r, c]),
                       float(x[r, c]), _bits(x[r, c])))


# ---- mq_quantize ----------------------------------------------------------------------------------------------------------------
def run_quantize(dev, c, row_sum):
    x, sc, of, qmin, qmax, cs = C.quantize_inputs(c)
    qb = C.Q_BYTES[c.q_dtype]
    xb = _inp(dev, x, c.x_off * x.dtype.itemsize)
    sb, ob = _inp(dev, sc), _inp(dev, of)
    cb = _inp(dev, cs, c.cs_off) if cs is not None else None
    q = Buf(dev, c.rows * c.cols * qb, c.q_off)
    rs = Buf(dev, c.rows * 4) if row_sum else None
    _call("mq_quantize", xb.ptr, MQ[c.dtype], c.rows, c.cols, sb.ptr, ob.ptr, sc.size, float(qmin), float(qmax), int(c.shift),
          cb.ptr if cb else None, q.ptr, MQ[c.q_dtype], rs.ptr if rs else None, _stream())
    torch.cuda.synchronize()
    return (q.take(C.Q_NUMPY[c.q_dtype], "q").reshape(c.rows, c.cols), rs.take(np.int32, "row_sum") if rs else None)


@pytest.mark.parametrize("c", C.QUANTIZE_CASES, ids=lambda c: c.id)
def test_quantize(dev, c):
    """Every branch of launch_quantize with every storage width it serves (quantize_cases.QUANTIZE_CASES): the b16 wave-per-row kernel
    up to its wave-stride second sweep, the generic kernel's vector and scalar forms (by shape and by pointer), per-tensor and per-row
    grids, chan_scale in each form, non-finite inputs.  A case with row_sum runs without it as well: the indices may not depend on it."""
    x = C.quantize_inputs(c)[0]
    want, want_rs = C.quantize_expect(c)
    got, got_rs = run_quantize(dev, c, c.row_sum)
    check_ints(got, want, x, c.id)
    if c.row_sum:
        check_sums(got_rs, want_rs, c.id)
        if c.rows * c.cols <= 1 << 20:
            check_ints(run_quantize(dev, c, False)[0], want, x, c.id + " (no row_sum)")


# ---- mq_quantize_tiled ----------------------------------------------------------------------------------------------------------
def run_tiled(dev, c, grid, shift, row_sum):
    x, sc, of, qmin, qmax, cs = C.tiled_inputs(c, grid)
    mp = (c.rows + 15) // 16 * 16
    xb, sb, ob = _inp(dev, x), _inp(dev, sc), _inp(dev, of)
    cb = _inp(dev, cs) if cs is not None else None
    q = Buf(dev, mp * c.cols)
    rs = Buf(dev, c.rows * 4) if row_sum else None
    _call("mq_quantize_tiled", xb.ptr, MQ[c.dtype], c.rows, c.cols, sb.ptr, ob.ptr, float(qmin), float(qmax), int(shift),
          cb.ptr if cb else None, q.ptr, rs.ptr if rs else None, _stream())
    torch.cuda.synchronize()
    return q.take(np.int8, "q_tiled"), (rs.take(np.int32, "row_sum") if rs else None)


def check_image(got, c, grid, shift, stored, what):
    """The real-row bytes against tiled_image_bytes; the message goes back from the first differing byte to its (row, column)."""
    x = C.tiled_inputs(c, grid)[0]
    want, real = O.tiled_image_bytes(stored, c.rows, c.cols)
    assert got.shape == want.shape
    bad = np.flatnonzero((got != want) & real)
    if len(bad):
        r, k = np.meshgrid(np.arange(c.rows), np.arange(c.cols), indexing="ij")
        off = O.tiled_offset(r, k, c.cols)
        row, col = (int(v[0]) for v in np.nonzero(off == bad[0]))
        pytest.fail("%s: %d image bytes differ, first at byte %d = (row %d, col %d): got %d want %d, x = %r (%s)"
                    % (what, len(bad), bad[0], row, col, got[bad[0]], want[bad[0]], float(x[row, col]), _bits(x[row, col])))


@pytest.mark.parametrize("c", C.TILED_CASES, ids=lambda c: c.id)
def test_quantize_tiled(dev, c):
    """Both tiled kernels at every branch of mq_quantize_tiled (quantize_cases.TILED_CASES), each with and without row_sum, on the u8 /
    shift 128, symmetric / shift 0 and 4-bit grids: real-row bytes, row sums, canaries behind ceil16(rows) * cols bytes and row_sum[rows].
    The tuning hooks are process-wide: restored whatever happens."""
    try:
        _call("mq_quantize_tiled_set_rows", c.knob_rows)
        _call("mq_quantize_tiled_set_staged", c.staged)
        for grid, shift in C.TILED_GRIDS:
            x, sc, of, qmin, qmax, cs = C.tiled_inputs(c, grid)
            stored, want_rs = O.quantize_storage(x, sc, of, qmin, qmax, shift, cs)
            for row_sum in (True, False):
                what = "%s %s%s" % (c.id, grid, " +row_sum" if row_sum else "")
                got, got_rs = run_tiled(dev, c, grid, shift, row_sum)
                check_image(got, c, grid, shift, stored, what)
                if row_sum:
                    check_sums(got_rs, want_rs, what)
    finally:
        _call("mq_quantize_tiled_set_rows", 0)
        _call("mq_quantize_tiled_set_staged", 1)


# ---- mq_fake_quant --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", C.FAKE_QUANT_CASES, ids=lambda c: c.id)
def test_fake_quant_forward(dev, c):
    """Quantizer.forward at every branch of launch_fake_quant: fp32 and fp16, per-tensor (fp16: half arithmetic per op) and per-row (fp16:
    fp32 arithmetic, one final rounding), vector and scalar forms by shape and by pointer, y aliasing x, and one vector and one scalar
    case past the 2048 x 256 grid cap (the grid-stride loop's second trip).  NaN is kept; bit for bit."""
    x, sc, of, qmin, qmax = C.fake_quant_inputs(c)
    want = C.fake_quant_expect(c)
    xb = _inp(dev, x, c.x_off * x.dtype.itemsize)
    sb, ob = _inp(dev, sc), _inp(dev, of)
    y = xb if c.alias else Buf(dev, x.nbytes)
    _call("mq_fake_quant", xb.ptr, y.ptr, MQ[c.dtype], c.rows, c.cols, sb.ptr, ob.ptr, sc.size, float(qmin), float(qmax), _stream())
    torch.cuda.synchronize()
    check_values(y.take(x.dtype, "y").reshape(c.rows, c.cols), want, x, c.id)
    if not c.alias:
        assert np.array_equal(xb.take(np.uint8, "x"), np.asarray(x).view(np.uint8).reshape(-1)), "x was written"


# ---- mq_linear_epilogue_prepare ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", C.EPILOGUE_N)
def test_linear_epilogue_prepare(dev, N):
    """alpha, w_zp and col_term, exact: per-tensor and per-row weight grids, shifts 0 and 128, K up to 2^24 - 1, column sums and zero
    points that make col_term wrap in both directions (two's complement, as the header documents)."""
    for tag, c in C.all_epilogue_cases():
        if tag[0] != N:
            continue
        alpha, w_zp, col = O.linear_epilogue_vectors(**c)
        ins = [_inp(dev, c[k]) for k in ("a_scale", "a_offset", "w_scale", "w_offset", "w_colsum")]
        out = [Buf(dev, N * 4) for _ in range(3)]
        _call("mq_linear_epilogue_prepare", ins[0].ptr, ins[1].ptr, int(c["a_shift"]), ins[2].ptr, ins[3].ptr, c["w_scale"].size,
              int(c["w_shift"]), ins[4].ptr, N, int(c["K"]), out[0].ptr, out[1].ptr, out[2].ptr, _stream())
        torch.cuda.synchronize()
        g_alpha, g_zp, g_col = out[0].take(np.float32, "alpha"), out[1].take(np.int32, "w_zp"), out[2].take(np.int32, "col_term")
        for name, g, w in (("alpha", g_alpha.view(np.uint32), alpha.view(np.uint32)), ("w_zp", g_zp, w_zp), ("col_term", g_col, col)):
            bad = np.flatnonzero(g != w)
            assert not len(bad), "%s %r: first at n = %d: got %d want %d (colsum %d, w_offset %r)" % (
                name, tag, bad[0], g[bad[0]], w[bad[0]], c["w_colsum"][bad[0]], float(c["w_offset"][bad[0] % c["w_offset"].size]))


# ---- mq_pack_w4 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", C.PACK_SHAPES)
def test_pack_w4(dev, N, K):
    """oracle.pack_w4 byte for byte; (257, 192) has an output count that is no multiple of the 256-thread workgroup."""
    q = C.pack_input(N, K)
    want = O.pack_w4(q, 0)
    src, out = _inp(dev, q), Buf(dev, N * K // 2)
    _call("mq_pack_w4", src.ptr, N, K, out.ptr, _stream())
    torch.cuda.synchronize()
    check_ints(out.take(np.uint8, "packed").reshape(N, K // 2), want, np.zeros((N, K // 2), F32), "pack_w4 %dx%d" % (N, K))
