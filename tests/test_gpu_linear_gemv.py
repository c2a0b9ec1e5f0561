"""GPU: the M <= 8 weight-streaming GEMV behind QLinear -- gemv_i8_fat_kernel (csrc/mq_gemv.hip) in all twelve instantiations
(MT 1 / 2 / 4 token rows per pass over the weights, int8 or fused fp32 activations, int8 or packed 4-bit weights), through
mq_w8a8_linear, mq_w4a8_linear, mq_w8a8_linear_f32in and mq_w4a8_linear_f32in -- against oracle.linear_gemv_launch, a plain numpy
restatement of its fixed sequence of correctly rounded fp32 and int32 operations.  EVERY element of every case is compared on its
stored bits: no tolerance, no excluded share.  No sibling kernel is a reference.

Every operand, grid and case comes from gemv_cases.py, whose lists test_gemv_oracle.py holds to their conditions on the CPU: exact
round-half-even ties of both parities in the output quantizer and in the fused activation quantize, the values one ulp either side,
both clamps and the steps around them, NaN / +-inf / -0.0 activations, accumulators beyond 2^24 and sums that wrap in int32, zero
points at both extremes, a caller's a_rowsum that is not the image's row sum (and NULL), every output storage type on every
instantiation, and the launch geometry: weight rows that span two load passes at an odd phase (cpl = 9), cpl = 16 and 64, a wave with
all 64 row slots, the rows_per_wg clamp, fewer rows than CUs, a ragged last workgroup, the M K limit.  The geometry classes are
re-evaluated with the device's own CU count; a class that is no longer reached fails by name.

Every call goes through the C ABI on buffers this file allocates: each output is pre-filled with 0xA5 and has 64 canary bytes in front
of it and behind it, and they have to survive.  A failure names the instantiation, the first differing (m, n), its workgroup, wave,
row slot, the pass and chunk slot in which the row completed, tt, f, the value in front of the rint, got, want and the distance to a
tie.

Measured wall time of the whole file on an MI355X: 9.0 s for its 207 tests; the slowest, the packed-weight cases at 4100 x 16640
(cpl = 9) and 262152 x 256, 0.6 s each, the 156 small cases a few milliseconds.  Most of that is the numpy oracle, not the GPU.  Every
kernel matched: the pin found no defect.  Against an oracle broken on purpose (oracle.LINEAR_GEMV_MUTATION) the file failed there in
158 (one fma for the multiply and the add), 69 (f / s for f fl(1 / s)), 167 (ties rounded half up), 151 (the offset in front of the
rint), 159 (the prefill GEMM's folded form) and 60 (the image's true row sum for the caller's) of its 207 tests; the rest are the
cases those changes do not reach (no grid, no bias, a power-of-two scale, an even offset, a true row sum, the refusals)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gemm_cases as GC  # noqa: E402
import gemv_cases as C  # noqa: E402
from oracle import mq_oracle as O  # noqa: E402
from test_gpu_quantize import MQ, Buf, _inp  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32}
MQ_EINVAL, MQ_EUNSUPPORTED = 1, 3
FILL = 0xA5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    assert _lib().device_info()["arch"].startswith("gfx950")
    return torch.device("cuda:0")


def _lib():
    import mobilequant_amd._lib as L
    return L


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(b):
    return b.ptr if b is not None else None


def _cus():
    return _lib().device_info()["cu_count"]


class Operands:
    """The device operands of a problem (gemv_cases.Problem or the seam's), and the argument list of its entry point."""

    def __init__(self, dev, entry, p, M, N, K, storage):
        self.entry, self.M, self.N, self.K, self.storage = entry, M, N, K, storage
        fuse, w4 = C.ENTRIES[entry]
        self.w = _inp(dev, p.w_packed if w4 else p.w)
        self.alpha, self.zp, self.ct = _inp(dev, p.alpha), _inp(dev, p.w_zp), _inp(dev, p.col_term)
        self.bias = _inp(dev, p.bias) if p.bias is not None else None
        self.a = _inp(dev, p.x if fuse else p.a)
        self.rs = _inp(dev, p.a_rowsum) if p.a_rowsum is not None else None
        self.agrid = p.agrid
        if fuse:
            self.a_s, self.a_o = _inp(dev, np.array([p.agrid[0]], F32)), _inp(dev, np.array([p.agrid[1]], F32))
        self.out_grid = p.out_grid
        if p.out_grid is not None:
            self.o_s, self.o_o = _inp(dev, np.array([p.out_grid[0]], F32)), _inp(dev, np.array([p.out_grid[1]], F32))
        self.dtype = O.PREFILL_GEMM_STORAGE[storage]
        self.nbytes = M * N * np.dtype(self.dtype).itemsize
        self.dev = dev

    def new_out(self):
        return Buf(self.dev, self.nbytes, data=np.full(self.nbytes, FILL, np.uint8))

    def args(self, out, M=None, K=None, storage=None, grid=True):
        M, K = M or self.M, K or self.K
        g = self.out_grid if grid else None
        tail = (self.alpha.ptr, self.zp.ptr, self.ct.ptr, _ptr(self.bias), self.o_s.ptr if g else None, self.o_o.ptr if g else None,
                float(g[2]) if g else 0.0, float(g[3]) if g else 0.0, out.ptr, MQ[storage or self.storage], _stream())
        if C.ENTRIES[self.entry][0]:
            s = self.agrid
            return (self.a.ptr, self.a_s.ptr, self.a_o.ptr, float(s[2]), float(s[3]), int(s[4]), self.w.ptr, M, self.N, K) + tail
        return (self.a.ptr, self.w.ptr, M, self.N, K, _ptr(self.rs)) + tail

    def launch(self, out=None):
        out = out or self.new_out()
        _lib().call(_entry_name(self.entry), *self.args(out))
        return out

    def take(self, out, what="out"):
        return out.take(self.dtype, what).reshape(self.M, self.N)


def _entry_name(entry):
    return "mq_%s" % entry.replace("w8a8", "w8a8_linear").replace("w4a8", "w4a8_linear")


def _report(c, got, e, what="output"):
    """Exact on the stored bits; the message locates the first difference in the launch for whoever has to read the kernel."""
    want = e["stored"]
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    u = UINT[want.dtype.itemsize]
    bad = np.argwhere(got.view(u) != want.view(u))
    if len(bad) == 0:
        return
    m, n = (int(v) for v in bad[0])
    cus = _cus()
    wg, wave, slot, ps, u_ = C.locate(c, n, cus)
    mt, fuse, w4 = C.instantiation(c)
    pytest.fail("%s %s on gemv_i8_fat_kernel<MT=%d, FUSEQ=%d, W4=%d> (%s, %d CUs): %d of %d differ, first at (m %d, n %d) = token group %d, "
                "workgroup %d wave %d row slot %d, completed in pass %d chunk slot %d, column class %s: got %r want %r; tt = %d, f = %r, "
                "value in front of the rint = %r, distance to a tie %.3g"
                % (c.id, what, mt, fuse, w4, C.geometry(c, cus), cus, len(bad), got.size, m, n, m // mt, wg, wave, slot, ps, u_,
                   C.col_classes(c.N)[n], got[m, n], want[m, n], int(e["tt"][m, n]), float(e["f"][m, n]), float(e["v"][m, n]),
                   float(e["tie"][m, n])))


def _operands(dev, c):
    return Operands(dev, c.entry, C.problem(c), c.M, c.N, c.K, C.storage_of(c))


@pytest.mark.parametrize("c", C.ALL_CASES, ids=lambda c: c.id)
def test_linear_gemv(dev, c):
    """Every case of gemv_cases.py, every stored bit."""
    assert C.takes_gemv(c.M, c.K)
    ops = _operands(dev, c)
    out = ops.launch()
    torch.cuda.synchronize()
    _report(c, ops.take(out), C.expect(c))


def test_geometry_classes_are_reached_on_this_device():
    """The branch conditions of the launch depend on the CU count: re-evaluated with the device's own, every class has to be reached by
    a case, and every instantiation by a multi-pass row and a ragged last workgroup."""
    cus = _cus()
    reached = set()
    per_inst = {i: set() for i in C.INSTANTIATIONS}
    for c in C.ALL_CASES:
        k = C.geometry_classes(c, cus)
        reached |= k
        per_inst[C.instantiation(c)] |= k
    missing = [k for k in C.GEOMETRY_CLASSES if k not in reached]
    assert not missing, "on %d CUs no case of gemv_cases.py reaches: %s" % (cus, ", ".join(missing))
    for i, k in per_inst.items():
        assert {"multi_pass", "ragged_last_wg"} <= k, "on %d CUs instantiation MT=%d FUSEQ=%d W4=%d misses %s" % (
            (cus,) + i + (sorted({"multi_pass", "ragged_last_wg"} - k),))


# ---- the M = 8 / M = 9 seam and the forced variant ------------------------------------------------------------------------------
def _seam_problem(M, grid, p2):
    """The first M rows of one nine-row operand set: rows 0..7 are gemv_cases' rows of M = 8, row 8 one more low-magnitude row."""
    N, K = C.SEAM_SHAPE
    c = C._case("w8a8", 8, N, K, grid, p2=p2)
    p = C.problem(c)
    if M <= 8:
        return c, p._replace(a=p.a[:M], a_rowsum=p.a_rowsum[:M], tt=p.tt[:M])
    extra = np.random.default_rng(9).integers(-2, 2, size=(1, K), dtype=np.int8)
    a = np.concatenate([p.a, extra])
    rs = a.astype(np.int64).sum(axis=1).astype(np.int32)
    return c, p._replace(a=a, a_rowsum=rs, tt=O.prefill_gemm_acc(a, p.w, rs, p.w_zp, p.col_term))


def _gemm_expect(c, p):
    g = GC.GRIDS[c.grid]
    stored, q, tie = O.prefill_gemm_epilogue(p.tt, p.alpha, p.bias, None if g is None else [(p.out_grid[0], p.out_grid[1])], None,
                                             0 if g is None else g.qmin, 255 if g is None else g.qmax, C.storage_of(c))
    return dict(stored=stored, tt=p.tt, f=q.astype(F32), v=q, tie=tie)


@pytest.mark.parametrize("grid,p2", C.SEAM_GRIDS, ids=lambda v: str(v))
def test_seam_between_gemv_and_gemm(dev, grid, p2):
    """One operand set through mq_w8a8_linear at M = 8 (the GEMV) and at M = 9 (the MFMA GEMM), the first eight rows equal: each result
    equals its OWN oracle (linear_gemv_launch / prefill_gemm_epilogue), and without a grid rows 0..7 are bit-identical across the seam."""
    N, K = C.SEAM_SHAPE
    c8, p8 = _seam_problem(8, grid, p2)
    c9, p9 = _seam_problem(9, grid, p2)
    o8, o9 = Operands(dev, "w8a8", p8, 8, N, K, C.storage_of(c8)), Operands(dev, "w8a8", p9, 9, N, K, C.storage_of(c9))
    b8, b9 = o8.launch(), o9.launch()
    torch.cuda.synchronize()
    got8, got9 = o8.take(b8), o9.take(b9)
    _report(c8, got8, O.linear_gemv_launch(**C.oracle_args(c8, p8)), "M = 8 (GEMV form)")
    e9 = _gemm_expect(c9, p9)
    u = UINT[got9.dtype.itemsize]
    bad = np.argwhere(got9.view(u) != e9["stored"].view(u))
    assert len(bad) == 0, "M = 9 (GEMM form): %d of %d differ from prefill_gemm_epilogue, first at %s" % (len(bad), got9.size, bad[0])
    if GC.GRIDS[grid] is None:
        assert np.array_equal(got8.view(u), got9[:8].view(u)), "without a grid the two forms are the same two roundings"


@pytest.mark.parametrize("grid,p2", (("u8", False), ("u16", False), ("none32", False)), ids=lambda v: str(v))
def test_forced_variant_sends_decode_shapes_to_the_gemm(dev, grid, p2):
    """mq_gemm_set_variant(v >= 0) turns the GEMV dispatch off: M = 8 then stores the prefill GEMM's folded form."""
    N, K = C.SEAM_SHAPE
    c, p = _seam_problem(8, grid, p2)
    ops = Operands(dev, "w8a8", p, 8, N, K, C.storage_of(c))
    lib = _lib().load()
    try:
        lib.mq_gemm_set_variant(8)
        out = ops.launch()
        torch.cuda.synchronize()
    finally:
        lib.mq_gemm_set_variant(-1)
    got, e = ops.take(out), _gemm_expect(c, p)
    u = UINT[got.dtype.itemsize]
    bad = np.argwhere(got.view(u) != e["stored"].view(u))
    assert len(bad) == 0, "forced variant 8 at M = 8: %d of %d differ from prefill_gemm_epilogue, first at %s" % (len(bad), got.size, bad[0])


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def _refused(ops, out, rc_want, **kw):
    lib = _lib().load()
    name = _entry_name(ops.entry)
    rc = getattr(lib, name)(*ops.args(out, **kw))
    torch.cuda.synchronize()
    msg = lib.mq_last_error().decode()
    assert rc == rc_want, (name, rc, msg)
    assert name in msg, (name, msg)
    assert np.all(out.take(np.uint8, "out of a refused call") == FILL), "%s wrote its output before refusing" % name


@pytest.mark.parametrize("entry", list(C.ENTRIES))
def test_integer_storage_without_a_grid_is_refused(dev, entry):
    c = C._case(entry, 2, 180, 256, "u8")
    ops = _operands(dev, c)
    for st in ("u8", "i8", "u16", "i16"):
        _refused(ops, ops.new_out(), MQ_EINVAL, storage=st, grid=False)


@pytest.mark.parametrize("entry", ["w8a8_f32in", "w4a8_f32in"])
def test_f32in_refuses_what_is_no_decode_shape(dev, entry):
    """M = 9, K % 256 != 0 and M K over the staging limit: MQ_EUNSUPPORTED, nothing written.  The operands are allocated at the largest
    shape asked for, so that a launch that went ahead would still stay inside them."""
    big_m, big_k = 9, 9472
    rng = np.random.default_rng(3)
    N = 180
    w4 = C.ENTRIES[entry][1]
    w = rng.integers(0, 16, size=(N, big_k), dtype=np.int8) if w4 else rng.integers(-128, 128, size=(N, big_k), dtype=np.int8)
    p = C.Problem(None, None, rng.standard_normal((big_m, big_k)).astype(F32), C.A_GRIDS["u8"], None, None, w, O.pack_w4(w, 0) if w4 else None,
                  np.zeros(N, np.int32), np.zeros(N, np.int32), np.ones(N, F32), None, (F32(0.05), F32(128.0), 0.0, 255.0), None)
    ops = Operands(dev, entry, p, big_m, N, big_k, "u8")
    for M, K in ((9, 256), (2, 384), (7, 9472), (8, 8192)):
        assert not C.f32in_accepts(M, K)
        _refused(ops, ops.new_out(), MQ_EUNSUPPORTED, M=M, K=K)


@pytest.mark.parametrize("w4", [False, True], ids=["w8", "w4"])
def test_first_shape_over_the_limit_goes_to_the_gemm(dev, w4):
    """M K one step over the staging limit (M = 8, K = 8192) is served by the GEMM from the int8 entries: the folded form."""
    M, K = C.OVER_LIMIT[1]
    assert not C.takes_gemv(M, K) and C.takes_gemv(M, K - 128)
    c = C._case("w4a8" if w4 else "w8a8", M, 180, K, "u8")
    p = C.problem(c)
    ops = Operands(dev, c.entry, p, M, c.N, K, "u8")
    out = ops.launch()
    torch.cuda.synchronize()
    got, e = ops.take(out), _gemm_expect(c, p)
    bad = np.argwhere(got != e["stored"])
    assert len(bad) == 0, "%s: %d of %d differ from prefill_gemm_epilogue, first at %s" % (c.id, len(bad), got.size, bad[0])


# ---- reproducibility and graph capture ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [C.MULTI_PASS_CASES[2], C.MULTI_PASS_CASES[5]], ids=lambda c: c.id)
def test_two_launches_give_the_same_bits(dev, c):
    ops = _operands(dev, c)
    a, b = ops.launch(), ops.launch()
    torch.cuda.synchronize()
    ga, gb = ops.take(a), ops.take(b)
    u = UINT[ga.dtype.itemsize]
    assert np.array_equal(ga.view(u), gb.view(u))
    _report(c, ga, C.expect(c))


def test_captured_launch_gives_the_bits_of_the_plain_launch(dev):
    """One small case, one stream, no parallel branches."""
    c = C._case("w8a8_f32in", 5, 580, 256, "u8", agrid="u8")
    ops = _operands(dev, c)
    plain = ops.launch()
    torch.cuda.synchronize()
    want = ops.take(plain)
    out = ops.new_out()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.launch(out)
    graph.replay()
    torch.cuda.synchronize()
    got = ops.take(out, "captured out")
    assert np.array_equal(got, want)
    _report(c, got, C.expect(c), "captured launch")
