"""GPU: the fused epilogues of the prefill GEMM family -- gemm_i8_kernel in every variant (csrc/mq_gemm.hip) and the generated programs
of tools/gen_fr_asm.py (fr, the pair launches, fr128, fr160, fr128r, fr128r8, frg, frw4x, frw4x_128r, frgw4x, 176 and 128 columns
wide) -- against oracle.prefill_gemm_epilogue, a plain numpy restatement of their fixed sequence of correctly rounded fp32 operations.
EVERY element of every real row is compared on its stored bits: no tolerance, no excluded share.  No sibling kernel is a reference.

Every operand, grid and case comes from gemm_cases.py, whose lists test_gemm_oracle.py holds to their conditions on the CPU: exact
round-half-even ties of both parities, both clamps and the steps around them, accumulators beyond 2^24, zero points at +-255, column
segments off every tile boundary, shapes with ragged M and every tail.  Every call goes through the C ABI on buffers this file
allocates: each output (indices, fp32 / fp16 values, idx_scratch, the fragment-blocked image [ceil16(M), N], row_sum) has 64 canary
bytes in front of it and behind it, and they have to survive; the gated pair's outputs are pre-filled with a pattern, row_sum with
non-zero garbage the first launch has to clear.  A failure names the kernel the dispatch predicate expects, the first differing
(row, column), its tile and lane, t, A', B', got, want and the oracle's distance to a tie.

Measured wall time of the whole file on an MI355X: 12.3 s for its 92 tests (91 run, the split-K case skips in a production build);
the slowest, a gated pair at 1793 x 4224 x 768 (7.6 M outputs per linear), 0.8 s, every small case below 0.1 s.  Most of that is the
numpy oracle, not the GPU.  Every kernel matched.  Against an oracle broken on purpose 78 of the 91 running tests failed
there (a multiply and an add for the fma) and 86 (ties rounded half up): all but the cases without a grid or without a bias."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gemm_cases as C  # noqa: E402
from oracle import mq_oracle as O  # noqa: E402
from test_gpu_quantize import MQ, Buf, _inp  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32}
HOOK_RESET = {C.SEG_TILE: 0, C.RES_TILE: 0, C.PAIR_MODE: 0}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    import mobilequant_amd._lib as L
    assert L.device_info()["arch"].startswith("gfx950")
    return torch.device("cuda:0")


def _lib():
    import mobilequant_amd._lib as L
    return L


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(b):
    return b.ptr if b is not None else None


class Linear:
    """The device operands of one linear of a case: weights (int8 or mq_pack_w4's image), epilogue vectors, its output grids."""

    def __init__(self, dev, c, p):
        self.w = _inp(dev, O.pack_w4(p.w, 0) if c.w4 else p.w.astype(np.int8))
        self.alpha, self.zp, self.ct = _inp(dev, p.alpha), _inp(dev, p.w_zp), _inp(dev, p.col_term)
        self.bias = _inp(dev, p.bias) if p.bias is not None else None
        g = C.GRIDS[c.grid]
        self.qmin, self.qmax = (0.0, 0.0) if g is None else (float(g.qmin), float(g.qmax))
        self.grids = [(_inp(dev, np.array([s], F32)), _inp(dev, np.array([o], F32))) for s, o in (p.grids or [])]
        self.n_seg = len(self.grids)
        self.seg_end = (ctypes.c_int64 * max(1, self.n_seg))(*(p.seg_end or [c.N]))
        self.mq_grids = (_lib().MqGrid * max(1, self.n_seg))(*[_lib().MqGrid(s.ptr, o.ptr, self.qmin, self.qmax) for s, o in self.grids])
        self.so, self.oo = (self.grids[0][0].ptr, self.grids[0][1].ptr) if self.grids else (None, None)

    def vectors(self):
        return self.alpha.ptr, self.zp.ptr, self.ct.ptr, _ptr(self.bias)


def _activation(dev, p, tiled):
    M, K = p.a.shape
    a = _inp(dev, O.tiled_image_bytes(p.a, M, K)[0] if tiled else p.a)
    return a, (_inp(dev, p.a_rowsum) if p.a_rowsum is not None else None)


def _report(c, kernel, tile, which, got, want, e, p, what):
    """Exact on the stored bits; the message locates the first difference for whoever has to read the kernel."""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    u = UINT[want.dtype.itemsize]
    bad = np.argwhere(got.view(u) != want.view(u))
    if len(bad) == 0:
        return
    r, n = (int(v) for v in bad[0])
    bm, bn = tile
    pytest.fail("%s %s (linear %d) on %s: %d of %d differ, first at (row %d, col %d) = tile (%d, %d) row %d col %d of it, lane %d element %d, "
                "column class %s: got %r want %r; t = %d, A' = %r, B' = %r, q = %r, distance to a tie %.3g"
                % (c.id, what, which, kernel, len(bad), got.size, r, n, r // bm, n // bn, r % bm, n % bn, (r % 16) + 16 * ((n % 16) // 4), n % 4,
                   C.col_classes(c.N)[n], got[r, n], want[r, n], int(p.t[r, n]), float(e.a1[n]), float(e.b1[n]), float(e.q[r, n]),
                   float(e.tie[r, n])))


def _run_single(dev, c):
    """One launch of a one-linear entry point -> the [M, N] storage array."""
    p = C.problem(c)
    M, N, K = c.M, c.N, c.K
    st = C.storage_of(c)
    tiled = c.entry.startswith("tiled")
    a, rs = _activation(dev, p, tiled)
    lin = Linear(dev, c, p)
    out = Buf(dev, M * N * np.dtype(O.PREFILL_GEMM_STORAGE[st]).itemsize)
    resid = _inp(dev, p.resid) if p.resid is not None else None
    head = (a.ptr, lin.w.ptr, M, N, K, _ptr(rs)) + lin.vectors()
    call = _lib().call
    w = "w4a8" if c.w4 else "w8a8"
    if c.entry == "linear":
        call("mq_%s_linear" % w, *head, lin.so, lin.oo, lin.qmin, lin.qmax, out.ptr, MQ[st], _stream())
    elif c.entry == "tiled":
        call("mq_w8a8_linear_tiled", *head, lin.so, lin.oo, lin.qmin, lin.qmax, out.ptr, MQ[st], _stream())
    elif c.entry == "linear_residual":
        call("mq_w8a8_linear_residual", *head, lin.so, lin.oo, lin.qmin, lin.qmax, resid.ptr, out.ptr, _stream())
    elif c.entry == "tiled_residual":
        call("mq_%s_linear_tiled_residual" % w, *head, lin.so, lin.oo, lin.qmin, lin.qmax, resid.ptr, out.ptr, _stream())
    elif c.entry == "segmented":
        call("mq_%s_linear_segmented" % w, *head, lin.n_seg, lin.seg_end, lin.mq_grids, out.ptr, _stream())
    elif c.entry == "tiled_segmented":
        call("mq_w8a8_linear_tiled_segmented", *head, lin.n_seg, lin.seg_end, lin.mq_grids, out.ptr, _stream())
    elif c.entry == "tiled_w4":
        call("mq_w4a8_linear_tiled", *head, lin.n_seg, lin.seg_end if c.segs else None, lin.mq_grids, out.ptr, MQ[st], _stream())
    else:
        raise ValueError(c.entry)
    torch.cuda.synchronize()
    return out.take(O.PREFILL_GEMM_STORAGE[st], "out").reshape(M, N)


class hooks:
    """The process-wide tuning hooks of a case, reset whatever happens.  Split-K residual tiles exist in experiment builds only."""

    def __init__(self, c):
        self.c = c

    def __enter__(self):
        lib, c = _lib().load(), self.c
        if c.hook and c.hook == (C.RES_TILE, 512):
            if lib.mq_gemm_set_residual_tile(512) != 0:
                lib.mq_gemm_set_residual_tile(0)
                pytest.skip("split-K residual tiles are compiled with `python -m mobilequant_amd.build --experiments` only")
        elif c.hook:
            getattr(lib, c.hook[0])(c.hook[1])
        lib.mq_gemm_set_variant(c.variant)

    def __exit__(self, *exc):
        lib = _lib().load()
        lib.mq_gemm_set_variant(-1)
        for name, v in HOOK_RESET.items():
            getattr(lib, name)(v)
        return False


SINGLE = [c for c in C.ALL_CASES if c.entry not in ("pair", "gated")]


@pytest.mark.parametrize("c", SINGLE, ids=lambda c: c.id)
def test_linear_epilogue(dev, c):
    """Every one-linear entry point: the row-major C++ kernel in each forced variant with int8 and packed weights and every output type,
    mq_w8a8_linear_residual, the segmented entry points, and the generated kernels behind mq_w8a8_linear_tiled (fr, pp_asm with the C++
    epilogue, fr128), _tiled_segmented (fr128 / fr160), _tiled_residual (fr128r / fr128r8 / frw4x_128r) and mq_w4a8_linear_tiled."""
    (kernel, tile), = C.kernels_of(c)
    assert kernel is not None
    with hooks(c):
        got = _run_single(dev, c)
    e = C.expect(c)
    _report(c, kernel, tile, 0, got, e.stored, e, C.problem(c), "output")


@pytest.mark.parametrize("c", [c for c in C.ALL_CASES if c.entry == "pair"], ids=lambda c: c.id)
def test_pair_epilogue(dev, c):
    """mq_w8a8_linear_tiled_pair in both mq_gemm_set_pair_mode settings: two linears over one activation image, each against its own
    oracle."""
    (kernel, tile), = C.kernels_of(c)
    M, N, K = c.M, c.N, c.K
    p = [C.problem(c, 0), C.problem(c, 1)]
    a, rs = _activation(dev, p[0], True)
    lin = [Linear(dev, c, q) for q in p]
    out = [Buf(dev, M * N, data=np.full(M * N, 0xA5, np.uint8)) for _ in range(2)]
    st = C.storage_of(c)
    args = []
    for i in range(2):
        args += [lin[i].w.ptr, *lin[i].vectors(), lin[i].so, lin[i].oo, out[i].ptr]
    with hooks(c):
        _lib().call("mq_w8a8_linear_tiled_pair", a.ptr, M, N, K, _ptr(rs), *args, MQ[st], _stream())
        torch.cuda.synchronize()
    for i in range(2):
        e = C.expect(c, i)
        _report(c, kernel, tile, i, out[i].take(O.PREFILL_GEMM_STORAGE[st], "out%d" % i).reshape(M, N), e.stored, e, p[i], "output")


@pytest.mark.parametrize("c", [c for c in C.ALL_CASES if c.entry == "gated"], ids=lambda c: c.id)
def test_gated_pair_epilogue(dev, c):
    """mq_w8a8 / mq_w4a8_linear_tiled_gated, wide and narrow: w1's indices in idx_scratch, w2's input image through the layout formula
    (all M N bytes of the real rows) and its row sums, which the FIRST launch has to clear: row_sum starts as non-zero garbage."""
    (k0, tile), (k1, _) = C.kernels_of(c)
    M, N, K = c.M, c.N, c.K
    mp = (M + 15) // 16 * 16
    p = [C.problem(c, 0), C.problem(c, 1)]
    a, rs = _activation(dev, p[0], True)
    lin = [Linear(dev, c, q) for q in p]
    table = _inp(dev, C.gate_table())
    rng = np.random.default_rng(1)
    idx = Buf(dev, M * N, data=np.full(M * N, 0xA5, np.uint8))
    img = Buf(dev, mp * N, data=np.full(mp * N, 0x5A, np.uint8))
    rsum = Buf(dev, M * 4, data=(rng.integers(1, 1 << 30, M) * np.where(np.arange(M) & 1, 1, -1)).astype(np.int32))
    args = []
    for i in range(2):
        args += [lin[i].w.ptr, *lin[i].vectors(), lin[i].so, lin[i].oo]
    with hooks(c):
        _lib().call("mq_%s_linear_tiled_gated" % ("w4a8" if c.w4 else "w8a8"), a.ptr, M, N, K, _ptr(rs), *args, table.ptr, idx.ptr, img.ptr,
                    rsum.ptr, _stream())
        torch.cuda.synchronize()
    e0, e1 = C.expect(c, 0), C.expect(c, 1)
    _report(c, k0, tile, 0, idx.take(np.uint8, "idx_scratch").reshape(M, N), e0.stored, e0, p[0], "idx_scratch")
    want_img, (want, real), want_rs = O.prefill_gemm_gated(e0.stored, e1.stored, C.gate_table())
    got = img.take(np.int8, "q_tiled")
    r, n = np.meshgrid(np.arange(M, dtype=np.int64), np.arange(N, dtype=np.int64), indexing="ij")
    got_img = got[O.tiled_offset(r, n, N)]                          # back through the layout formula: [M, N]
    assert int(real.sum()) == M * N
    _report(c, k1, tile, 1, got_img, want_img, e1, p[1], "image (table[ia * 256 + ib], ia from idx_scratch)")
    got_rs = rsum.take(np.int32, "row_sum")
    bad = np.flatnonzero(got_rs != want_rs)
    assert len(bad) == 0, "%s on %s: row_sum differs in %d rows, first row %d: got %d want %d" % (
        c.id, k1, len(bad), bad[0], got_rs[bad[0]], want_rs[bad[0]])
