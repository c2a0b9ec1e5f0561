"""GPU: the training passes of csrc/mq_fake_quant.hip -- mq_fake_quant_backward (scalar, vector and per-row kernels), mq_lwc_fake_quant and its
backward, mq_attention_probs_train and its backward -- against the numpy oracles (oracle.mq_oracle fake_quant_backward_terms, lwc_fused_*,
train_attn_probs*) at every dispatch branch, on every grid-stride / row-loop trip, in the FAST and the !FAST body.  No sibling kernel and no
torch GPU op is a reference.  Every case, grid, designed gradient and add count comes from train_cases.py, which test_train_oracle.py holds
to the launch code, to the undecided cap and to the sensitivity condition on the CPU.

Exact (== with NaN a NaN; zeros by ==): grad_x of all three fake-quant backward kernels; the LWC forward's values, row_min, row_max, scale,
offset; LWC grad_w at every element that is no row extreme (and at the extremes of a row whose range gradient the CLIPMIN / CLIPMAX clamp
blocks); the attention probabilities at every element that is not undecided, exact 0 at -inf-masked positions and in grad_raw wherever Q1
clamps, all-NaN rows.  An UNDECIDED probability (t2 within its envelope of a half-integer; at most 1 % of a case, none at a clamp edge)
may be either neighbouring grid value and nothing else.
Bounded, against the float64 value: every sum -- grad_scale / grad_offset, LWC grad_sig_lo / grad_sig_hi and the scatter into the extreme
elements, the four attention grid gradients -- by gamma_n * sum|term| (n from the launch geometry), plus the propagated envelope for the
attention backward (oracle.train_attn_probs_backward; it rests on the ASSUMED oracle.EXPF_ULP = 1, the documented figure); grad_raw by its
per-element envelope.  No bar is fitted to a kernel.  Worst observed got / bound on an MI355X (printed at the end of the module):
mq_fake_quant_backward 0.24, mq_lwc_fake_quant_backward 0.19, attention grid gradients 0.15, grad_raw 0.61; 1723 undecided probabilities
over the file, 20 of them on the farther grid value.

Every call goes through ops._lib.call on buffers this file allocates, inputs included; every output and gradient slot sits between 64
canary bytes (gpu_buffers.py), pointer offsets included, and inputs have to come back unchanged.

Measured wall time of the whole file on an MI355X: 7.3 s for its 223 tests (the slowest, the 10.5 M-element vector sweep -- 126 MB of x,
grad_y and grad_x, the oracle's terms formed once --, 1.9 s; the 4099 x 516 attention trips 0.4 s each; everything else under 0.2 s)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import train_cases as T  # noqa: E402
from gpu_buffers import Buf, _bits  # noqa: E402
from oracle import mq_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
WORST = {"fake_quant_backward": 0.0, "lwc_backward": 0.0, "attention_grad_raw": 0.0, "attention_grid_gradients": 0.0}
SEEN = {"undecided": 0, "undecided_alt": 0}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    import mobilequant_amd._lib as L
    assert L.device_info()["arch"].startswith("gfx950")
    yield torch.device("cuda:0")
    print("\ntest_gpu_train worst observed got / bound: %r; undecided probabilities: %r" % (WORST, SEEN))


def _call(name, *args):
    from mobilequant_amd import ops
    ops._lib.call(name, *args)
    torch.cuda.synchronize()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _inp(dev, a, off=0):
    a = np.ascontiguousarray(a)
    return Buf(dev, a.nbytes, off, a)


def _unchanged(buf, a, what):
    assert np.array_equal(buf.take(np.uint8, what), np.ascontiguousarray(a).view(np.uint8).reshape(-1)), "%s was written" % what


def check_exact(got, want, x, what, where=None):
    """== (NaN exactly where the oracle has one; +0 == -0) at every element of `where`; names the first differing (row, column)."""
    got, want = np.atleast_2d(got), np.atleast_2d(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    with np.errstate(invalid="ignore"):
        ok = (np.isnan(got) & np.isnan(want)) | (got == want)
    if where is not None:
        ok = ok | ~np.atleast_2d(where)
    bad = np.argwhere(~ok)
    if len(bad):
        r, c = (int(v) for v in bad[0])
        xv = F32(np.atleast_2d(x)[r, c]) if x is not None else F32(0)
        pytest.fail("%s: %d of %d differ, first at (row %d, col %d): got %r (%s) want %r, input %r (%s)"
                    % (what, len(bad), got.size, r, c, float(got[r, c]), _bits(F32(got[r, c])), float(want[r, c]), float(xv), _bits(xv)))


def check_bounded(got, want, bar, what, key, where=None):
    """|got - want| <= bar elementwise (want float64); NaN where the oracle has NaN; bar 0 is ==.  Records the worst got / bound."""
    got, want, bar = (np.atleast_1d(np.asarray(v, F64)).reshape(-1) for v in (got, want, bar))
    held = np.ones(got.shape, bool) if where is None else np.asarray(where).reshape(-1)
    with np.errstate(invalid="ignore"):
        err = np.abs(got - want)
        ok = (np.isnan(want) & np.isnan(got)) | (err <= bar) | ~held
        ratio = np.where(held & (bar > 0) & np.isfinite(err), err / np.where(bar > 0, bar, 1.0), 0.0)
    bad = np.flatnonzero(~ok)
    if len(bad):
        i = int(bad[0])
        pytest.fail("%s: %d of %d outside the bound, first at %d: got %r want %r, off by %.3e, bound %.3e"
                    % (what, len(bad), got.size, i, got[i], want[i], err[i], bar[i]))
    WORST[key] = max(WORST[key], float(ratio.max()) if ratio.size else 0.0)


# ---- mq_fake_quant_backward -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.FQB_CASES, ids=lambda c: c.name)
def test_fake_quant_backward_every_kernel_trip_and_grid(dev, case):
    """grad_x bit for bit, grad_scale and grad_offset within gamma_n * sum|term| of the float64 sums of the oracle's fp32 terms (NaN where a
    term is NaN: a NaN or an infinity in x), in the scalar kernel (small, misaligned by one pointer in turn, numel % 4 != 0, nine
    grid-stride trips behind the 512-workgroup cap), the vector kernel (every unroll slot full, slot 3 partly filled, a second sweep behind
    the 2048-workgroup cap) and the per-row kernel (1 .. 1000 columns, 4099 rows); rows == n_scale == 1 takes the per-tensor path."""
    d, e = T.fqb_inputs(case), T.fqb_expect(case)
    what = "mq_fake_quant_backward %s (%s kernel, %r)" % (case.name, T.fqb_kernel(case.rows, case.cols, case.n_scale, case.offs), case.grid)
    n_s = d["n_group"]
    xb, gb = _inp(dev, d["x"], case.offs[0]), _inp(dev, d["g"], case.offs[1])
    ob = Buf(dev, d["x"].nbytes, case.offs[2])
    sb, fb = _inp(dev, d["scale"]), _inp(dev, d["offset"])
    gs, go = Buf(dev, 4 * n_s, fill=F32(0)), Buf(dev, 4 * n_s, fill=F32(0))
    _call("mq_fake_quant_backward", xb.ptr, gb.ptr, case.rows, case.cols, sb.ptr, fb.ptr, n_s, float(d["qmin"]), float(d["qmax"]), ob.ptr, gs.ptr,
          go.ptr, _stream())
    gx = ob.take(F32, "grad_x").reshape(case.rows, case.cols)
    check_exact(gx, e["gx"], d["x"], what + " grad_x")
    check_bounded(gs.take(F32, "grad_scale"), e["sum_ts"], e["bar_ts"], what + " grad_scale (n = %d)" % e["n"], "fake_quant_backward")
    check_bounded(go.take(F32, "grad_offset"), e["sum_to"], e["bar_to"], what + " grad_offset (n = %d)" % e["n"], "fake_quant_backward")
    _unchanged(xb, d["x"], "x")
    _unchanged(gb, d["g"], "grad_y")
    _unchanged(sb, d["scale"], "scale")
    _unchanged(fb, d["offset"], "offset")


# ---- mq_lwc_fake_quant(_backward) -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,sym", T.LWC_GRIDS)
@pytest.mark.parametrize("cols", T.LWC_COLS)
def test_lwc_fused_pass_forward_exact_and_backward(dev, cols, bits, sym):
    """1, 5 and 33 rows of `cols` columns (both sides of every VPT boundary, VPT = 8 included): out, row_min, row_max, scale, offset exact;
    grad_w exact off the extremes and within the bound on them; grad_sig_lo / grad_sig_hi within gamma_n |c| sum|term|.  Unique extremes
    walk through every (wave, k) and the vectors around every 1024 k; ties, a constant row, an all-zero row, -0.0 as the minimum, a NaN
    row and a +inf row included."""
    for rows in T.LWC_ROWS:
        d = T.lwc_inputs(cols, bits, sym, rows)
        what = "mq_lwc_fake_quant %d x %d, %d bit %s" % (rows, cols, bits, "symmetric" if sym else "asymmetric")
        w, f = d["w"], d["fwd"]
        wb, lb, hb = _inp(dev, w), _inp(dev, d["sig_lo"]), _inp(dev, d["sig_hi"])
        ob = Buf(dev, w.nbytes)
        stat = [Buf(dev, 4 * rows) for _ in range(4)]
        _call("mq_lwc_fake_quant", wb.ptr, rows, cols, lb.ptr, hb.ptr, bits, int(sym), ob.ptr, stat[0].ptr, stat[1].ptr, stat[2].ptr, stat[3].ptr,
              _stream())
        got = {k: b.take(F32, k) for k, b in zip(("row_min", "row_max", "scale", "offset"), stat)}
        for k in got:
            check_exact(got[k], f[k], None, "%s %s (row kinds %r)" % (what, k, d["kinds"]))
        check_exact(ob.take(F32, "out").reshape(rows, cols), f["y"], w, what + " out")
        b = O.lwc_fused_backward(w, d["g"], d["sig_lo"], d["sig_hi"], f["row_min"], f["row_max"], bits, sym)
        gb, mnb, mxb = _inp(dev, d["g"]), _inp(dev, got["row_min"]), _inp(dev, got["row_max"])
        gwb, glo, ghi = Buf(dev, w.nbytes), Buf(dev, 4 * rows), Buf(dev, 4 * rows)
        _call("mq_lwc_fake_quant_backward", wb.ptr, gb.ptr, rows, cols, lb.ptr, hb.ptr, mnb.ptr, mxb.ptr, bits, int(sym), gwb.ptr, glo.ptr, ghi.ptr,
              _stream())
        gw = gwb.take(F32, "grad_w").reshape(rows, cols)
        n = T.lwc_n(cols)
        check_exact(gw, b["gx"], w, what + " grad_w off the row extremes", where=~b["extreme"])
        with np.errstate(invalid="ignore"):
            bar_w = np.where(b["c_scat"] > 0, T.gamma(n + 8) * (np.abs(b["gx"]) + b["c_scat"] * b["sumabs"][:, None]), 0.0)
        check_bounded(gw, b["grad_w"], bar_w, what + " grad_w on the row extremes", "lwc_backward", where=b["extreme"])
        for name, buf, c in (("grad_sig_lo", glo, b["c_sig_lo"]), ("grad_sig_hi", ghi, b["c_sig_hi"])):
            with np.errstate(invalid="ignore"):
                bar = np.where(c > 0, T.gamma(n + 6) * c * b["sumabs"], 0.0)
            check_bounded(buf.take(F32, name), b[name], bar, "%s %s (row kinds %r)" % (what, name, d["kinds"]), "lwc_backward")
        _unchanged(wb, w, "w")
        _unchanged(gb, d["g"], "grad_out")


# ---- mq_attention_probs_train(_backward) ----------------------------------------------------------------------------------------------------
def _attn_args(dev, d):
    g1, g2 = d["grid1"], d["grid2"]
    grids = [_inp(dev, np.array([v], F32)) for v in (g1[0], g1[1], g2[0], g2[1])]
    mb = _inp(dev, d["mask"]) if d["mask"] is not None else None
    return grids, mb, (float(g1[2]), float(g1[3])), (float(g2[2]), float(g2[3]))


@pytest.mark.parametrize("case", T.ATTN_CASES, ids=lambda c: c.name)
def test_attention_probs_train_forward(dev, case):
    """Q2(softmax(Q1(raw) / sqrt_d + mask)): every decided element equals the oracle's grid value, an undecided one is one of the two
    neighbouring grid values, -inf-masked positions are exactly 0, a fully masked row is NaN throughout -- on every VPT edge, with a
    partial last group of four rows, past 32768 rows (a second trip of the row loop), without a mask, with mask_rows == rows, with
    row % mask_rows wrapping and under the causal -inf mask, with sqrt_d a power of two (FAST) and not, and with s1 = 2^61 (!FAST by scale)."""
    d = T.attn_inputs(case)
    f, raw = d["fwd"], d["raw"]
    what = "mq_attention_probs_train %s (FAST %d, %r)" % (case.name, T.attn_fast(d["grid1"][0], d["grid2"][0], case.sqrt_d), T.attn_fwd_geom(case.rows, case.cols))
    grids, mb, l1, l2 = _attn_args(dev, d)
    rb, ob = _inp(dev, raw), Buf(dev, raw.nbytes)
    _call("mq_attention_probs_train", rb.ptr, case.rows, case.cols, mb.ptr if mb else None, case.mask_rows if mb else 1, grids[0].ptr, grids[1].ptr,
          l1[0], l1[1], grids[2].ptr, grids[3].ptr, l2[0], l2[1], float(case.sqrt_d), ob.ptr, _stream())
    got = ob.take(F32, "out").reshape(case.rows, case.cols)
    und = f["undecided"] & ~f["nan_row"][:, None]
    check_exact(got, f["out"], raw, what + " decided probabilities", where=~und)
    alt = und & (got != f["out"])
    check_exact(got, f["out_alt"], raw, what + " undecided probabilities that are not the nearer grid value", where=alt)
    assert np.all(got[f["masked"] & ~f["nan_row"][:, None]] == 0)
    SEEN["undecided"] += int(und.sum())
    SEEN["undecided_alt"] += int(alt.sum())
    _unchanged(rb, raw, "raw")


@pytest.mark.parametrize("case", T.ATTN_CASES, ids=lambda c: c.name)
def test_attention_probs_train_backward(dev, case):
    """grad_raw within its envelope of the float64 chain, exactly 0 wherever Q1 clamps, NaN in a NaN row; the four grid gradients within
    gamma_n sum|term| + the propagated envelope (NaN where a NaN row reaches them) -- both row layouts on every VPT edge, a third trip of
    the wave-per-row loop and of the workgroup-per-row loop (the LDS slot of trip 0 reused, dead workgroups on the last trip)."""
    d = T.attn_inputs(case)
    b, raw, gy = d["bwd"], d["raw"], d["gy"]
    ge = T.attn_bwd_geom(case.rows, case.cols)
    what = "mq_attention_probs_train_backward %s (FAST %d, %r)" % (case.name, T.attn_fast(d["grid1"][0], d["grid2"][0], case.sqrt_d), ge)
    grids, mb, l1, l2 = _attn_args(dev, d)
    rb, gb = _inp(dev, raw), _inp(dev, gy)
    ob, gg = Buf(dev, raw.nbytes), Buf(dev, 16, fill=F32(0))
    _call("mq_attention_probs_train_backward", rb.ptr, gb.ptr, case.rows, case.cols, mb.ptr if mb else None, case.mask_rows if mb else 1,
          grids[0].ptr, grids[1].ptr, l1[0], l1[1], grids[2].ptr, grids[3].ptr, l2[0], l2[1], float(case.sqrt_d), ob.ptr, gg.ptr, _stream())
    got = ob.take(F32, "grad_raw").reshape(case.rows, case.cols)
    in1 = b["fwd"]["in1"]
    check_exact(got, np.zeros_like(got), raw, what + " grad_raw where Q1 clamps", where=~in1)
    check_bounded(got, b["grad_raw"], b["e_raw"], what + " grad_raw", "attention_grad_raw", where=in1)
    vals, bars = T.attn_bwd_sums(case, d)
    ggot = gg.take(F32, "grad_grids")
    for i, name in enumerate(("d s1", "d o1", "d s2", "d o2")):
        check_bounded(ggot[i], vals[i], bars[i], "%s %s (n = %d)" % (what, name, ge.n_grid), "attention_grid_gradients")
    _unchanged(rb, raw, "raw")
    _unchanged(gb, gy, "grad_out")
