"""The pointer contract of mobilequant_amd/ops.py, one table for its public wrappers: what every tensor operand has to be (dtype, element
count, converted by the wrapper or handed to the C entry as a raw pointer), a small valid call per branch of the wrapper that picks
another C entry or argument form, and the oracle of that call's result -- the function and the exactness class of the entry's own pin
(quantize_cases / gemm_cases / train_cases / prefill_elementwise_cases over oracle.mq_oracle; no tolerance is invented here).

test_ops_contract_host.py holds the table to ops.py on the CPU (names, signatures, operand paths, element counts of the built calls);
test_gpu_ops_contract.py makes the calls: the result against the oracle, the same bits from every layout / dtype a converted operand
may arrive in, and -- with _lib.call replaced by a recorder -- a refusal for every malformed operand with nothing launched.

Everything here is numpy: a call's arguments are arrays (tensors-to-be), tuples / dicts / lists of them, and plain scalars; DEVICE stands
for the device.  An operand is addressed by its path into the arguments: ("scale",), ("in_grid", 0), ("first", "alpha")."""
import os
import sys
from collections import namedtuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import calib_cases as K  # noqa: E402
import gemm_cases as G  # noqa: E402
import gemv_cases as V  # noqa: E402
import hist_ref as H  # noqa: E402
import lwc_search_ref as LS  # noqa: E402
import grouped_gemm_cases as GG  # noqa: E402
import qmatmul_cases as QM  # noqa: E402
import prefill_elementwise_cases as P  # noqa: E402
import quantize_cases as Q  # noqa: E402
import train_cases as T  # noqa: E402
from oracle import mq_oracle as O  # noqa: E402

F32, F16 = np.float32, np.float16
DEVICE = "<device>"
NP = {"f32": np.float32, "f16": np.float16, "i8": np.int8, "u8": np.uint8, "i16": np.int16, "u16": np.uint16, "i32": np.int32, "i64": np.int64,
      "f64": np.float64}                                                            # the dtype names of the operand table
MQ = {"f32": 0, "f16": 1, "i8": 2, "u8": 3, "i16": 4, "u16": 5, "i32": 6}          # mq_dtype (include/mobilequant_amd.h)

# ---- operands -------------------------------------------------------------------------------------------------------------------
# kind:  "conv"    read as float32: the wrapper converts any floating dtype and any layout, and keeps its copy alive over the launch
#        "layout"  any layout (the wrapper makes it contiguous), the dtype is the operand's own and one of `dtype`
#        "raw"     the pointer goes to the entry as it is: dtype, contiguity and element count are checked, nothing is copied
#        "inplace" raw, and written by the launch (a running statistic)
#        "out"     raw, the caller's output buffer
# numel: an expression over the call's sizes; None where the operand itself defines a size (nothing to be short of).
# label: the name the refusal message carries (a regular expression: an older message may name the operand in words).  align16: the entry documents 16-byte alignment (no misaligned form in part b).
Operand = namedtuple("Operand", "path kind dtype numel label align16")


def op(path, kind, dtype, numel, label=None, align16=False):
    path = (path,) if isinstance(path, str) else tuple(path)
    return Operand(path, kind, (dtype,) if isinstance(dtype, str) else tuple(dtype), numel, label or str(path[-1]), align16)


def grid_ops(param, s_label="scale", o_label="offset"):
    """A per-tensor grid tuple (scale, offset, qmin, qmax): both tensors converted, one element each."""
    return [op((param, 0), "conv", "f32", "1", s_label), op((param, 1), "conv", "f32", "1", o_label)]


def grid_pairs(w):
    """(scale path, offset path) of every grid among a wrapper's operands: element 0 and 1 of a grid tuple, or `*scale` beside `*offset`.
    The two hold different values in every case (the host test asserts it), so that a pointer mix-up changes the result."""
    paths = {o.path for o in w.operands}
    out = []
    for p in sorted(paths, key=str):
        last = p[-1]
        mate = p[:-1] + (1,) if last == 0 and len(p) > 1 else (p[:-1] + (last[:-5] + "offset",) if isinstance(last, str) and last.endswith("scale") else None)
        if mate in paths:
            out.append((p, mate))
    return out


Case = namedtuple("Case", "id build")
# check(out, after): out = the wrapper's result, after = the arguments afterwards.  canon(out): the result with what no caller may read
# (the padding rows of a fragment-blocked image, which the wrapper leaves uninitialised) blanked before two calls' bits are compared.
# stable False: the result holds sums gathered with atomics, whose bits move from launch to launch inside the pin's bound: another form
# of an operand is then held to `check` again, not to the canonical call's bits.
Built = namedtuple("Built", "args sizes check canon stable", defaults=(None, True))


def blank_padding(img, rows, cols):
    """A fragment-blocked image with the bytes of its padding rows set to zero."""
    _, real = O.tiled_image_bytes(np.zeros((rows, cols), np.int8), rows, cols)
    return np.where(real.reshape(img.shape), img, np.int8(0))
# aliases: pairs of C-argument positions that may hold one pointer (documented); scalars: the parameters that are no tensors
Wrapper = namedtuple("Wrapper", "name operands scalars cases aliases", defaults=((),))


def lookup(args, path):
    v = args[path[0]]
    for k in path[1:]:
        v = v[k]
    return v


def replace(args, path, value):
    """A copy of args (containers along the path copied, leaves shared) with the operand at `path` replaced."""
    def go(v, p):
        if not p:
            return value
        if isinstance(v, dict):
            c = dict(v)
            c[p[0]] = go(v[p[0]], p[1:])
            return c
        c = list(v)
        c[p[0]] = go(v[p[0]], p[1:])
        return tuple(c) if isinstance(v, tuple) else c
    return go(args, tuple(path))


# ---- comparisons (the pins' own) ------------------------------------------------------------------------------------------------------
def same_bits(got, want, what):
    """Bit for bit, NaN exactly where the oracle has NaN (test_gpu_quantize.check_values)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype.kind != "f":
        bad = np.argwhere(got != want)
    else:
        u = {2: np.uint16, 4: np.uint32, 8: np.uint64}[want.dtype.itemsize]
        ng, nw = np.isnan(got), np.isnan(want)
        bad = np.argwhere((ng != nw) | (~nw & ~ng & (got.view(u) != want.view(u))))
    assert len(bad) == 0, "%s: %d of %d differ, first at %r: got %r want %r" % (what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])],
                                                                               want[tuple(bad[0])])


def same_ints(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got.astype(np.int64) != want.astype(np.int64))
    assert len(bad) == 0, "%s: %d of %d differ, first at %r: got %d want %d" % (what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])],
                                                                               want[tuple(bad[0])])


# ---- a1: scale_offset_from_minmax -----------------------------------------------------------------------------------------------------
def _so_case(bits, sym):
    def build():
        mn = np.array([-2.0, -0.5, 0.0, -3.25, 0.125], F32)           # every value exact in fp16
        mx = np.array([2.5, 0.75, 1.0, -1.0, 0.125], F32)

        def check(out, after):
            s, o, _, _ = O.scale_offset_from_min_max(mn, mx, bits, sym)
            same_bits(out[0], s, "scale")
            same_bits(out[1], o, "offset")
        return Built(dict(min_val=mn, max_val=mx, bitwidth=bits, is_symmetric=sym), dict(n=5), check)
    return Case("%dbit-%s" % (bits, "sym" if sym else "asym"), build)


# ---- a3: min / max -------------------------------------------------------------------------------------------------------------------
def _mm_x(rows, cols, dtype):
    dt = F32 if dtype == "f32" else F16
    x = np.random.default_rng(rows * 1009 + cols).uniform(-3, 3, (rows, cols)).astype(dt)
    x[rows - 1, cols - 1], x[0, 0] = dt(7.5), dt(-6.25)                                   # the extremes at the two ends
    return x


def _running(n, k):
    """Running statistics that already hold something in every other slot: the launch has to fold, not overwrite."""
    mn, mx = np.full(n, np.inf, F32), np.full(n, -np.inf, F32)
    mn[::2], mx[::2] = F32(-100.0 - k), F32(100.0 + k)
    return mn, mx


def _mm_inplace_case(which, dtype):
    rows, cols = 5, 67

    def build():
        x = _mm_x(rows, cols, dtype)
        n = {"tensor": 1, "rows": rows, "cols": cols}[which]
        mn, mx = _running(n, 0) if which != "tensor" else (np.array([1.5], F32), np.array([-1.5], F32))
        axis = {"tensor": None, "rows": 1, "cols": 0}[which]

        def check(out, after):
            same_bits(after["mn"], np.minimum(mn, np.atleast_1d(x.min(axis=axis).astype(F32))), "mn")
            same_bits(after["mx"], np.maximum(mx, np.atleast_1d(x.max(axis=axis).astype(F32))), "mx")
        return Built({("x" if which == "tensor" else "x2d"): x, "mn": mn, "mx": mx}, dict(rows=rows, cols=cols, numel=rows * cols), check)
    return Case(dtype, build)


def _mm_fresh_case(which, dtype):
    rows, cols = 5, 67

    def build():
        x = _mm_x(rows, cols, dtype)
        axis = {"tensor": None, "rows": 1, "cols": 0}[which]

        def check(out, after):
            same_bits(out[0], np.atleast_1d(x.min(axis=axis).astype(F32)), "min")
            same_bits(out[1], np.atleast_1d(x.max(axis=axis).astype(F32)), "max")
        return Built({("x" if which == "tensor" else "x2d"): x}, dict(rows=rows, cols=cols, numel=rows * cols), check)
    return Case(dtype, build)


def _mm_new_case():
    def build():
        def check(out, after):
            same_bits(out[0], np.full(5, np.inf, F32), "min")
            same_bits(out[1], np.full(5, -np.inf, F32), "max")
        return Built(dict(n=5, device=DEVICE), {}, check)
    return Case("n5", build)


# ---- a5: fake_quant / quantize / epilogue vectors / pack_w4 ----------------------------------------------------------------------------
def _fq_case(cid, rows, cols, dtype, grid, per_row, out=False):
    def build():
        x, sc, of, qmin, qmax = Q.make_input(rows, cols, grid, dtype, per_row, True)
        with np.errstate(over="ignore", invalid="ignore"):
            if dtype == "f32":
                want = O.fake_quant(x, sc.reshape(-1, 1), of.reshape(-1, 1), qmin, qmax)
            elif per_row:
                want = O.fake_quant_f16_per_row(x, sc, of, qmin, qmax)
            else:
                want = O.fake_quant_f16_per_tensor(x, sc[0], of[0], qmin, qmax)[0]
        args = dict(x=x, scale=sc, offset=of, qmin=float(qmin), qmax=float(qmax))
        if out:
            args["out"] = np.full(x.shape, 9.0, x.dtype)

        def check(res, after):
            same_bits(res, want, cid)
            if out:
                same_bits(after["out"], want, cid + " out=")
        return Built(args, dict(rows=rows, cols=cols, numel=rows * cols, n_scale=sc.size), check)
    return Case(cid, build)


def _fqb_case(cid, rows, cols, n_scale, grid):
    """fake_quant_backward: grad_x bit for bit, the two sums within gamma_n sum|term| of the float64 sums (train_cases / test_gpu_train)."""
    case = T.FqbCase("contract_" + cid, rows, cols, n_scale, (0, 0, 0), T.FQB_GRIDS[grid], False)

    def build():
        d, e = T.fqb_inputs(case), T.fqb_expect(case)
        args = dict(x=d["x"], grad_y=d["g"], scale=d["scale"], offset=d["offset"], qmin=float(d["qmin"]), qmax=float(d["qmax"]))

        def check(res, after):
            gx, gs, go = res
            same_bits(gx.reshape(case.rows, case.cols), np.asarray(e["gx"], F32).reshape(case.rows, case.cols), cid + " grad_x")
            for name, g, want, bar in (("grad_scale", gs, e["sum_ts"], e["bar_ts"]), ("grad_offset", go, e["sum_to"], e["bar_to"])):
                g, want, bar = (np.asarray(v, np.float64).reshape(-1) for v in (g, want, bar))
                with np.errstate(invalid="ignore"):
                    ok = (np.isnan(want) & np.isnan(g)) | (np.abs(g - want) <= bar)
                assert ok.all(), "%s %s: got %r want %r bound %r" % (cid, name, g, want, bar)
        return Built(args, dict(rows=case.rows, cols=case.cols, numel=case.rows * case.cols, n_scale=d["n_group"]), check)
    return Case(cid, build)


def _q_case(cid, rows, cols, dtype, grid, shift, q_dtype, per_row=False, row_sum=False, chan=False, rows_arg=False):
    def build():
        if chan:
            x, sc, of, qmin, qmax = Q.chan_input(rows, cols, grid)
            cs = Q.chan_scale(cols)
        else:
            x, sc, of, qmin, qmax = Q.make_input(rows, cols, grid, dtype, per_row, False)
            cs = None
        want, want_rs = O.quantize_storage(x, sc, of, qmin, qmax, shift, cs)
        args = dict(x=x.reshape(-1) if rows_arg else x, scale=sc, offset=of, qmin=float(qmin), qmax=float(qmax), q_dtype=MQ[q_dtype], shift=shift,
                    want_row_sum=row_sum)
        if rows_arg:
            args["rows"] = rows
        if chan:
            args["chan_scale"] = cs

        def check(res, after):
            q, rs = res if row_sum else (res, None)
            assert q.dtype == Q.Q_NUMPY[q_dtype] and q.shape == args["x"].shape, (cid, q.dtype, q.shape)
            same_ints(q.reshape(rows, cols), want, cid)
            if row_sum:
                assert rs.dtype == np.int32
                same_ints(rs, want_rs, cid + " row_sum")
        return Built(args, dict(rows=rows, cols=cols, numel=rows * cols, n_scale=sc.size), check)
    return Case(cid, build)


def _qt_case(cid, rows, cols, grid, shift, chan=False, row_sum=True):
    def build():
        if chan:
            x, sc, of, qmin, qmax = Q.chan_input(rows, cols, grid)
            cs = Q.chan_scale(cols)
        else:
            x, sc, of, qmin, qmax = Q.make_input(rows, cols, grid, "f32", False, False)
            cs = None
        stored, want_rs = O.quantize_storage(x, sc, of, qmin, qmax, shift, cs)
        want, real = O.tiled_image_bytes(stored, rows, cols)
        args = dict(x2d=x, scale=sc, offset=of, qmin=float(qmin), qmax=float(qmax), shift=shift, want_row_sum=row_sum)
        if chan:
            args["chan_scale"] = cs

        def check(res, after):
            q, rs = res if row_sum else (res, None)
            assert q.dtype == np.int8 and q.shape == ((rows + 15) // 16 * 16, cols), (cid, q.dtype, q.shape)
            got = q.reshape(-1)
            bad = np.flatnonzero((got != want.reshape(-1)) & real.reshape(-1))
            assert len(bad) == 0, "%s: %d image bytes differ, first at byte %d" % (cid, len(bad), bad[0])
            if row_sum:
                same_ints(rs, want_rs, cid + " row_sum")
        def canon(res):
            return (blank_padding(res[0], rows, cols), res[1]) if row_sum else blank_padding(res, rows, cols)
        return Built(args, dict(rows=rows, cols=cols, numel=rows * cols, n_scale=1), check, canon)
    return Case(cid, build)


def _epi_case(cid, N, per_row):
    def build():
        c = Q.epilogue_case(N, per_row, 121.0, 128, 128, 5632)
        alpha, w_zp, col = O.linear_epilogue_vectors(**c)

        def check(res, after):
            same_bits(res[0], alpha, cid + " alpha")
            same_ints(res[1], w_zp, cid + " w_zp")
            same_ints(res[2], col, cid + " col_term")
            assert res[1].dtype == np.int32 and res[2].dtype == np.int32
        return Built(dict(c), dict(N=N, n_w=c["w_scale"].size), check)
    return Case(cid, build)


def _pack_case():
    N, K = 3, 128

    def build():
        q = Q.pack_input(N, K)

        def check(res, after):
            assert res.dtype == np.uint8
            same_ints(res, O.pack_w4(q, 0), "pack_w4")
        return Built(dict(nibbles=q), dict(N=N, K=K), check)
    return Case("3x128", build)


# ---- prefill element-wise: act_quant ----------------------------------------------------------------------------------------------------
def _grid_tuple(g):
    return None if g is None else (np.array([g.scale], F32), np.array([g.offset], F32), float(g.qmin), float(g.qmax))


def _act_case(act, mid_on, in_on, numel=1027):
    cid = "%s%s%s" % ("gelu" if act else "silu", "-mid" if mid_on else "", "-in" if in_on else "")

    def build():
        grids = P.act_grids(act, mid_on, in_on)
        x = np.array(P.act_input(numel))
        r = O.prefill_act(P.act_base(), act, *grids)
        want, tie = np.resize(r["y"], numel), np.resize(r["tie"], numel)

        def check(res, after):
            # test_gpu_prefill_elementwise.check_act: bit for bit where `tie` is clear, one output-grid step where it is set
            assert res.shape == x.shape and res.dtype == F32
            same_bits(res[~tie], want[~tie], cid)
            with np.errstate(invalid="ignore"):
                assert np.all(np.abs(res[tie] - want[tie]) <= F32(grids[2].scale) * F32(1.001)), cid
        return Built(dict(x=x, act="gelu" if act else "silu", in_grid=_grid_tuple(grids[0]), mid_grid=_grid_tuple(grids[1]),
                          out_grid=_grid_tuple(grids[2])), dict(numel=numel), check)
    return Case(cid, build)


# ---- prefill element-wise: the gated routes (prefill_elementwise_cases / oracle.prefill_act + prefill_gate) ----------------------------------
def _gated_world(act):
    """The grids and the 256 x 256 expectation of the gated pin.  The pin OBSERVES mq_act_quant on the 256 values of a's grid and holds the
    observation to oracle.prefill_act bit for bit (none of the 256 is flagged on these grids: asserted here too), so the oracle's own
    values stand in for it."""
    va256, obs_grids, Gd = P.gated_observation(act)
    ref = O.prefill_act(va256, act, *obs_grids)
    assert not ref["tie"].any()
    vb256 = O.dequantize_index(np.arange(256, dtype=F32), Gd["b"].scale, Gd["b"].offset)
    e = O.prefill_gate(ref["y"][:, None], vb256[None, :], Gd["out"], 128)
    return va256, vb256, Gd, e["q8"], e["prod"]


def _gated_grid_args(Gd, index):
    return dict(out_grid=_grid_tuple(Gd["out"]), a_grid=_grid_tuple(Gd["a"]) if index else None, b_grid=_grid_tuple(Gd["b"]) if index else None,
                mid_grid=_grid_tuple(Gd["mid"]), act_grid=_grid_tuple(Gd["act"]))


def _gated_case(act, index, want_y, rows=5, cols=16):
    cid = "%s-%s%s" % (("silu", "gelu")[act], "index" if index else "values", "-y" if want_y else "")

    def build():
        va256, vb256, Gd, table, prod = _gated_world(act)
        ai, bi = P.gated_indices(rows, cols)
        a, b = (np.array(ai), np.array(bi)) if index else (va256[ai], vb256[bi])
        args = dict(a=a, b=b, act=("silu", "gelu")[act], q_shift=128, want_y=want_y, **_gated_grid_args(Gd, index))

        def check(res, after):
            q = table[ai, bi]
            same_ints(res[0], q, cid + " q")
            assert res[0].dtype == np.int8 and res[1].dtype == np.int32
            same_ints(res[1], q.astype(np.int64).sum(axis=1), cid + " row_sum")
            if want_y:
                same_bits(res[2], prod[ai, bi], cid + " y")
        return Built(args, dict(rows=rows, cols=cols, numel=rows * cols), check)
    return Case(cid, build)


def _gated_table_case(act):
    def build():
        _, _, Gd, table, _ = _gated_world(act)

        def check(res, after):
            assert res.dtype == np.int8
            same_ints(res.reshape(256, 256), table, "gated_table")
        return Built(dict(act=("silu", "gelu")[act], q_shift=128, **_gated_grid_args(Gd, True)), {}, check)
    return Case(("silu", "gelu")[act], build)


def _lookup_case(tiled, rows=5, cols=64):
    def build():
        ai, bi = P.gated_indices(rows, cols)
        table = np.array(G.gate_table())                          # the lookup only looks up: any int8 map of the 65 536 pairs

        def check(res, after):
            q = table.reshape(256, 256)[ai, bi]
            if tiled:
                want, real = O.tiled_image_bytes(q, rows, cols)
                assert res[0].shape == ((rows + 15) // 16 * 16, cols)
                assert not ((res[0].reshape(-1) != want.reshape(-1)) & real.reshape(-1)).any(), "tiled image"
            else:
                same_ints(res[0], q, "q")
            same_ints(res[1], q.astype(np.int64).sum(axis=1), "row_sum")
        def canon(res):
            return (blank_padding(res[0], rows, cols), res[1]) if tiled else res
        return Built(dict(a=np.array(ai), b=np.array(bi), table=table, tiled=tiled), dict(rows=rows, cols=cols, numel=rows * cols), check, canon)
    return Case("tiled" if tiled else "rowmajor", build)


_GATED_GRIDS = [o for p_ in ("out_grid", "a_grid", "b_grid", "mid_grid", "act_grid") for o in grid_ops(p_, "scale|per-tensor", "offset|per-tensor")]


# ---- the prefill GEMMs behind int8_linear -------------------------------------------------------------------------------------------------
ROWMAJOR = (21, 72, 128)               # the row-major C++ kernel takes any shape: two 16-row fragments, a ragged one, N no multiple of a tile


def _smallest(pred, Ms=(17,), Ns=range(64, 1024, 16), Ks=range(256, 2049, 256)):
    """The smallest (M, N, K) a dispatch predicate of gemm_cases accepts, K first (what the C++ shim restates)."""
    return next((M, N, K) for K in Ks for N in Ns for M in Ms if pred(M, N, K))


FR128 = _smallest(lambda M, N, K: G.fr128_shape(M, N, K) and not G.tiled_supported(M, N, K))


def _gemm_case(cid, entry, shape, grid, w4=False, out=False):
    c = G._case(entry, shape, grid, w4=w4)

    def build():
        p, e = G.problem(c), G.expect(c)
        M, N, K = shape
        tiled = entry.startswith("tiled")
        g = G.GRIDS[grid]
        st = G.storage_of(c)
        args = dict(a_q=O.tiled_image_bytes(p.a, M, K)[0].reshape(-1, K) if tiled else np.array(p.a),
                    w_q=O.pack_w4(p.w, 0) if w4 else p.w.astype(np.int8), a_rowsum=np.array(p.a_rowsum), alpha=np.array(p.alpha),
                    w_zp=np.array(p.w_zp), col_term=np.array(p.col_term), bias=np.array(p.bias), out_dtype=MQ[st], w4=w4)
        if g is not None:
            args.update(out_scale=np.array([p.grids[0][0]], F32), out_offset=np.array([p.grids[0][1]], F32), out_qmin=float(g.qmin),
                        out_qmax=float(g.qmax))
        if tiled:
            args["a_tiled_rows"] = M
        if p.resid is not None:
            args["resid"] = np.array(p.resid)
        if out:
            args["out"] = np.full((M, N), 0x5A, e.stored.dtype)

        def check(res, after):
            same_bits(res, e.stored, cid)
            if out:
                same_bits(after["out"], e.stored, cid + " out=")
        return Built(args, dict(M=M, N=N, K=K, Kw=K // 2 if w4 else K, Mp=(M + 15) // 16 * 16 if tiled else M), check)
    return Case(cid, build)


def _seg_case(cid, entry, shape, segs, grid="u8", w4=False, wrapper="segmented", out=False):
    """int8_linear_segmented (row-major, packed, fragment-blocked) and w4a8_linear_tiled: one GEMM, one 8-bit grid per column segment."""
    c = G._case(entry, shape, grid, w4=w4, segs=segs)

    def build():
        p, e = G.problem(c), G.expect(c)
        M, N, K = shape
        tiled = entry.startswith("tiled")
        w4_ = c.w4
        a = O.tiled_image_bytes(p.a, M, K)[0].reshape(-1, K) if tiled else np.array(p.a)
        grids = [(np.array([s], F32), np.array([o], F32)) for s, o in p.grids]
        common = dict(a_rowsum=np.array(p.a_rowsum), alpha=np.array(p.alpha), w_zp=np.array(p.w_zp), col_term=np.array(p.col_term),
                      bias=np.array(p.bias), grids=grids)
        wq = O.pack_w4(p.w, 0) if w4_ else p.w.astype(np.int8)
        if wrapper == "segmented":
            args = dict(a_q=a, w_q=wq, seg_ends=list(p.seg_end), w4=w4_, **common)
            if tiled:
                args["a_tiled_rows"] = M
        else:
            args = dict(a_tiled=a, M=M, w_packed=wq, out_dtype=MQ[G.storage_of(c)], **common)
            if segs:
                args["seg_ends"] = list(p.seg_end)
        if out:
            args["out"] = np.full((M, N), 0x5A, e.stored.dtype)

        def check(res, after):
            same_bits(res, e.stored, cid)
            if out:
                same_bits(after["out"], e.stored, cid + " out=")
        return Built(args, dict(M=M, N=N, K=K, Kw=K // 2 if w4_ else K, Mp=(M + 15) // 16 * 16 if tiled else M), check)
    return Case(cid, build)


def _seg_grid_ops(n=3):
    return [op(("grids", i, j), "conv", "f32", "1", ("scale", "offset")[j]) for i in range(n) for j in range(2)]


SEG_ROWMAJOR, SEGS = (21, 96, 128), (36, 68, 96)
FRW4 = _smallest(G.frw4_shape)


def _f32in_case(cid, entry, M, N, Kk, grid, agrid, out=False):
    """int8_linear_f32in: the activation quantize fused into the M <= 8 weight-streaming GEMV (gemv_cases / oracle.linear_gemv_launch)."""
    c = V._case(entry, M, N, Kk, grid, agrid=agrid)
    assert V.f32in_accepts(M, Kk)

    def build():
        p, e = V.problem(c), V.expect(c)
        w4 = V.w4_of(c)
        ag = p.agrid
        args = dict(x2d=np.array(p.x), a_scale=np.array([ag[0]], F32), a_offset=np.array([ag[1]], F32), a_qmin=float(ag[2]), a_qmax=float(ag[3]),
                    a_shift=int(ag[4]), w_q=np.array(p.w_packed) if w4 else p.w.astype(np.int8), alpha=np.array(p.alpha), w_zp=np.array(p.w_zp),
                    col_term=np.array(p.col_term), bias=np.array(p.bias), out_dtype=MQ[V.storage_of(c)], w4=w4)
        if p.out_grid is not None:
            args.update(out_scale=np.array([p.out_grid[0]], F32), out_offset=np.array([p.out_grid[1]], F32), out_qmin=float(p.out_grid[2]),
                        out_qmax=float(p.out_grid[3]))
        if out:
            args["out"] = np.full((M, N), 0x5A, e["stored"].dtype)

        def check(res, after):
            same_bits(res, e["stored"], cid)
            if out:
                same_bits(after["out"], e["stored"], cid + " out=")
        return Built(args, dict(M=M, N=N, K=Kk, Kw=Kk // 2 if w4 else Kk), check)
    return Case(cid, build)


# ---- two linears over one fragment-blocked activation (gemm_cases "pair" / "gated": the smallest shapes their dispatch serves) -------------------
def _half(c, p):
    return dict(w=O.pack_w4(p.w, 0) if c.w4 else p.w.astype(np.int8), alpha=np.array(p.alpha), w_zp=np.array(p.w_zp), col_term=np.array(p.col_term),
                bias=None if p.bias is None else np.array(p.bias), out_scale=np.array([p.grids[0][0]], F32), out_offset=np.array([p.grids[0][1]], F32))


def _pair_case(gated):
    c = G._case("gated", G.WN, "u8") if gated else G._case("pair", G.W1, "u8")

    def build():
        p, e = [G.problem(c, 0), G.problem(c, 1)], [G.expect(c, 0), G.expect(c, 1)]
        M, N, K = c.M, c.N, c.K
        args = dict(a_tiled=O.tiled_image_bytes(p[0].a, M, K)[0].reshape(-1, K), rows=M, a_rowsum=np.array(p[0].a_rowsum), first=_half(c, p[0]),
                    second=_half(c, p[1]))
        if gated:
            args["table"] = np.array(G.gate_table())

        def check(res, after):
            if not gated:
                same_bits(res[0], e[0].stored, c.id + " first")
                same_bits(res[1], e[1].stored, c.id + " second")
                return
            want_img, (want, real), want_rs = O.prefill_gemm_gated(e[0].stored, e[1].stored, G.gate_table())
            assert res[0].shape == ((M + 15) // 16 * 16, N) and res[0].dtype == np.int8
            assert not ((res[0].reshape(-1) != want.reshape(-1)) & real.reshape(-1)).any(), c.id + " image"
            same_ints(res[1], want_rs, c.id + " row_sum")

        def canon(res):
            return (blank_padding(res[0], M, N), res[1]) if gated else res
        return Built(args, dict(M=M, N=N, K=K, Mp=(M + 15) // 16 * 16), check, canon)
    return Case(c.id, build)


def _pair_ops(gated):
    out = [op("a_tiled", "raw", ("i8", "u8"), "Mp*K"), op("a_rowsum", "raw", "i32", "M")]
    for h in ("first", "second"):
        out += [op((h, "w"), "raw", ("i8", "u8"), "N*K", r"%s\['w'\]" % h), op((h, "alpha"), "raw", "f32", "N", "alpha"), op((h, "w_zp"), "raw", "i32", "N", "w_zp"),
                op((h, "col_term"), "raw", "i32", "N", "col_term"), op((h, "bias"), "conv", "f32", "N"), op((h, "out_scale"), "conv", "f32", "1", "out_scale"),
                op((h, "out_offset"), "conv", "f32", "1", "out_offset|out_scale")]
    return out + ([op("table", "raw", "i8", "65536")] if gated else [])


# ---- prefill attention and its cache bridges (the checks of test_gpu_prefill_attention.py / test_gpu_prefill_append.py) -----------------------
_AGRIDS = ("qk_a", "qk_b", "qk_out", "pv_a", "pv_b", "pv_out")
SENT = 0x55


def _attq_case(cid, idx_inputs=False, cache=False, tiled=False):
    def build():
        import test_gpu_prefill_attention as A
        case = A.Case(D=64, H=2, KV=1, S=128, idx_inputs=idx_inputs)
        qk, pv = case.grids()
        inp = case.inputs()
        q, k, v, cos, sin, idx = inp
        S, HD, row0 = case.S, case.H * case.D, 5
        rows = row0 + S + 11
        image = (np.full(((rows + 15) // 16 * 16 if tiled else rows, HD), A.SENT, np.int8), np.full(rows, A.SENT, np.int32), row0, 128, tiled)
        args = dict(q=None if idx else np.array(q), k=None if idx else np.array(k), v=None if idx else np.array(v), cos=np.array(cos), sin=np.array(sin),
                    heads=case.H, kv_heads=case.KV, grids={n: _grid_tuple(g) for n, g in zip(_AGRIDS, (*qk, *pv))}, image=image, want_out=True,
                    head_dim=case.D)
        if idx:
            args["qkv_idx"] = (np.array(idx[0]), tuple((np.array([g.scale], F32), np.array([g.offset], F32)) for g in idx[1]))
        if cache:
            n = case.KV * 128 * case.D
            args.update(pos0=0, cache=dict(rows=128, kv_heads=case.KV, head_dim=case.D, k_i8=np.zeros(n, np.int8), vt_i8=np.zeros(n, np.int8),
                                           k_rs=np.zeros(case.KV * 128, np.int32), k_f16=np.zeros(n, F16), v_pre=None))

        def check(res, after):
            import torch
            assert res.shape == (S, HD) and res.dtype == F32 and np.isfinite(res).all()
            A._image_check(case, pv, res, torch.from_numpy(after["image"][0]), torch.from_numpy(after["image"][1]), row0, S, tiled, cid)
            A._oracle_check(case, qk, pv, inp, res, A._rows(S, case.seed), [], cid)
        return Built(args, dict(S=S, rot=cos.shape[1], n8=case.KV * 128 * case.D, nrs=case.KV * 128), check)
    return Case(cid, build)


def _attq_ops():
    out = [op(n, "layout", "f32", None, n) for n in "qkv"] + [op("cos", "conv", "f32", "S*rot"), op("sin", "conv", "f32", "S*rot", "cos / sin|sin")]
    out += [op(("grids", n, j), "conv", "f32", "1", ("scale|per-tensor", "offset|per-tensor")[j]) for n in _AGRIDS for j in range(2)]
    out += [op(("image", 0), "out", "i8", None, "image"), op(("image", 1), "out", "i32", None, "image")]
    out += [op(("qkv_idx", 0), "layout", "u8", None, "qkv_idx")]
    out += [op(("qkv_idx", 1, i, j), "conv", "f32", "1", ("scale|per-tensor", "offset|per-tensor")[j]) for i in range(3) for j in range(2)]
    return out + _cache_ops("raw", False)


def _cache_ops(kind, bridge):
    lab = r"cache\['%s'\]|shape / device|different devices"
    return [op(("cache", "k_i8"), kind, "i8", "n8", lab % "k_i8"), op(("cache", "vt_i8"), kind, "i8", "n8", lab % "vt_i8"),
            op(("cache", "k_rs"), kind, "i32", "nrs", lab % "k_rs"), op(("cache", "k_f16"), kind, "f16", "n8", lab % "k_f16")]


_BR = dict(KV=2, D=64, L=128)


def _bridge_cache(fill):
    KV, D, L = _BR["KV"], _BR["D"], _BR["L"]
    n = KV * L * D
    return dict(rows=L, kv_heads=KV, head_dim=D, k_i8=np.full(n, fill, np.int8), vt_i8=np.full(n, fill, np.int8), k_rs=np.full(KV * L, 0x33333333, np.int32),
                k_f16=np.full(n, 0x3333, np.uint16).view(F16), v_pre=None)


def _tcache(c):
    import torch
    return {k: (torch.from_numpy(np.array(v)) if isinstance(v, np.ndarray) else v) for k, v in c.items()}


def _import_case(chunked):
    def build():
        import test_gpu_prefill_append as B
        import torch
        KV, D, L, n = _BR["KV"], _BR["D"], _BR["L"], 64
        rng = np.random.default_rng(5 + chunked)
        k = rng.integers(-128, 128, (KV, L, D)).astype(np.int8)
        vl = rng.integers(-128, 128, (KV, L, D)).astype(np.int8)                                   # the values, position-major
        v = np.ascontiguousarray(vl.reshape(KV, L // 16, 16, D).transpose(0, 1, 3, 2)) if chunked else vl
        zq, zk = 131.0, 125.0
        grids = dict(qk_a=(np.array([0.05], F32), np.array([zq], F32), 0.0, 255.0), qk_b=(np.array([0.047], F32), np.array([zk], F32), 0.0, 255.0))
        args = dict(cache=_bridge_cache(0x33), k=k, v=v, n=n, grids=grids, v_chunked=chunked)

        def check(res, after):
            # test_gpu_prefill_append.test_import_matches_the_header_formulas
            iv = B._image_views(_tcache(after["cache"]))
            tk, tv = torch.from_numpy(k[:, :n].copy()), torch.from_numpy(vl[:, :n].copy())
            assert torch.equal(iv["k_i8"][:, :n], tk)
            assert torch.equal(iv["k_rs"][:, :n], (-(int(zq) - 128) * tk.int().sum(-1)).int())
            assert torch.equal(iv["vt_i8"][:, :n // 64], B._vt_of(tv))
            assert torch.equal(iv["k_f16"][:, :n // 64], B._k_f16_of(tk, zk).view(torch.int16))
            assert bool((iv["k_f16"][:, n // 64:] == 0x3333).all()) and bool((iv["k_i8"][:, n:] == 0x33).all())
            assert bool((iv["vt_i8"][:, n // 64:] == 0x33).all()) and bool((iv["k_rs"][:, n:] == 0x33333333).all())
            same_bits(after["k"], k, "k untouched")
            same_bits(after["v"], v, "v untouched")
        return Built(args, dict(n8=KV * L * D, nrs=KV * L, KLD=KV * L * D), check)
    return Case("chunked" if chunked else "position-major", build)


def _export_case(chunked):
    def build():
        import test_gpu_prefill_append as B
        import torch
        KV, D, L, p0, n = _BR["KV"], _BR["D"], _BR["L"], 64, 37
        rng = np.random.default_rng(9 + chunked)
        cache = _bridge_cache(0)
        cache["k_i8"] = rng.integers(-128, 128, KV * L * D).astype(np.int8)
        cache["vt_i8"] = rng.integers(-128, 128, KV * L * D).astype(np.int8)
        k = np.full((KV, L, D), SENT, np.int8)
        v = np.full((KV, L // 16, D, 16) if chunked else (KV, L, D), SENT, np.int8)
        args = dict(cache=cache, k=k, v=v, p0=p0, n=n, v_chunked=chunked)

        def check(res, after):
            # test_gpu_prefill_append.test_export_writes_the_rows_and_nothing_else
            want_k, want_v = B._decoded(_tcache(cache), L)
            gk, gv = torch.from_numpy(after["k"]), torch.from_numpy(after["v"])
            logical = gv.permute(0, 1, 3, 2).reshape(KV, L, D) if chunked else gv
            for got, want in ((gk, want_k), (logical, want_v)):
                assert torch.equal(got[:, p0:p0 + n], want[:, p0:p0 + n])
                assert bool((got[:, :p0] == SENT).all()) and bool((got[:, p0 + n:] == SENT).all())
        return Built(args, dict(n8=KV * L * D, nrs=KV * L, KLD=KV * L * D), check)
    return Case("chunked" if chunked else "position-major", build)


# ---- LWC ------------------------------------------------------------------------------------------------------------------------------
def _lwc_case(bits, sym):
    rows, cols = 5, 64
    cid = "%dbit-%s" % (bits, "sym" if sym else "asym")

    def build():
        d = T.lwc_inputs(cols, bits, sym, rows)
        f = d["fwd"]

        def check(res, after):
            out, mn, mx, sc, of = res
            for name, g in (("row_min", mn), ("row_max", mx), ("scale", sc), ("offset", of)):
                same_bits(g, np.asarray(f[name], F32), "%s %s" % (cid, name))
            same_bits(out, np.asarray(f["y"], F32), cid + " out")
        return Built(dict(w=np.array(d["w"]), sig_lo=np.array(d["sig_lo"]), sig_hi=np.array(d["sig_hi"]), bitwidth=bits, is_symmetric=sym),
                     dict(N=rows, K=cols, numel=rows * cols), check)
    return Case(cid, build)


def _lwc_bwd_case(bits, sym):
    rows, cols = 5, 64
    cid = "%dbit-%s" % (bits, "sym" if sym else "asym")

    def build():
        d = T.lwc_inputs(cols, bits, sym, rows)
        f, w = d["fwd"], d["w"]
        b = O.lwc_fused_backward(w, d["g"], d["sig_lo"], d["sig_hi"], f["row_min"], f["row_max"], bits, sym)
        n = T.lwc_n(cols)

        def bounded(got, want, bar, what, where=None):
            got, want, bar = (np.asarray(v, np.float64) for v in (got, want, bar))
            with np.errstate(invalid="ignore"):
                ok = (np.isnan(want) & np.isnan(got)) | (np.abs(got - want) <= bar)
            if where is not None:
                ok = ok | ~where
            assert ok.all(), "%s %s outside the bound" % (cid, what)

        def check(res, after):
            # test_gpu_train.test_lwc_fused_pass_forward_exact_and_backward, through the wrapper
            gw, glo, ghi = res
            ext = b["extreme"]
            with np.errstate(invalid="ignore"):
                exact_ok = (np.isnan(gw) & np.isnan(b["gx"])) | (gw == b["gx"]) | ext
            assert exact_ok.all(), cid + " grad_w off the row extremes"
            with np.errstate(invalid="ignore"):
                bar_w = np.where(b["c_scat"] > 0, T.gamma(n + 8) * (np.abs(b["gx"]) + b["c_scat"] * b["sumabs"][:, None]), 0.0)
            bounded(gw, b["grad_w"], bar_w, "grad_w on the row extremes", ext)
            for name, g, c in (("grad_sig_lo", glo, b["c_sig_lo"]), ("grad_sig_hi", ghi, b["c_sig_hi"])):
                with np.errstate(invalid="ignore"):
                    bar = np.where(c > 0, T.gamma(n + 6) * c * b["sumabs"], 0.0)
                bounded(g, b[name], bar, name)
        return Built(dict(w=np.array(w), grad_out=np.array(d["g"]), sig_lo=np.array(d["sig_lo"]), sig_hi=np.array(d["sig_hi"]),
                          row_min=np.asarray(f["row_min"], F32), row_max=np.asarray(f["row_max"], F32), bitwidth=bits, is_symmetric=sym),
                     dict(N=rows, K=cols, numel=rows * cols), check)
    return Case(cid, build)


# ---- training: attention_probs_train(_backward) ---------------------------------------------------------------------------------------------
def _g4(g):
    return (np.array([g[0]], F32), np.array([g[1]], F32), float(g[2]), float(g[3]))


def _exact_where(got, want, where, what):
    with np.errstate(invalid="ignore"):
        ok = (np.isnan(got) & np.isnan(want)) | (got == want) | ~where
    assert ok.all(), "%s: %d differ" % (what, int((~ok).sum()))


def _bounded(got, want, bar, what, where=None):
    got, want, bar = (np.asarray(v, np.float64) for v in (got, want, bar))
    with np.errstate(invalid="ignore"):
        ok = (np.isnan(want) & np.isnan(got)) | (np.abs(got - want) <= bar)
    if where is not None:
        ok = ok | ~where
    assert ok.all(), "%s: %d outside the bound" % (what, int((~ok).sum()))


def _attn_case(case, backward):
    def build():
        d = T.attn_inputs(case)
        f, raw = d["fwd"], d["raw"]
        args = dict(raw=np.array(raw), mask=None if d["mask"] is None else np.array(d["mask"]), grid1=_g4(d["grid1"]), grid2=_g4(d["grid2"]),
                    sqrt_d=float(case.sqrt_d))
        if backward:
            args["grad_out"] = np.array(d["gy"])

        def check_fwd(res, after):
            # test_gpu_train.test_attention_probs_train_forward: decided elements exact, an undecided one either neighbouring grid value
            assert res.shape == raw.shape and res.dtype == F32
            und = f["undecided"] & ~f["nan_row"][:, None]
            _exact_where(res, f["out"], ~und, case.name + " decided probabilities")
            _exact_where(res, f["out_alt"], und & (res != f["out"]), case.name + " undecided probabilities")
            assert np.all(res[f["masked"] & ~f["nan_row"][:, None]] == 0)

        def check_bwd(res, after):
            # test_gpu_train.test_attention_probs_train_backward
            graw, gg = res
            b = d["bwd"]
            in1 = b["fwd"]["in1"]
            _exact_where(graw, np.zeros_like(graw), ~in1, case.name + " grad_raw where Q1 clamps")
            _bounded(graw, b["grad_raw"], b["e_raw"], case.name + " grad_raw", in1)
            vals, bars = T.attn_bwd_sums(case, d)
            for i in range(4):
                _bounded(gg[i], vals[i], bars[i], "%s grid gradient %d" % (case.name, i))
        return Built(args, dict(rows=case.rows, cols=case.cols, numel=case.rows * case.cols), check_bwd if backward else check_fwd, None,
                     not backward)                                # the four grid gradients are atomic sums
    return Case(case.name, build)


_ATTN = [c for c in T.ATTN_CASES if c.rows <= 30 and c.cols <= 256][:4]


def _attn_ops(backward):
    return ([op("raw", "conv", "f32", None)] + ([op("grad_out", "conv", "f32", "numel")] if backward else []) + [op("mask", "conv", "f32", None)]
            + grid_ops("grid1", "grid", "grid") + grid_ops("grid2", "grid", "grid"))


# ---- prefill: rmsnorm_quant (the norm pin's own checks, test_gpu_prefill_elementwise.check_norm) ------------------------------------------
def _norm_case(cid, tag, emit_int8=False, emit_tiled=False, want_y=True, emit_rowmajor=True):
    def build():
        c = P.NORM_CASES[tag]
        rows, cols = c["x"].shape
        args = dict(x=np.array(c["x"]), weight=np.array(c["w"]), bias=None if c["b"] is None else np.array(c["b"]), eps=float(c["eps"]),
                    in_grid=_grid_tuple(c["in_q"]), out_grid=_grid_tuple(c["out_q"]), emit_int8=emit_int8, layernorm=bool(c["layernorm"]),
                    emit_tiled=emit_tiled, want_y=want_y, emit_rowmajor=emit_rowmajor)

        def check(res, after):
            import test_gpu_prefill_elementwise as E              # the pin's comparison (row-scalar search, tie classes), not a new one
            y, q, rs, shift, qt = res if emit_int8 else (res, None, None, c["shift"], None)
            assert shift == c["shift"] and (y is None) == (not want_y) and (q is None) == (not (emit_int8 and (emit_rowmajor or not emit_tiled)))
            got = dict(y=y, q=q, rs=None if rs is None else rs.astype(np.int64), qt=None)
            if y is not None:
                assert y.shape == (rows, cols) and y.dtype == F32
            if qt is not None:
                assert qt.shape == ((rows + 15) // 16 * 16, cols) and qt.dtype == np.int8
                un = np.array(E.untile(qt.reshape(-1), cols))
                un[rows:] = E.CQ                                  # the wrapper's padding rows are uninitialised: only the real rows are judged
                got["qt"] = un
            E.check_norm(c, got, tag=cid)

        def canon(res):
            if not (emit_int8 and emit_tiled):
                return res
            return tuple(res[:4]) + (blank_padding(res[4], rows, cols),)
        return Built(args, dict(rows=rows, cols=cols), check, canon)
    return Case(cid, build)


# ---- qmatmul: every form x2 may arrive in against ONE oracle (qmatmul_cases / oracle.qmatmul_launch) ------------------------------------------
def _qmm_case(cid, qid, x2_form):
    c = QM.BY_ID[qid]

    def build():
        x1, x2m = QM.operands(qid)
        e = QM.expect(qid)
        g1, g2, go = QM.grids_of(c)
        logical = QM.logical_x2(c)                                # [B, K, N] as the wrapper's signature has it
        if x2_form == "dense":
            x2 = np.ascontiguousarray(logical)
        elif x2_form == "transposed-view":
            x2 = np.swapaxes(np.ascontiguousarray(np.swapaxes(logical, 1, 2)), 1, 2)
        else:                                                     # "sliced": neither dense nor a transposed dense tensor -> copied
            buf = np.zeros(logical.shape[:-1] + (logical.shape[-1] + 3,), F32)
            buf[..., :logical.shape[-1]] = logical
            x2 = buf[..., :logical.shape[-1]]
        args = dict(x1=np.array(x1), x2=x2, grid1=_g4(g1), grid2=_g4(g2), grid_out=None if go is None else _g4(go))

        def check(res, after):
            same_bits(res, e["out"], cid)
        return Built(args, dict(B=c.batch, M=c.M, N=c.N, K=c.K), check)
    return Case(cid, build)


# ---- per-group GEMM (grouped_gemm_cases / oracle.grouped_linear) -----------------------------------------------------------------------------
def _grouped_case(gid):
    c = GG.BY_ID[gid]

    def build():
        p, e = GG.problem(gid), GG.expect(gid)
        args = dict(a_q=np.array(p["a"]), w_q=np.array(p["w"]), group_size=c.gs, a_gsum=np.array(p["a_gsum"]), alpha=np.array(p["alpha"]),
                    cw=np.array(p["cw"]), t=np.array(p["t"]), bias=None if p["bias"] is None else np.array(p["bias"]))

        def check(res, after):
            same_bits(res, e["out"], gid)
        return Built(args, dict(M=c.M, N=c.N, K=c.gs * c.G, G=c.G), check)
    return Case(gid, build)


# ---- prefill attention's two host helpers --------------------------------------------------------------------------------------------------
def _image_cache_case():
    def build():
        def check(res, after):
            rows = 128                                                # ceil64(100)
            assert (res["rows"], res["kv_heads"], res["head_dim"]) == (rows, 2, 64)
            for k, n, dt in (("k_i8", 2 * rows * 64, np.int8), ("vt_i8", 2 * rows * 64, np.int8), ("k_rs", 2 * rows, np.int32), ("k_f16", 2 * rows * 64, F16)):
                assert res[k].dtype == dt and res[k].shape == (n,) and not res[k].any(), k
            assert res["v_pre"] is None                               # head_dim 64 keeps no value prefix
        return Built(dict(kv_heads=2, head_dim=64, max_len=100, device=DEVICE), {}, check)
    return Case("kv2-d64-len100", build)


def _f16_ok_case():
    def build():
        def check(res, after):
            from mobilequant_amd import ops
            lo, hi = ops.F16_OFFSETS
            assert res is True
            assert ops.attention_f16_offsets_ok(lo, hi) and not ops.attention_f16_offsets_ok(lo - 1, 0.0) and not ops.attention_f16_offsets_ok(0.0, hi + 1)
        return Built(dict(), {}, check)
    return Case("no-offsets", build)


# ---- token scoring (the float64 reference and bounds of test_gpu_score.py, evaluated on the host) ---------------------------------------------
def _score_case(cid, M, Kk, V, with_bias, with_targets):
    def build():
        rng = np.random.default_rng(7 * M + V)
        y = rng.standard_normal((M, Kk)).astype(F32)
        w = (rng.standard_normal((V, Kk)) * (3.0 / np.sqrt(Kk))).astype(F32)
        b = rng.standard_normal(V).astype(F32) if with_bias else None
        t = rng.integers(0, V, M).astype(np.int64) if with_targets else None
        if t is not None:
            t[::3] = -1                                              # ignored rows: logprob exactly 0
        args = dict(y=y, weight=w, bias=b, targets=t)

        def check(res, after):
            import torch
            import test_gpu_score as S
            lp, lse, am = res
            assert lp.dtype == lse.dtype == F32 and am.dtype == np.int64 and lp.shape == lse.shape == am.shape == (M,)
            tt = torch.from_numpy(t) if t is not None else torch.full((M,), -1, dtype=torch.int64)
            ref = S.reference(torch.from_numpy(y), torch.from_numpy(w), None if b is None else torch.from_numpy(b), tt)
            b_lse, b_lp = (v.numpy() for v in S.bounds(ref, V))
            assert np.all(np.abs(lse.astype(np.float64) - ref["lse"].numpy()) <= b_lse), cid + " lse"
            assert np.all(np.abs(lp.astype(np.float64) - ref["lp"].numpy()) <= b_lp), cid + " logprob"
            assert np.all(lp[tt.numpy() < 0] == 0)
            decided = (ref["gap"] > 2 * ref["E"]).numpy()
            assert np.array_equal(am[decided], ref["arg"].numpy()[decided]), cid + " argmax"
        return Built(args, dict(M=M, K=Kk, V=V), check)
    return Case(cid, build)


# ---- calibration: histograms (hist_ref) -----------------------------------------------------------------------------------------------------
def _hist_new_case():
    def build():
        def check(res, after):
            assert res[0].dtype == np.int64 and res[1].dtype == np.int64
            same_ints(res[0], np.zeros((3, 512 << 2), np.int64), "counts")
            same_ints(res[1], np.zeros(3, np.int64), "nan")
        return Built(dict(n_slots=3, mantissa_bits=2, device=DEVICE), {}, check)
    return Case("3x2", build)


def _hist_case(fp16, m, minmax=True, numel=1027):
    cid = "%s-m%d%s" % ("f16" if fp16 else "f32", m, "" if minmax else "-histogram-only")

    def build():
        x = np.array(H.planted_data(numel, 1000 + numel, fp16))
        (want_c, want_nan), (want_mn, want_mx) = H.histogram(x, m), H.minmax(x)
        have = np.arange(2 * H.nb_of(m), dtype=np.int64) % 3              # the histogram is ADDED to what the row holds
        args = dict(t=x, counts_row=have.copy(), nan_row=np.array([5], np.int64), mn=np.array([np.inf], F32) if minmax else None,
                    mx=np.array([-np.inf], F32) if minmax else None, mantissa_bits=m)

        def check(res, after):
            same_ints(after["counts_row"], have + np.asarray(want_c, np.int64), cid + " counts")
            same_ints(after["nan_row"], np.array([5 + int(want_nan)]), cid + " nan")
            if minmax:
                same_bits(after["mn"], np.array([want_mn], F32), cid + " min")
                same_bits(after["mx"], np.array([want_mx], F32), cid + " max")
        return Built(args, dict(numel=numel, NB2=2 * H.nb_of(m)), check)
    return Case(cid, build)


# ---- training: the clip search (lwc_search_ref: the pin's tolerance on the costs, its rules on the choice) ---------------------------------------
def _lsearch_case(cid, rows, cols, bits, sym, ncand, cw_mode, return_costs):
    c = LS._case(rows, cols, bits, sym, ncand, cw_mode)

    def build():
        w, lo, hi, cw = LS.case_inputs(c)
        want = LS.cost_table(w, lo, hi, bits, sym, cw)
        want_idx, cls = LS.first_min(want), LS.classify(want, cols)
        args = dict(w2d=np.array(w), sig_lo=np.array(lo), sig_hi=np.array(hi), bitwidth=bits, is_symmetric=sym,
                    col_weight=None if cw is None else np.array(cw), return_costs=return_costs)

        def check(res, after):
            idx, best, base = res[:3]
            assert idx.dtype == np.int32 and best.dtype == base.dtype == np.float64 and idx.shape == best.shape == base.shape == (rows,)
            tol = LS.TOL(cols)
            if return_costs:
                costs = res[3]
                assert costs.shape == want.shape and np.array_equal(np.isnan(costs), np.isnan(want))
                ok = ~np.isnan(want)
                assert (np.abs(costs[ok] - want[ok]) <= tol * want[ok]).all(), cid
                assert np.array_equal(base, costs[:, 0], equal_nan=True) and np.array_equal(best, costs[np.arange(rows), idx], equal_nan=True)
                assert np.array_equal(idx, LS.first_min(costs))
            for r in range(rows):
                if cls[r] == "nan":
                    assert idx[r] == 0 and np.isnan(best[r]) and np.isnan(base[r])
                    continue
                if cls[r] in ("clear", "tie"):
                    assert idx[r] == want_idx[r], (cid, r)
                assert want[r, idx[r]] <= want[r].min() * (1.0 + 4.0 * tol), (cid, r)
                assert abs(best[r] - want[r, idx[r]]) <= tol * want[r, idx[r]] and abs(base[r] - want[r, 0]) <= tol * want[r, 0], (cid, r)
        return Built(args, dict(rows=rows, cols=cols, C=ncand, numel=rows * cols), check)
    return Case(cid, build)


# ---- calibration: the score chain, the norm and the gated product with their statistics (the calibration pin's own checks) --------------------
def _slots(n):
    return [np.array([np.inf if i % 2 == 0 else -np.inf], F32) for i in range(n)]


_STAT4 = ("raw_min", "raw_max", "probs_min", "probs_max")


def _probs_case(c, causal=False, store_masked=True):
    def build():
        if causal:
            raw, mask = np.array(K.causal_base(c)).reshape(c.blocks, c.seq, c.seq), None
        else:
            raw, mask = K.probs_input(c, 0)
            raw = np.array(raw).reshape(2, c.rows // 2, c.cols)            # [..., S, T]: rows come from every leading dimension
        st = dict(zip(_STAT4, _slots(4)))
        args = dict(raw=raw, sqrt_d=float(K.SQRT_D), **st)
        if causal:
            args.update(out=np.zeros_like(raw), store_masked=store_masked)
        else:
            args["mask"] = None if mask is None else np.array(mask)
        raw2d = raw.reshape(-1, raw.shape[-1]).copy()

        def check(res, after):
            import test_gpu_calib as TC
            got = np.asarray(res).reshape(raw2d.shape)
            if causal:
                TC.compare_probs(got, raw2d, c.id, causal=True)          # quads above the diagonal hold the buffer's zeros either way
                same_bits(after["out"].reshape(raw2d.shape), got, c.id + " out=")
                same_bits(after["raw"].reshape(raw2d.shape), raw2d, c.id + " raw untouched")
            else:
                TC.compare_probs(got, raw2d, c.id, mask=args["mask"])
                same_bits(after["raw"].reshape(raw2d.shape), got, c.id + " in place")
            TC.check_prob_stats(np.concatenate([after[k] for k in _STAT4]), raw2d, got, c.id)
        return Built(args, dict(numel=raw.size, S=raw.shape[-2], T=raw.shape[-1]), check)
    return Case(c.id + ("" if not causal else ("-stored" if store_masked else "-skipped")), build)


def _cnorm_case(c):
    def build():
        x, d, w, b = K.norm_input(c)
        names = ("in_min", "in_max", "out_min", "out_max") + (("delta_min", "delta_max") if c.slots else ())
        args = dict(x=np.array(x), delta=None if d is None else np.array(d), weight=np.array(w), bias=None if b is None else np.array(b),
                    eps=float(K.NORM_EPS), layernorm=bool(c.ln), **dict(zip(names, _slots(len(names)))))

        def check(res, after):
            import test_gpu_calib as TC
            o = O.calib_norm_rows(x, d, w, b, K.NORM_EPS, c.ln, candidates=True)
            h, y = res
            same_bits(h, np.asarray(o["h"], F32), c.id + " h")
            assert np.all(np.abs(y.astype(np.float64) - o["y64"]) <= o["err"]), c.id + " y outside the oracle's bound"
            for r in range(c.rows):
                assert O.calib_norm_replay(y[r], o["h"][r], o["cand"][r], w, b, c.ln), "%s: no row statistic replays row %d" % (c.id, r)
            TC.check_stat(np.concatenate([after["in_min"], after["in_max"]]), [o["h"].min(), o["h"].max()], c.id + " h statistic")
            TC.check_stat(np.concatenate([after["out_min"], after["out_max"]]), [y.min(), y.max()], c.id + " y statistic")
            if c.slots:
                TC.check_stat(np.concatenate([after["delta_min"], after["delta_max"]]), [d.min(), d.max()], c.id + " delta statistic")
        return Built(args, dict(rows=c.rows, cols=c.cols, numel=c.rows * c.cols), check)
    return Case(c.id, build)


def _cgated_case(act, numel):
    def build():
        a, b = K.gated_base(numel)
        args = dict(a=np.array(a), b=np.array(b), act=("silu", "gelu")[act], stats=_slots(8))

        def check(res, after):
            import test_gpu_calib as TC                       # the bounds of test_calib_gated, none of them new
            wp, ws = O.calib_gated(a, b, act)
            err = np.abs(res.astype(np.float64) - wp)
            lever = 0.5 * np.abs(a.astype(np.float64) * b.astype(np.float64))
            assert np.all(err <= TC.PROD_ATOL + TC.PROD_RTOL * np.abs(wp) + (TC.GELU_ERF_ABS * lever if act == 1 else 0)), "product outside the pin's bound"
            st = np.concatenate(after["stats"])
            TC.check_stat(st[0:2], [a.min(), a.max()], "a statistic")
            TC.check_stat(st[4:6], [b.min(), b.max()], "b statistic")
            TC.check_stat(st[6:8], [res.min(), res.max()], "product statistic")
            lo, hi = ws.min(), ws.max()
            assert abs(float(st[2]) - lo) <= 1e-6 * max(1, abs(lo)) and abs(float(st[3]) - hi) <= 2e-6 * abs(hi), "act(a) statistic"
        return Built(args, dict(numel=numel), check)
    return Case("%s-%d" % (("silu", "gelu")[act], numel), build)


_STAT_OPS4 = [op(n, "inplace", "f32", "1") for n in _STAT4]
_PROBS = [c for c in K.PROBS_CASES if c.cols == 260 and c.rows == 6]                        # one with a mask, one without; 260 keys: a vector tail
_CAUSAL = [c for c in K.CAUSAL_CASES if (c.seq, c.blocks) == (100, 2)]
_CNORM = sorted((c for c in K.NORM_CASES if c.rows <= 64), key=lambda c: c.rows * c.cols)


def _pick_norm():
    """The smallest calibration norm cases that between them pass a delta with its slots, a delta without, no delta, a bias, both norms."""
    out, seen = [], set()
    for c in _CNORM:
        key = (c.ln, c.delta, c.slots, c.bias)
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


# ---- calibration: RoPE with its statistics ------------------------------------------------------------------------------------------------
def _rope_case(qkv):
    c = K.RopeCase("contract%s" % ("_qkv" if qkv else ""), 2, 5, 6, 3, 12, 8, qkv)        # head_dim 12, 8 rotated: pass-through lanes, an idle head slot

    def build():
        q, k, v, cos, sin = K.rope_input(c)
        rep = c.H // c.KV if qkv else 1
        ins = [q, k] + ([v] if qkv else [])
        want = [O.calib_rope(q, c.H, c.D, cos, sin), O.calib_rope(k, c.KV, c.D, cos, sin, True, rep)]
        if qkv:
            want.append(O.calib_rope(v, c.KV, c.D, cos, sin, False, rep))
        n = 10 if qkv else 8
        stats = [np.array([np.inf if i % 2 == 0 else -np.inf], F32) for i in range(n)]
        args = dict(q_lin=np.array(q), k_lin=np.array(k), heads=c.H, kv_heads=c.KV, head_dim=c.D, cos=np.array(cos), sin=np.array(sin), stats=stats)
        if qkv:
            args["v_lin"] = np.array(v)

        def check(res, after):
            # test_gpu_calib.test_calib_rope: the rotated tensors bit for bit, every statistic exact
            st = np.concatenate(after["stats"])
            for i, name in enumerate("qkv"[:len(ins)]):
                same_bits(res[i], want[i], "%s rotated %s" % (c.id, name))
                same_bits(st[4 * i:4 * i + 2], np.array([ins[i].min(), ins[i].max()], F32), "%s %s-linear statistic" % (c.id, name))
                if i < 2:
                    same_bits(st[4 * i + 2:4 * i + 4], np.array([want[i].min(), want[i].max()], F32), "%s rotated %s statistic" % (c.id, name))
        return Built(args, dict(B=c.B, S=c.S, H=c.H, KV=c.KV, D=c.D, rot=c.rot), check)
    return Case("B2S5H6KV3D12rot8", build)


def _rope_ops(qkv):
    ops_ = [op("q_lin", "raw", "f32", "B*S*H*D", "q"), op("k_lin", "raw", "f32", "B*S*KV*D", "k")]
    if qkv:
        ops_.append(op("v_lin", "raw", "f32", "B*S*KV*D", "v"))
    ops_ += [op("cos", "conv", "f32", "S*rot"), op("sin", "conv", "f32", "S*rot")]
    return ops_ + [op(("stats", i), "inplace", "f32", "1", r"stats\[%d\]" % i) for i in range(10 if qkv else 8)]


# ---- the table ------------------------------------------------------------------------------------------------------------------------
_X_ANY = ("f32", "f16")
_GEMM_OPS = [op("a_q", "raw", ("i8", "u8"), "Mp*K"), op("w_q", "raw", ("i8", "u8"), "N*Kw"), op("a_rowsum", "raw", "i32", "M"),
             op("alpha", "raw", "f32", "N"), op("w_zp", "raw", "i32", "N"), op("col_term", "raw", "i32", "N"),
             op("bias", "conv", "f32", None), op("out_scale", "conv", "f32", None), op("out_offset", "conv", "f32", None),
             op("out", "out", ("f32", "f16", "u8", "i8", "u16", "i16"), "M*N"), op("resid", "conv", "f32", "M*N")]

WRAPPERS = [
    Wrapper("scale_offset_from_minmax", [op("min_val", "conv", "f32", None), op("max_val", "conv", "f32", "n")], ("bitwidth", "is_symmetric"),
            [_so_case(8, False), _so_case(8, True), _so_case(16, False), _so_case(4, True)]),
    Wrapper("minmax_new", [], ("n", "device"), [_mm_new_case()]),
    Wrapper("minmax_tensor_", [op("x", "layout", _X_ANY, None), op("mn", "inplace", "f32", "1"), op("mx", "inplace", "f32", "1")], (),
            [_mm_inplace_case("tensor", "f32"), _mm_inplace_case("tensor", "f16")]),
    Wrapper("minmax_rows_", [op("x2d", "layout", _X_ANY, None, "x"), op("mn", "inplace", "f32", "rows"), op("mx", "inplace", "f32", "rows")], (),
            [_mm_inplace_case("rows", "f32"), _mm_inplace_case("rows", "f16")]),
    Wrapper("minmax_cols_", [op("x2d", "layout", _X_ANY, None, "x"), op("mn", "inplace", "f32", "cols"), op("mx", "inplace", "f32", "cols")], (),
            [_mm_inplace_case("cols", "f32"), _mm_inplace_case("cols", "f16")]),
    Wrapper("minmax_tensor", [op("x", "layout", _X_ANY, None)], (), [_mm_fresh_case("tensor", "f32"), _mm_fresh_case("tensor", "f16")]),
    Wrapper("minmax_rows", [op("x2d", "layout", _X_ANY, None, "x")], (), [_mm_fresh_case("rows", "f32"), _mm_fresh_case("rows", "f16")]),
    Wrapper("minmax_cols", [op("x2d", "layout", _X_ANY, None, "x")], (), [_mm_fresh_case("cols", "f32"), _mm_fresh_case("cols", "f16")]),
    Wrapper("fake_quant", [op("x", "layout", _X_ANY, None), op("scale", "conv", "f32", None), op("offset", "conv", "f32", "n_scale"),
                           op("out", "out", _X_ANY, "numel")], ("qmin", "qmax"),
            [_fq_case("f32-tensor", 3, 67, "f32", "h8", False), _fq_case("f32-row", 5, 68, "f32", "h8", True),
             _fq_case("f16-tensor", 3, 67, "f16", "h8", False), _fq_case("f16-row", 5, 72, "f16", "h8", True),
             _fq_case("f32-out", 3, 68, "f32", "h8", False, out=True), _fq_case("f16-out", 3, 72, "f16", "hw4", False, out=True)]),
    Wrapper("fake_quant_backward", [op("x", "conv", "f32", None), op("grad_y", "conv", "f32", "numel"), op("scale", "conv", "f32", None),
                                    op("offset", "conv", "f32", "n_scale")], ("qmin", "qmax"),
            [_fqb_case("tensor-1x1023", 1, 1023, 1, 3), _fqb_case("row-3x96", 3, 96, 3, 6)]),
    Wrapper("quantize", [op("x", "layout", _X_ANY, None), op("scale", "conv", "f32", None), op("offset", "conv", "f32", "n_scale"),
                         op("chan_scale", "conv", "f32", "cols")], ("qmin", "qmax", "q_dtype", "shift", "rows", "want_row_sum"),
            [_q_case("tensor-i8", 3, 67, "f32", "h8", 128, "i8"), _q_case("row-u8", 5, 68, "f32", "h8", 0, "u8", per_row=True),
             _q_case("row-sum-b16", 5, 272, "f32", "h8", 128, "i8", per_row=True, row_sum=True),
             _q_case("tensor-sum-f16", 3, 72, "f16", "h8", 128, "i8", row_sum=True), _q_case("chan", 5, 100, "f32", "u8", 128, "i8", chan=True),
             _q_case("chan-sum", 5, 101, "f32", "u8", 128, "i8", chan=True, row_sum=True), _q_case("u16", 3, 67, "f32", "u16", 0, "u16"),
             _q_case("i16", 5, 68, "f32", "i16", 0, "i16", per_row=True), _q_case("i32", 3, 67, "f32", "u16", 0, "i32", row_sum=True),
             _q_case("rows-arg", 6, 67, "f32", "h8", 128, "i8", rows_arg=True, row_sum=True)]),
    Wrapper("quantize_tiled", [op("x2d", "layout", _X_ANY, None, "x"), op("scale", "conv", "f32", "1"), op("offset", "conv", "f32", "1"),
                               op("chan_scale", "conv", "f32", "cols")], ("qmin", "qmax", "shift", "want_row_sum"),
            [_qt_case("7x128", 7, 128, "h8", 128), _qt_case("7x128-nosum", 7, 128, "h8", 128, row_sum=False),
             _qt_case("17x256-chan", 17, 256, "u8", 128, chan=True)]),
    Wrapper("linear_epilogue_prepare", [op("a_scale", "conv", "f32", "1"), op("a_offset", "conv", "f32", "1"), op("w_scale", "conv", "f32", None),
                                        op("w_offset", "conv", "f32", "n_w"), op("w_colsum", "raw", "i32", None)],
            ("a_shift", "w_shift", "K"), [_epi_case("tensor-257", 257, False), _epi_case("row-257", 257, True)]),
    Wrapper("pack_w4", [op("nibbles", "layout", "u8", None)], (), [_pack_case()]),
    Wrapper("act_quant", [op("x", "conv", "f32", None)] + grid_ops("in_grid") + grid_ops("mid_grid") + grid_ops("out_grid"), ("act",),
            [_act_case(0, True, True), _act_case(0, False, False), _act_case(1, False, True), _act_case(0, True, False, numel=7)]),
    Wrapper("gated_act_quant", [op("a", "layout", ("f32", "u8"), None, "a must|two float32"), op("b", "layout", ("f32", "u8"), "numel", "b must|two float32")]
            + _GATED_GRIDS, ("act", "q_shift", "want_y"),
            [_gated_case(0, True, False), _gated_case(0, True, True), _gated_case(0, False, True), _gated_case(1, False, False), _gated_case(1, True, True)]),
    Wrapper("gated_table", _GATED_GRIDS, ("act", "q_shift"), [_gated_table_case(0), _gated_table_case(1)]),
    Wrapper("gated_lookup", [op("a", "layout", "u8", None, "a must|two uint8"), op("b", "layout", "u8", "numel", "b must|two uint8"),
                             op("table", "raw", "i8", "65536")], ("tiled",), [_lookup_case(False), _lookup_case(True)]),
    Wrapper("int8_linear", _GEMM_OPS, ("out_qmin", "out_qmax", "out_dtype", "w4", "a_tiled_rows"),
            [_gemm_case("plain-u8", "linear", ROWMAJOR, "u8"), _gemm_case("plain-u8-out", "linear", ROWMAJOR, "u8", out=True),
             _gemm_case("plain-f32-16", "linear", ROWMAJOR, "f32_16"),
             _gemm_case("plain-none16", "linear", ROWMAJOR, "none16"), _gemm_case("w4-u8", "linear", ROWMAJOR, "u8", w4=True),
             _gemm_case("tiled-u8", "tiled", FR128, "u8"), _gemm_case("resid", "linear_residual", ROWMAJOR, "f32_16"),
             _gemm_case("resid-none", "linear_residual", ROWMAJOR, "none32"), _gemm_case("resid-tiled", "tiled_residual", FR128, "f32_16")]),
    Wrapper("int8_linear_segmented", _GEMM_OPS[:7] + _seg_grid_ops(), ("seg_ends", "w4", "a_tiled_rows"),
            [_seg_case("rowmajor", "segmented", SEG_ROWMAJOR, SEGS), _seg_case("w4", "segmented", SEG_ROWMAJOR, SEGS, w4=True),
             _seg_case("tiled", "tiled_segmented", FR128, (44, 84, FR128[1]))]),
    Wrapper("w4a8_linear_tiled", [op("a_tiled", "raw", ("i8", "u8"), "Mp*K"), op("w_packed", "raw", ("i8", "u8"), "N*Kw")] + _GEMM_OPS[2:7]
            + _seg_grid_ops() + [op("out", "out", ("u8", "i8"), "M*N")], ("M", "seg_ends", "out_dtype"),
            [_seg_case("one-grid-out", "tiled_w4", FRW4, None, wrapper="w4", out=True), _seg_case("segs-i8", "tiled_w4", FRW4, (44, 84, FRW4[1]), "i8u", wrapper="w4")]),
    Wrapper("int8_linear_f32in", [op("x2d", "conv", "f32", None, "x"), op("a_scale", "conv", "f32", None), op("a_offset", "conv", "f32", None),
                                  op("w_q", "raw", ("i8", "u8"), "N*Kw")] + _GEMM_OPS[3:10],
            ("a_qmin", "a_qmax", "a_shift", "out_qmin", "out_qmax", "out_dtype", "w4"),
            [_f32in_case("w8-u8-out", "w8a8_f32in", 5, 72, 256, "u8", "u8", out=True), _f32in_case("w4-f32-16", "w4a8_f32in", 3, 72, 256, "f32_16", "s8"),
             _f32in_case("w8-none32", "w8a8_f32in", 8, 72, 512, "none32", "s8")]),
    Wrapper("int8_linear_pair", _pair_ops(False), ("rows", "out_dtype"), [_pair_case(False)]),
    Wrapper("int8_linear_gated", _pair_ops(True), ("rows", "w4"), [_pair_case(True)]),
    Wrapper("attention_quant", _attq_ops(), ("heads", "kv_heads", "want_out", "head_dim", "pos0", "f16"),
            [_attq_case("image"), _attq_case("image-tiled", tiled=True), _attq_case("qkv-idx", idx_inputs=True), _attq_case("cache-pos0", cache=True)]),
    Wrapper("attention_cache_import", _cache_ops("inplace", True) + [op("k", "raw", "i8", "KLD", "k|decode caches"), op("v", "raw", "i8", "KLD", "v|decode caches")]
            + [op(("grids", n, j), "conv", "f32", "1", ("scale|per-tensor", "offset|per-tensor")[j]) for n in ("qk_a", "qk_b") for j in range(2)],
            ("n", "v_chunked", "k_f16_exact"), [_import_case(False), _import_case(True)]),
    Wrapper("attention_cache_export", _cache_ops("raw", True) + [op("k", "out", "i8", "KLD", "k|decode caches"), op("v", "out", "i8", "KLD", "v|decode caches")],
            ("p0", "n", "v_chunked"), [_export_case(False), _export_case(True)]),
    Wrapper("int8_linear_grouped", [op("a_q", "raw", ("i8", "u8"), "M*K"), op("w_q", "raw", ("i8", "u8"), "N*K"), op("a_gsum", "raw", "i32", "G*M"),
                                    op("alpha", "conv", "f32", "G*N"), op("cw", "raw", "i32", "G*N"), op("t", "raw", "i32", "G*N"),
                                    op("bias", "conv", "f32", None)], ("group_size",), [_grouped_case("g64-G2"), _grouped_case("g128-G2-M1")]),
    Wrapper("attention_probs_train", _attn_ops(False), ("sqrt_d",), [_attn_case(c, False) for c in _ATTN]),
    Wrapper("attention_probs_train_backward", _attn_ops(True), ("sqrt_d",), [_attn_case(c, True) for c in _ATTN]),
    Wrapper("rmsnorm_quant", [op("x", "conv", "f32", None), op("weight", "conv", "f32", "cols"), op("bias", "conv", "f32", "cols")]
            + grid_ops("in_grid", "in_scale", "in_offset") + grid_ops("out_grid", "out_scale", "out_offset"),
            ("eps", "emit_int8", "layernorm", "emit_tiled", "want_y", "emit_rowmajor"),
            [_norm_case("rms-y16", ("rowmajor", 60, P.NORM_ROWS, False, True, True, 16)),
             _norm_case("layernorm-int8", ("rowmajor", 60, P.NORM_ROWS, True, False, False, 8), emit_int8=True),
             _norm_case("rms-int8-in", ("rowmajor", 1028, P.NORM_ROWS, False, True, True, 8), emit_int8=True),
             _norm_case("rms-tiled", ("generic-tiled",) + P.GENERIC_TILED + (False,), emit_int8=True, emit_tiled=True),
             _norm_case("layernorm-tiled-only", ("generic-tiled",) + P.GENERIC_TILED + (True,), emit_int8=True, emit_tiled=True, want_y=False,
                        emit_rowmajor=False)]),
    Wrapper("qmatmul", [op("x1", "layout", "f32", None, "x1|float32 operands"), op("x2", "layout", "f32", None, "x2|float32 operands")]
            + grid_ops("grid1", "grid scale|per-tensor", "grid offset|per-tensor") + grid_ops("grid2", "grid scale|per-tensor", "grid offset|per-tensor")
            + grid_ops("grid_out", "grid scale|per-tensor", "grid offset|per-tensor"), (),
            [_qmm_case("kT-transposed-view", "tile-kT-nothing-divides", "transposed-view"), _qmm_case("kT-dense-copied", "tile-kT-nothing-divides", "dense"),
             _qmm_case("kT-sliced-copied", "tile-kT-nothing-divides", "sliced"), _qmm_case("kn-dense", "tile-kn-K9", "dense"),
             _qmm_case("kn-transposed-view", "tile-kn-K9", "transposed-view"), _qmm_case("kn-sliced-copied", "tile-kn-K9", "sliced"),
             _qmm_case("out-grid-dense", "tile-fits32-offsets", "dense"), _qmm_case("out-grid-view", "tile-fits32-offsets", "transposed-view")]),
    Wrapper("score_head", [op("y", "layout", "f32", None), op("weight", "conv", "f32", None), op("bias", "conv", "f32", "V"),
                           op("targets", "layout", "i64", "M")], (),
            [_score_case("7x128x97-bias-targets", 7, 128, 97, True, True), _score_case("3x64x160", 3, 64, 160, False, False)]),
    Wrapper("attention_image_cache", [], ("kv_heads", "head_dim", "max_len", "device"), [_image_cache_case()]),
    Wrapper("attention_f16_offsets_ok", [], ("offsets",), [_f16_ok_case()]),
    Wrapper("hist_new", [], ("n_slots", "mantissa_bits", "device"), [_hist_new_case()]),
    Wrapper("hist_minmax_tensor_", [op("t", "layout", _X_ANY, None, "x"), op("counts_row", "inplace", "i64", "NB2"), op("nan_row", "inplace", "i64", "1"),
                                    op("mn", "inplace", "f32", "1"), op("mx", "inplace", "f32", "1")], ("mantissa_bits",),
            [_hist_case(False, 0), _hist_case(True, 2), _hist_case(False, 1, minmax=False)]),
    Wrapper("lwc_search", [op("w2d", "raw", "f32", None), op("sig_lo", "raw", "f32", None), op("sig_hi", "raw", "f32", "C", "sig_hi|candidate tables"),
                           op("col_weight", "raw", "f32", None)], ("bitwidth", "is_symmetric", "return_costs"),
            [_lsearch_case("8x16-plain", 8, 16, 4, False, 8, None, False), _lsearch_case("5x128-row-costs", 5, 128, 4, True, 8, "row", True),
             _lsearch_case("6x132-grouped", 6, 132, 8, False, 5, "grouped", True)]),
    Wrapper("calib_attention_probs_", [op("raw", "inplace", "f32", None, "raw|score tensor"), op("mask", "raw", "f32", "S*T")] + _STAT_OPS4, ("sqrt_d",),
            [_probs_case(c) for c in _PROBS], aliases=((0, 1),)),              # raw is passed as input and as output: in place
    Wrapper("calib_attention_probs_causal_", [op("raw", "raw", "f32", None, r"raw|S, S\] tensors"), op("out", "out", "f32", "numel", r"out|S, S\] tensors")] + _STAT_OPS4,
            ("sqrt_d", "store_masked"), [_probs_case(c, True, sm) for c in _CAUSAL for sm in (True, False)]),
    Wrapper("calib_norm_", [op("x", "raw", "f32", None, "x must|tensors of one shape"), op("delta", "raw", "f32", "numel", "delta|tensors of one shape"),
                            op("weight", "conv", "f32", "cols"),
                            op("bias", "conv", "f32", "cols")] + [op(n, "inplace", "f32", "1") for n in
                                                                   ("in_min", "in_max", "out_min", "out_max", "delta_min", "delta_max")],
            ("eps", "layernorm"), [_cnorm_case(c) for c in _pick_norm()]),
    Wrapper("calib_gated_", [op("a", "raw", "f32", None), op("b", "raw", "f32", "numel")]
            + [op(("stats", i), "inplace", "f32", "1", r"stats\[%d\]" % i) for i in range(8)], ("act",),
            [_cgated_case(0, K.GATED_SIZES[1]), _cgated_case(1, K.GATED_SIZES[1])]),
    Wrapper("calib_rope_", _rope_ops(False), ("heads", "kv_heads", "head_dim"), [_rope_case(False)]),
    Wrapper("calib_rope_qkv_", _rope_ops(True), ("heads", "kv_heads", "head_dim"), [_rope_case(True)]),
    Wrapper("lwc_fake_quant", [op("w", "conv", "f32", None), op("sig_lo", "conv", "f32", "N", "sig_lo|bound factor"), op("sig_hi", "conv", "f32", "N", "sig_hi|bound factor")],
            ("bitwidth", "is_symmetric"), [_lwc_case(4, False), _lwc_case(8, True)]),
    Wrapper("lwc_fake_quant_backward", [op("w", "conv", "f32", None), op("grad_out", "conv", "f32", "numel"), op("sig_lo", "conv", "f32", "N", "sig_lo|bound factor"),
                                        op("sig_hi", "conv", "f32", "N", "sig_hi|bound factor"), op("row_min", "raw", "f32", "N"), op("row_max", "raw", "f32", "N")],
            ("bitwidth", "is_symmetric"), [_lwc_bwd_case(4, False), _lwc_bwd_case(8, True)]),
]
BY_NAME = {w.name: w for w in WRAPPERS}

# These pass a filled struct straight through, or refuse on their own with tests of their own.
EXEMPT = {
    "decode_gemv_grouped": "passes a filled MqDecodeGemvGroupedArgs through; the C entry validates it (test_gpu_decode_grouped.py)",
    "decode_attention_multi": "passes a filled MqDecodeAttentionMultiArgs through; the C entry validates it (test_gpu_decode_multi.py)",
    "decode_attention_ragged": "passes a filled MqDecodeAttentionRaggedArgs through; the C entry validates it (test_gpu_decode_ragged.py)",
    "decode_cache_table": "refusals in test_gpu_decode_fork.py",
    "decode_cache_fork": "refusals in test_gpu_decode_fork.py",
    "decode_cache_reorder": "refusals in test_gpu_decode_reorder.py",
    "beam_select": "refusals in test_gpu_beam_select.py",
}
# ... and the names ops.py only re-exports: they are functions of sampling.py, which builds and validates its own argument blocks
# (_lib.call is made there, not in ops.py), with refusal tests in test_gpu_sample.py, test_gpu_sample_penalty.py and test_gpu_logprob.py.
REEXPORTED = {name: "defined in mobilequant_amd/sampling.py and re-exported; its argument checks and their tests live with it"
              for name in ("sample_history_count", "sample_history_count_ragged", "sample_history_prompt", "sample", "sample_ragged", "sample_rows",
                           "sample_uniforms", "logprob_top")}

# The predicates: no pointer goes anywhere; test_gpu_ops_contract.py violates each condition of their bodies once and follows a True with
# the call it promises.
PREDICATES = ("lwc_fake_quant_supported", "attention_probs_train_supported", "qmatmul_supported", "gemm_tiled_supported", "gemm_tiled128_supported",
              "gemm_tiled_w4_supported", "decode_shape")

def all_cases():
    """(wrapper, case) of every valid call in the table."""
    return [(w, c) for w in WRAPPERS for c in w.cases]


def sizes_numel(expr, sizes):
    return int(eval(expr, {"__builtins__": {}}, dict(sizes)))          # the table's own expressions: products of the call's sizes
