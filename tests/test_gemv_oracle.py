"""CPU: the oracle of the M <= 8 weight-streaming GEMV (oracle.linear_gemv_launch) and the case lists of gemv_cases.py, held to what
test_gpu_linear_gemv.py relies on -- without a GPU.

  * every case: exact ties of both parities, near-ties, both clamps and the steps around them, accumulators beyond 2^24 whose
    conversion rounds, sums that wrap in int32, zero points at both extremes, a caller's row sum that is off or NULL;
  * the fused cases' activations: ties of x / s of both parities and their ulp neighbours, both clamps, NaN / +-inf / -0.0, on the
    grid 0..255 with shift 128 and on -128..127 with shift 0;
  * the geometry, restated at 256 CUs: every branch class is reached, and every one of the twelve instantiations meets every output
    grid, a multi-pass row and a ragged last workgroup;
  * the oracle against the older ones: qlinear_int_exact without a grid, _fq_recip on the fake-quant outputs, decode_gemv_epilogue
    on single-token cases, quantize_storage on the fused image;
  * every mutation of the oracle changes a stored element in every case it can bear on (gemv_cases.MUTATION_BEARS says which and why);
  * the M = 8 / M = 9 seam: linear_gemv_launch against prefill_gemm_epilogue on the same accumulators, per column class."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gemv_cases as C  # noqa: E402
from oracle import mq_oracle as O  # noqa: E402
from test_gpu_parity import _int_problem  # noqa: E402

F32 = np.float32
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32}


def _bits(a):
    return a.view(UINT[a.dtype.itemsize])


@pytest.fixture(scope="module", params=C.ALL_CASES, ids=lambda c: c.id)
def case(request):
    return request.param


# ---- every case -----------------------------------------------------------------------------------------------------------------
def test_case_conditions(case):
    c = case
    k = C.conditions(c)
    g = C.GRIDS[c.grid]
    assert C.takes_gemv(c.M, c.K) and (not C.fuse_of(c) or C.f32in_accepts(c.M, c.K))
    if not C.fuse_of(c):
        assert (k["rowsum_off"] > 0) == (c.rowsum != "true"), k
    if c.N < C.COL_PERIOD:
        return                                                     # (four columns: the geometry case, tie columns only)
    assert k["big"] > 0 and k["big_rounds"] > 0 and k["wraps"] > 0, k
    assert k["zp_hi"] > 0 and k["zp_lo"] > 0, k
    if g is None:
        return
    if c.p2:
        assert k["tie_even"] > 0 and k["tie_odd"] > 0, k
        assert not c.bias or k["near_tie"] > 0, k
    assert k["sat_lo"] > 0 and (c.M < 2 or k["sat_hi"] > 0), k
    if c.M > C.ZERO_ROW:                                # the zero row: tt = col_term = 0 in the sat columns
        assert all(k[s] > 0 for s in ("lo-1", "lo", "lo+1", "hi-1", "hi", "hi+1")), k


def test_fused_image(case):
    """The image the oracle feeds the contraction is quantize_storage's, and the adversarial activations sit where they should."""
    c = case
    if not C.fuse_of(c):
        return
    p, e = C.problem(c), C.expect(c)
    s, o, qmin, qmax, shift = p.agrid
    stored, rs = O.quantize_storage(p.x, s, o, qmin, qmax, shift)
    assert np.array_equal(e["image"], stored) and np.array_equal(e["rs"], rs.astype(np.int64))
    sp = C.specials(c.agrid)
    pos = C.special_positions(c.K, len(sp))
    names = [n for n, _ in sp]
    assert {"tie_even", "tie_odd", "tie_ulp_in", "tie_ulp_out", "lo_out", "lo_on", "hi_on", "hi_out", "nan", "pinf", "ninf", "negzero"} <= set(names)
    for m in range(c.M):
        if C.ROW_CLASS[m] == "zero":
            assert not e["image"][m].any()
            continue
        for (name, x), k in zip(sp, pos):
            got = int(e["image"][m, k])
            if name in ("nan", "pinf", "ninf", "lo_out", "lo_on", "lo_far"):
                assert got == qmin - shift, (name, got)
            elif name in ("hi_on", "hi_out", "hi_far"):
                assert got == qmax - shift, (name, got)
            elif name == "negzero":
                assert got == int(o) - shift
            elif name.startswith("tie_e") or name.startswith("tie_o"):
                t = float(F32(x) / F32(s))
                assert t - np.floor(t) == 0.5
                even = np.floor(t) if np.floor(t) % 2 == 0 else np.floor(t) + 1
                assert got == int(even + float(o)) - shift, (name, t, got)
                assert (np.floor(t) % 2 == 0) == (name == "tie_even")


def test_mutations_change_what_they_bear_on(case, monkeypatch):
    c = case
    e = C.expect(c)
    real, memo = O._contract_rows, {}

    def cached(image, w, w4=False, block=16384):                    # (the contraction is not what the mutations touch)
        key = (id(w), w4)
        if key not in memo:
            memo[key] = real(image, w, w4, block)
        return memo[key]
    monkeypatch.setattr(O, "_contract_rows", cached)
    for name in O.LINEAR_GEMV_MUTATIONS:
        if not C.MUTATION_BEARS[name](c):
            continue
        m = O.linear_gemv_launch(mutation=name, **C.oracle_args(c))
        assert (_bits(m["stored"]) != _bits(e["stored"])).any(), "%s: mutation %s changes nothing" % (c.id, name)


def test_every_mutation_bears_on_cases_of_every_instantiation():
    for name in O.LINEAR_GEMV_MUTATIONS:
        insts = {C.instantiation(c) for c in C.ALL_CASES if C.MUTATION_BEARS[name](c)}
        if name == "divide":                                        # (bound to show only on 16 384 or more 16-bit outputs: the large cases)
            assert len([c for c in C.ALL_CASES if C.MUTATION_BEARS[name](c)]) >= 3 and len(insts) >= 2, (name, insts)
            continue
        want = {i for i in C.INSTANTIATIONS if not (name == "rowsum_recomputed" and i[1])}       # (the fused entries own their row sum)
        assert insts == want, (name, sorted(want - insts))


# ---- the lists ------------------------------------------------------------------------------------------------------------------
def test_geometry_classes_and_instantiations_at_256_cus():
    reached, per_inst, grids = {}, {i: set() for i in C.INSTANTIATIONS}, {i: set() for i in C.INSTANTIATIONS}
    for c in C.ALL_CASES:
        for k in C.geometry_classes(c):
            reached.setdefault(k, c.id)
        per_inst[C.instantiation(c)] |= C.geometry_classes(c)
        grids[C.instantiation(c)].add(c.grid)
    assert not [k for k in C.GEOMETRY_CLASSES if k not in reached]
    for i in C.INSTANTIATIONS:
        assert {"multi_pass", "odd_phase", "ragged_last_wg"} <= per_inst[i], i
        assert grids[i] == set(C.GRIDS), (i, set(C.GRIDS) - grids[i])
    assert {c.M for c in C.ALL_CASES} == set(range(1, 9))
    assert {c.M for c in C.ALL_CASES if "multi_pass" in C.geometry_classes(c)} >= {1, 2, 3, 6, 7}
    assert {c.rowsum for c in C.ALL_CASES} == {None, "true", "off", "null"}
    assert {(c.agrid, C.A_GRIDS[c.agrid][4]) for c in C.ALL_CASES if c.agrid} == {("u8", 128), ("s8", 0)}
    assert {C.storage_of(c) for c in C.ALL_CASES} == {"u8", "i8", "u16", "i16", "f32", "f16"}


def test_the_shapes_the_issue_names():
    by = {(c.entry, c.M, c.N, c.K): C.geometry(c) for c in C.ALL_CASES}
    assert by[("w8a8", 1, 4100, 8320)].cpl == 9 and by[("w4a8", 3, 4100, 16640)].cpl == 9
    assert by[("w8a8", 1, 4100, 8320)].passes_per_row == 2          # 9 chunks: every row ends in the pass after the one it starts in
    assert by[("w8a8", 3, 4100, 16384)].cpl == 16 and by[("w8a8", 7, 580, 8192)].cpl == 8
    assert by[("w8a8", 1, 180, 65408)].cpl == 64 and 65408 <= C.LDS_LIMIT < 65408 + 128                # the largest K % 128 == 0 under the limit
    assert by[("w4a8", 2, 180, 128)].kchunks == 4
    g = by[("w8a8", 2, 258052, 128)]
    assert (g.rows_per_wg, g.nslots, g.grid) == (1009, 64, 256)
    g = by[("w8a8_f32in", 1, 262152, 256)]
    assert (g.rows_per_wg, g.nslots, g.grid) == (1024, 64, 257)
    assert by[("w8a8", 2, 32772, 256)].nslots == 9
    assert by[("w8a8", 1, 4, 128)].grid == 4 and by[("w8a8", 1, 4, 128)].rows_per_wg == 1
    for M, K in C.OVER_LIMIT:
        assert not C.takes_gemv(M, K) and C.takes_gemv(M, K - 256)
    assert C.f32in_accepts(7, 9216) and not C.f32in_accepts(7, 9472) and not C.f32in_accepts(8, 8192)
    assert C.locate(C.GEOMETRY_CASES[9], 4099) == (241, 2, 0, 1, 0)  # the ragged last workgroup: 3 rows, one slot, done in pass 1


# ---- the oracle against the older ones ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 64, 128), (5, 180, 256), (8, 260, 384)])
@pytest.mark.parametrize("per_row", [False, True])
def test_without_grid_is_qlinear_int_exact(shape, per_row):
    M, N, K = shape
    rng = np.random.default_rng(M * 7 + N)
    qa, qw, za, zw, sa, sw, bias = _int_problem(rng, M, N, K, per_row)
    _, want = O.qlinear_int_exact(qa, za, sa, qw, zw, sw, bias)
    a8, w8 = (qa - 128).astype(np.int8), (qw - 128).astype(np.int8)
    alpha, w_zp, ct = O.linear_epilogue_vectors(np.array([sa], F32), np.array([za], F32), 128, np.asarray(sw, F32), np.asarray(zw, F32), 128,
                                                w8.astype(np.int64).sum(axis=1), K)
    rs = a8.astype(np.int64).sum(axis=1).astype(np.int32)
    got = O.linear_gemv_launch(w8, alpha, w_zp, ct, bias, a=a8, a_rowsum=rs)
    assert np.array_equal(_bits(got["stored"]), _bits(want))
    half = O.linear_gemv_launch(w8, alpha, w_zp, ct, bias, a=a8, a_rowsum=rs, out_dtype="f16")
    assert np.array_equal(_bits(half["stored"]), _bits(want.astype(np.float16)))
    # the same launch on the prefill GEMM's oracle: without a grid the two epilogues are the same two roundings
    t = O.prefill_gemm_acc(a8, w8, rs, w_zp, ct)
    assert np.array_equal(t, got["tt"])
    assert np.array_equal(_bits(O.prefill_gemm_epilogue(t, alpha, bias)[0]), _bits(got["stored"]))


def test_dequantised_outputs_are_fq_recip_and_single_rows_the_decode_epilogue(case):
    c = case
    g = C.GRIDS[c.grid]
    if g is None or g.storage not in ("f32", "f16"):
        return
    p, e = C.problem(c), C.expect(c)
    q = O.quantizer_oracle_from(p.out_grid[0], p.out_grid[1], g.qmin, g.qmax)
    want = O._fq_recip(e["f"], q)
    assert np.array_equal(_bits(e["stored"]), _bits(want.astype(e["stored"].dtype)))
    if c.M == 1 and g.storage == "f32":
        sums = O.decode_gemv_sums(e["image"][0], p.w_packed if C.w4_of(c) else p.w, C.w4_of(c))
        d = O.decode_gemv_epilogue(sums, int(e["rs"][0]), p.alpha, p.w_zp, p.col_term, p.bias, out_grid=(q, None, None))
        assert np.array_equal(d["tt"], e["tt"][0]) and np.array_equal(_bits(d["y"]), _bits(e["stored"][0]))


# ---- the seam -------------------------------------------------------------------------------------------------------------------
FOLDED_ODD = ("u8", "i8u", "u4", "f32_8", "f16_8")                  # 8-bit grids: the GEMM adds the (odd) offset in front of its rint


def seam_shares(cases):
    """{(grid class, p2, column class): [differing, all]} of linear_gemv_launch against prefill_gemm_epilogue on the same tt."""
    out = {}
    for c in cases:
        g = C.GRIDS[c.grid]
        p, e = C.problem(c), C.expect(c)
        stored, _, _ = O.prefill_gemm_epilogue(e["tt"], p.alpha, p.bias, None if g is None else [(p.out_grid[0], p.out_grid[1])], None,
                                               0 if g is None else g.qmin, 255 if g is None else g.qmax, C.storage_of(c))
        d = _bits(stored) != _bits(e["stored"])
        kind = "none" if g is None else "8-bit, odd offset folded" if c.grid in FOLDED_ODD else "s8, offset 0" if c.grid == "s8" else "16-bit"
        cls = C.col_classes(c.N)
        for k in ("tie", "near", "generic", "sat", "big"):
            v = out.setdefault((kind, c.p2, k), [0, 0])
            v[0] += int(d[:, cls == k].sum())
            v[1] += int(d[:, cls == k].size)
        if g is not None and c.p2 and c.grid in FOLDED_ODD:         # an exact tie h: rint(h) + o against rint(h + o), o odd -- always one apart
            inside = (e["tie"] == 0) & (np.floor(e["v"]) + g.offset >= g.qmin) & (np.floor(e["v"]) + 1 + g.offset <= g.qmax)
            inside &= (cls == "tie")[None, :]
            assert inside.any() and d[inside].all(), c.id
    return out


def test_seam_between_the_gemv_and_the_gemm_form():
    sh = seam_shares(C.TYPE_CASES)
    for (kind, p2, k), (diff, total) in sorted(sh.items()):
        print("seam  %-26s %-4s %-8s %6d of %7d  %.4f" % (kind, "p2" if p2 else "", k, diff, total, diff / total))
    for (kind, p2, k), (diff, total) in sh.items():
        if kind == "none":
            assert diff == 0, (kind, p2, k)                         # the same two roundings
        if p2 and k == "tie" and kind in ("16-bit", "s8, offset 0"):
            assert diff == 0, (kind, p2, k)                         # every step exact in both forms, the offset added behind the rint or 0
    assert any(diff > 0 for (kind, p2, k), (diff, _) in sh.items() if k == "near")
    assert any(diff > 0 for (kind, p2, k), (diff, _) in sh.items() if k == "near" and kind == "16-bit" and not p2)
