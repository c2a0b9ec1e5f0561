"""CPU: the oracle of the quantize-to-integer pin (oracle.quantize_storage / tiled_offset / tiled_image_bytes / linear_epilogue_vectors /
fake_quant_f16_per_row) against the frozen reference outputs and against independent restatements, and the case lists of
quantize_cases.py against the dispatch code: every branch test_gpu_quantize.py has to reach is named here with the predicate that
reaches it, so a case list that stops reaching one fails without a GPU."""
import numpy as np
import torch

import quantize_cases as C
from conftest import load_meta, load_npz
from oracle import mq_oracle as O
from test_gpu_round2 import tiled_image

F32 = np.float32


# ---- the oracle ---------------------------------------------------------------------------------------------------------------
def test_quantize_storage_reproduces_the_frozen_indices():
    """The `_q` arrays of quantizer_cases.npz (the reference's own indices, torch CPU), every fp32 case, with the frozen grid: per-tensor
    and per-row, 4 / 8 / 16 bits, with a shift and without."""
    z = load_npz("quantizer_cases.npz")
    n = 0
    for m in load_meta(z):
        if m["dtype"] != "float32":
            continue
        k = m["id"]
        x, want = z[k + "_x"], z[k + "_q"]
        sc, of = z[k + "_scale"].reshape(-1), z[k + "_offset"].reshape(-1)
        rows = sc.size if sc.size > 1 else int(np.prod(x.shape[:-1]))
        x2 = x.reshape(rows, -1)
        assert np.all(np.isfinite(want))
        for shift in (0, 128):
            st, rs = O.quantize_storage(x2, sc, of, m["qmin"], m["qmax"], shift)
            assert np.array_equal(st + shift, want.reshape(rows, -1).astype(np.int64)), m["tag"]
            assert np.array_equal(rs.astype(np.int64), (want.reshape(rows, -1).astype(np.int64) - shift).sum(axis=1)), m["tag"]
        n += 1
    assert n == 39


def test_quantize_storage_rules():
    """Non-finite inputs and overflowing quotients store qmin - shift; fp16 is widened, not computed in half; chan_scale rounds the
    quotient to fp32 first; half-step ties go to the even index."""
    s, o = F32(0.0031), F32(5.0)
    x = np.array([[np.nan, np.inf, -np.inf, C.FLT_MAX, -C.FLT_MAX, 0.0, -0.0, 1e-40]], F32)
    st, rs = O.quantize_storage(x, [s], [o], 0, 255, 128)
    assert st.tolist() == [[-128] * 5 + [5 - 128] * 3] and rs.tolist() == [5 * -128 + 3 * (5 - 128)]
    ties = ((np.arange(10, 20) + 0.5 - 121.0) * 0.25).astype(F32)[None, :]              # exact in fp32: true ties
    st, _ = O.quantize_storage(ties, [0.25], [121.0], 0, 255, 0)
    assert st.tolist() == [[11, 11, 13, 13, 15, 15, 17, 17, 19, 19]]        # rint(-110.5) = -110, rint(-109.5) = -110: even QUOTIENTS
    xh = np.array([[0.1234, 3.3, -2.7]], np.float16)
    assert np.array_equal(O.quantize_storage(xh, [0.031], [121.0], 0, 255, 128)[0], O.quantize_storage(xh.astype(F32), [0.031], [121.0], 0, 255, 128)[0])
    xs, cs = np.array([[1.0, 0.7]], F32), np.array([3.0, 1.1], F32)
    twice = O.quantize_storage((xs / cs).astype(F32), [0.031], [121.0], 0, 255, 128)[0]
    assert np.array_equal(O.quantize_storage(xs, [0.031], [121.0], 0, 255, 128, cs)[0], twice)


def test_tiled_image_bytes_is_the_permute_form_and_a_bijection():
    rng = np.random.default_rng(5)
    for rows, cols in ((7, 128), (33, 1152), (80, 640)):
        a = rng.integers(-128, 128, (rows, cols)).astype(np.int8)
        img, real = O.tiled_image_bytes(a, rows, cols)
        mp = (rows + 15) // 16 * 16
        assert img.shape == real.shape == (mp * cols,)
        assert np.array_equal(img, tiled_image(a).reshape(-1)), (rows, cols)
        # a bijection onto the real-row bytes: rows * cols distinct offsets, inside the image, and the padding rows take the others
        r, k = np.meshgrid(np.arange(mp), np.arange(cols), indexing="ij")
        off = O.tiled_offset(r, k, cols)
        assert np.array_equal(np.sort(off.reshape(-1)), np.arange(mp * cols))
        assert int(real.sum()) == rows * cols and np.array_equal(np.sort(off[:rows].reshape(-1)), np.flatnonzero(real))
        assert O.tiled_offset(17, 70, cols) == ((cols >> 6) + 1) * 1024 + 16 * 1 + 6


def test_linear_epilogue_vectors_wrap_like_int64():
    up = down = 0
    for tag, c in C.all_epilogue_cases():
        alpha, w_zp, col = O.linear_epilogue_vectors(**c)
        za = np.int64(int(c["a_offset"][0]) - c["a_shift"])
        zw = np.broadcast_to(c["w_offset"].astype(np.int64) - c["w_shift"], col.shape)
        full = -za * c["w_colsum"].astype(np.int64) + np.int64(c["K"]) * za * zw                  # |.| < 2^63: no wrap in int64
        assert np.array_equal(col, full.astype(np.uint64).astype(np.uint32).view(np.int32)), tag
        assert np.array_equal(w_zp, zw.astype(np.int32)) and alpha.dtype == F32
        assert np.array_equal(alpha, np.broadcast_to(c["a_scale"] * c["w_scale"], alpha.shape))
        up += int((full > 2 ** 31 - 1).sum())
        down += int((full < -2 ** 31).sum())
    assert up > 0 and down > 0, "col_term has to wrap in both directions"
    assert max(c["K"] for _, c in C.all_epilogue_cases()) == (1 << 24) - 1


def test_fake_quant_f16_per_row_matches_torch_cpu():
    """torch promotes half x with a [rows, 1] fp32 grid to fp32 and the caller casts back once (qmodule.py:286-295)."""
    for c in C.FAKE_QUANT_CASES:
        if c.dtype != "f16" or not c.per_row:
            continue
        x, sc, of, qmin, qmax = C.fake_quant_inputs(c)
        xt, s, o = torch.from_numpy(np.array(x)), torch.from_numpy(np.array(sc)).reshape(-1, 1), torch.from_numpy(np.array(of)).reshape(-1, 1)
        t = xt / s
        q = torch.clamp(((t.round() - t) + t) + o, qmin, qmax)
        want = ((q - o) * s).to(torch.float16).numpy()
        got = C.fake_quant_expect(c)
        nan = np.isnan(want)
        assert nan.any() and np.array_equal(np.isnan(got), nan)
        assert np.array_equal(got[~nan].view(np.uint16), want[~nan].view(np.uint16)), c.id


# ---- the inputs ---------------------------------------------------------------------------------------------------------------
def test_inputs_hold_the_ties_and_stay_in_the_domain():
    for grid in C.GRIDS:
        x, sc, of, qmin, qmax = C.make_input(9, 1040, grid)
        s = float(sc[0])
        assert np.log2(s) != np.round(np.log2(s)) and 2.0 ** -60 <= s <= 2.0 ** 60
        t = x.astype(np.float64) / s
        assert np.all(np.isfinite(x)) and np.abs(t).max() <= 1e30
        t32 = (x / sc[0]).astype(F32).astype(np.float64)                             # the fp32 quotient the reference rounds
        exact = t32[t32 - np.floor(t32) == 0.5]                                      # exact ties of it ...
        assert exact.size >= 8 and {0, 1} <= set((np.floor(exact).astype(np.int64) & 1).tolist())        # ... of both parities
        idx = O.quantize_index(x, sc, of, qmin, qmax)
        assert (idx == qmin).any() and (idx == qmax).any() and (x == 0).any()
        assert t.min() + float(of[0]) < qmin - 0.25 * (qmax - qmin) and t.max() + float(of[0]) > qmax + 0.25 * (qmax - qmin)
        if grid != "i16" and grid != "u16":
            assert (np.abs(x[x != 0]) < 1e-38).any()                                 # denormals
    x, sc, _, _, _ = C.make_input(5, 272, "clamp", nonfinite=True)
    assert np.isnan(x).any() and np.isposinf(x).any() and np.isneginf(x).any() and (x == C.FLT_MAX).any() and (x == -C.FLT_MAX).any()
    for r in (0, 4):
        assert not np.isfinite(x[r, [0, 3, 4, 15, 16, 255, 256, 271]]).all() or (np.abs(x[r, [0, 3, 4, 15, 16, 255, 256, 271]]) == C.FLT_MAX).any()
    x, _, _, _, _ = C.make_input(5, 272, "u8", nonfinite=True)
    assert not (np.abs(x) == C.FLT_MAX).any(), "+-FLT_MAX only with scales <= 2^-8"
    cs = C.chan_scale(256)
    assert cs.min() >= 0.25 and cs.max() <= 4 and not ((cs.view(np.uint32) & 0x007FFFFF) == 0).any()


NO_TIES = {"vec-1000-f16-U16", "scalar-1x1", "scalar-3x5-rows"}     # a 16-bit grid under fp16 values; tensors too small to hold the pool


def _both_parities(t):
    return t.size >= 8 and {0, 1} <= set((np.floor(t).astype(np.int64) & 1).tolist())


def test_every_case_rounds_exact_ties_of_both_parities():
    """A kernel that rounded half away from zero (or up) instead of half to even has to show in EVERY case: the quotient the reference
    rounds -- behind the widening of fp16 and behind chan_scale -- is an exact half step at eight elements or more, with even and odd
    integer parts.  (The fp16 per-tensor fake-quant rounds its quotient to half first: a sixteenth of its quotients are ties.)"""
    for c in C.QUANTIZE_CASES:
        x, sc, of, qmin, qmax, cs = C.quantize_inputs(c)
        assert _both_parities(C.exact_ties(x, sc, cs)) or c.id in NO_TIES, c.id
    for c in C.TILED_CASES:
        for grid, _ in C.TILED_GRIDS:
            x, sc, of, qmin, qmax, cs = C.tiled_inputs(c, grid)
            assert _both_parities(C.exact_ties(x, sc, cs)), (c.id, grid)
    for c in C.FAKE_QUANT_CASES:
        x, sc, of, qmin, qmax = C.fake_quant_inputs(c)
        if c.dtype == "f16" and not c.per_row:
            with np.errstate(all="ignore"):
                t = (x.astype(F32) / sc[0]).astype(np.float16).astype(np.float64)
            t = t[np.isfinite(t)]
            assert _both_parities(t[t - np.floor(t) == 0.5]), c.id
        else:
            assert _both_parities(C.exact_ties(x, sc)), c.id


# ---- the case lists against the dispatch code -----------------------------------------------------------------------------------
def _reached(branches, **want):
    return any(all(b[k] == v for k, v in want.items()) for b in branches)


def test_quantize_cases_reach_every_branch():
    ids = [c.id for c in C.QUANTIZE_CASES]
    assert len(set(ids)) == len(ids) and 35 <= len(ids) <= 48
    B = [C.quantize_branch(c) for c in C.QUANTIZE_CASES]
    for c, b in zip(C.QUANTIZE_CASES, B):
        assert c.rows * c.cols <= 16400 * 256
        lo, hi = C.GRIDS[c.grid][2] - c.shift, C.GRIDS[c.grid][3] - c.shift
        info = np.iinfo(C.Q_NUMPY[c.q_dtype])
        assert info.min <= lo and hi <= info.max, c.id
        assert c.q_off % C.Q_BYTES[c.q_dtype] == 0, c.id                        # a store is never misaligned for its own type
        assert c.id.split("-")[0] in ("b16", "vec", "scalar", "cs", "nonfinite")
        if c.id.startswith(("b16", "vec", "scalar")):
            assert b["kernel"] == {"b16": "b16", "vec": "generic-vec", "scalar": "generic-scalar"}[c.id.split("-")[0]], c.id
    # b16: every 1-byte storage, per-tensor and per-row, with and without row_sum, the second sweep in both grid forms
    for q in ("i8", "u8"):
        for pr in (False, True):
            assert _reached(B, kernel="b16", q_dtype=q, per_row=pr), (q, pr)
    for pr in (False, True):
        assert _reached(B, kernel="b16", per_row=pr, row_sum=False) and _reached(B, kernel="b16", per_row=pr, row_sum=True)
        assert _reached(B, kernel="b16", per_row=pr, sweep2=True)
    assert _reached(B, kernel="b16", sweep2=True, row_sum=True) and _reached(B, kernel="b16", sweep2=True, row_sum=False)
    # generic kernel: every storage width in the vector form, fp32 (VN = 4) and fp16 (VN = 8); the scalar form by shape and by pointer
    for q in ("i8", "u8", "i16", "u16", "i32"):
        assert _reached(B, kernel="generic-vec", q_dtype=q), q
    for q in ("i8", "u8", "u16"):
        assert _reached(B, kernel="generic-scalar", q_dtype=q), q
    for dt in ("f32", "f16"):
        for k in ("generic-vec", "generic-scalar"):
            assert _reached(B, kernel=k, dtype=dt) and _reached(B, kernel=k, per_row=True) and _reached(B, kernel=k, per_row=False)
        assert _reached(B, kernel="generic-scalar", dtype=dt, forced_scalar=True)
    assert _reached(B, kernel="generic-scalar", forced_scalar=False)
    forced = [c for c, b in zip(C.QUANTIZE_CASES, B) if b["forced_scalar"]]
    assert any(c.x_off for c in forced) and any(c.q_off for c in forced)
    assert any(c.rows == 1 and c.cols == 1 for c in C.QUANTIZE_CASES) and {5, 255, 1027} <= {c.cols for c in C.QUANTIZE_CASES}
    assert any(c.rows == 1 and not b["per_row"] for c, b in zip(C.QUANTIZE_CASES, B))
    assert any(c.rows > 1 and b["per_row"] for c, b in zip(C.QUANTIZE_CASES, B))
    # chan_scale: the b16 form, the generic forms, and the pointer that is 4 but not 16 bytes aligned
    for k in ("b16-cs", "generic-cs-vec", "generic-cs-scalar"):
        assert _reached(B, kernel=k), k
    assert any(c.cs_off == 4 and c.cols % 16 == 0 and c.cols >= 256 and b["kernel"] == "generic-cs-vec" for c, b in zip(C.QUANTIZE_CASES, B))
    # non-finite inputs in both kernels
    assert _reached(B, kernel="b16", nonfinite=True) and any(b["nonfinite"] and b["kernel"].startswith("generic") for b in B)
    assert {c.grid for c in C.QUANTIZE_CASES} >= {"u8", "clamp", "coarse", "sym", "w4", "u16", "i16", "h8"}


def test_tiled_cases_reach_every_branch():
    ids = [c.id for c in C.TILED_CASES]
    assert len(set(ids)) == len(ids)
    B = [C.tiled_branch(c) for c in C.TILED_CASES]
    by_id = dict(zip(ids, B))
    for k in ("lane-generic", "lane-steps1", "lane-steps2", "lane-generic-f16", "lane-generic-cs",
              "staged-V1-rows4", "staged-V2-rows4", "staged-V3-rows8", "staged-V4-rows8", "staged-V2-rows8", "staged-V4-rows4"):
        assert _reached(B, kernel=k), k
    assert _reached(B, kernel="staged-V2-rows4", knob=4) and _reached(B, kernel="staged-V4-rows8", knob=8)
    assert _reached(B, kernel="lane-steps2", staged_off=True, rows_lt_64=False)
    for k in ("lane-generic", "lane-steps1", "lane-steps2"):
        assert _reached(B, kernel=k, rows_lt_64=True) and _reached(B, kernel=k, padding_workgroup=True), k
    assert _reached(B, kernel="lane-generic", idle_waves=True, padding_workgroup=True)          # (7, 128)
    assert by_id["lane-7x128"]["idle_waves"] and by_id["lane-7x128"]["padding_workgroup"]
    assert by_id["lane-33x1152"]["second_trip"] and by_id["lane-33x1152"]["unequal_waves"]      # nine pairs: wave 0 goes twice
    assert by_id["lane-40x5632"]["unequal_waves"] and by_id["lane-100x5120"]["second_trip"]
    assert _reached(B, kernel="lane-generic", nonfinite=True) and any(b["nonfinite"] and b["kernel"].startswith("staged") for b in B)
    assert all(c.rows * c.cols <= 2200000 for c in C.TILED_CASES)
    for g, shift in C.TILED_GRIDS:
        assert -128 <= C.GRIDS[g][2] - shift and C.GRIDS[g][3] - shift <= 127


def test_fake_quant_cases_reach_every_branch():
    B = [C.fake_quant_branch(c) for c in C.FAKE_QUANT_CASES]
    for dt in ("f32", "f16"):
        for g in ("tensor", "row"):
            for f in ("vec", "scalar"):
                assert _reached(B, kernel="%s-%s-%s" % (dt, g, f)), (dt, g, f)
    assert _reached(B, kernel="f32-tensor-scalar", misaligned=True) and _reached(B, kernel="f32-tensor-scalar", misaligned=False)
    assert _reached(B, kernel="f32-tensor-vec", second_trip=True) and _reached(B, kernel="f32-tensor-scalar", second_trip=True)
    assert _reached(B, alias=True)
    assert all(c.rows * c.cols <= 2200000 for c in C.FAKE_QUANT_CASES)
    for c in C.FAKE_QUANT_CASES:                       # half arithmetic holds the limits exactly only up to 8 bits (mq_fake_quant.hip)
        if c.dtype == "f16" and not c.per_row:
            assert C.GRIDS[c.grid][3] <= 255
        assert np.isnan(C.fake_quant_inputs(c)[0]).any()


def test_pack_and_epilogue_case_lists():
    assert C.EPILOGUE_N == [1, 255, 256, 257, 5632] and C.PACK_SHAPES == [(1, 64), (3, 128), (257, 192)]
    assert (257 * 192 // 2) % 256 != 0
    shifts = {(c["a_shift"], c["w_shift"]) for _, c in C.all_epilogue_cases()}
    assert {s for p in shifts for s in p} == {0, 128}
    for N, K in C.PACK_SHAPES:
        q = C.pack_input(N, K)
        assert np.array_equal(O.unpack_w4(O.pack_w4(q, 0), 0), q)
