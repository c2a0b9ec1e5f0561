"""CPU: the case lists of the training-pass pin (train_cases.py) reach the branches of csrc/mq_fake_quant.hip they exist for, planted values
are where they claim to be, the undecided cap and the sensitivity condition hold for every case (from the float64 reference alone), the
oracles (oracle.mq_oracle fake_quant_backward_terms, lwc_fused_*, train_attn_probs*) agree with an independent restatement -- the
reference's expression under torch-CPU autograd, fp32 for the bit-exact parts and float64 where the quotient is exact -- and four
deliberately broken oracles are seen to differ."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import train_cases as T  # noqa: E402
from oracle import mq_oracle as O  # noqa: E402

F32, F64 = np.float32, np.float64
FQB = {c.name: c for c in T.FQB_CASES}
ATTN = {c.name: c for c in T.ATTN_CASES}
SMALL_FQB = [c for c in T.FQB_CASES if c.rows * c.cols <= 70000]


def _same(a, b):
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    return bool(np.all((np.isnan(a) & np.isnan(b)) | (a == b)))


# ---- mq_fake_quant_backward -----------------------------------------------------------------------------------------------------------------
def test_fake_quant_backward_cases_reach_every_kernel_trip_and_unroll_slot():
    geo = {c.name: T.fqb_geom(c.rows, c.cols, c.n_scale, c.offs) for c in T.FQB_CASES}
    assert {g.kernel for g in geo.values()} == {"scalar", "vec", "row"}
    sizes = {c.rows * c.cols for c in T.FQB_CASES if geo[c.name].kernel == "scalar" and c.offs == (0, 0, 0)}
    assert sizes >= {1, 1023, 1152, 65535, 65538, 2 * 524288 + 259, 300}
    for w in ("x", "gy", "gx"):                               # a 4-byte offset of each pointer in turn sends 65536 elements to the scalar kernel
        c = FQB["scalar_65536_%s_off4" % w]
        assert geo[c.name].kernel == "scalar" and T.fqb_kernel(c.rows, c.cols, c.n_scale) == "vec" and sorted(c.offs) == [0, 0, 4]
    assert geo["scalar_65538"].kernel == "scalar" and 65538 % 4 and geo["scalar_65535"].kernel == "scalar"
    assert geo["scalar_1"].g == 1 and 1 < geo["scalar_65535"].g < 512
    big = geo["scalar_trips"]
    assert big.g == 512 and big.trips == 9 and (2 * 524288 + 259) % big.stride == 259, "eight full grid-stride trips and 259 elements of a ninth"
    v = geo["vec_65536"]
    assert v.kernel == "vec" and 65536 // 4 == 4 * v.stride and v.trips == 1, "every unroll slot exactly full"
    v, cl = geo["vec_65540"], T.fqb_classes(1, 65540, 1)
    assert v.kernel == "vec" and v.trips == 1 and 0 < np.count_nonzero(cl["u"] == 3) < 4 * v.stride, "slot u = 3 partly filled"
    assert set(cl["u"].tolist()) == {0, 1, 2, 3}
    assert geo["vec_262148"].kernel == "vec" and 1 < geo["vec_262148"].g < 2048
    v, cl = geo["vec_capped"], T.fqb_classes(1, 8388608 + 4 * 524365, 1)
    assert v.g == 2048 and v.trips == 2 and set(cl["sweep"][-8:].tolist()) == {1} and set(cl["u"][cl["sweep"] == 1].tolist()) == {0, 1}
    assert {(c.rows, c.cols) for c in T.FQB_CASES if geo[c.name].kernel == "row"} >= {(2, 1), (3, 96), (5, 255), (5, 256), (5, 257), (7, 1000), (4099, 8)}
    c = FQB["row_1x300_is_per_tensor"]
    assert c.rows == c.n_scale == 1 and geo[c.name].kernel == "scalar"
    for k in ("scalar", "vec", "row"):
        grids = {(c.grid.bits, c.grid.sym) for c in T.FQB_CASES if geo[c.name].kernel == k}
        assert grids == {(b, s) for b in (4, 8, 16) for s in (False, True)}, (k, grids)
        assert any(c.grid.offset < 0 for c in T.FQB_CASES if geo[c.name].kernel == k), "a negative offset"
        assert any(c.nonfinite for c in T.FQB_CASES if geo[c.name].kernel == k), "a NaN and an infinity in x"
    for c in T.FQB_CASES:                                     # the add counts: per thread, 6 + 2, the atomics
        g = geo[c.name]
        per_thread = {"scalar": g.trips, "row": g.trips, "vec": 16 * g.trips}[g.kernel]
        assert g.n == per_thread + 8 + (1 if g.kernel == "row" else g.g)


@pytest.mark.parametrize("case", SMALL_FQB, ids=lambda c: c.name)
def test_fake_quant_backward_plants_sit_on_and_around_both_clamp_edges(case):
    d = T.fqb_inputs(case)
    t, r, inside, qc, _ = O.fq_point(d["x"], d["s2d"], d["o2d"], d["qmin"], d["qmax"])
    q = r + d["o2d"]
    want = {"qmax": (d["qmax"], True), "qmin": (d["qmin"], True), "above": (d["qmax"] + 1, False), "below": (d["qmin"] - 1, False)}
    pow2 = np.log2(case.grid.scale) % 1 == 0 and T.fqb_kernel(case.rows, case.cols, case.n_scale, case.offs) != "row"
    for kind, pos in d["plants"].items():
        for (rr, cc) in pos:
            if (rr * case.cols + cc) in [p for p, _ in d["nonfinite"]]:
                continue
            if kind in want:
                assert q[rr, cc] == want[kind][0] and bool(inside[rr, cc]) == want[kind][1], (kind, rr, cc, q[rr, cc])
            elif pow2:
                assert (2 * t[rr, cc]) % 2 == 1, "an exact tie under a power-of-two scale"
    if case.rows * case.cols >= 8:
        assert all(len(d["plants"][k]) for k in ("qmax", "qmin", "above", "below"))
    assert (~inside).any() or case.rows * case.cols < 8
    e = T.fqb_expect(case)
    if case.nonfinite:
        flat = d["x"].reshape(-1)
        assert np.isnan(flat[d["nonfinite"][0][0]]) and np.isposinf(flat[d["nonfinite"][1][0]])
        assert np.isnan(e["sum_ts"]).any() and np.all(np.isfinite(e["sum_to"])), "a non-finite x makes grad_scale NaN and leaves grad_offset finite"
        assert all(e["gx"].reshape(-1)[p] == 0 for p, _ in d["nonfinite"])


@pytest.mark.parametrize("case", T.FQB_CASES, ids=lambda c: c.name)
def test_fake_quant_backward_losing_any_trip_slot_or_wave_moves_a_sum_by_eight_bars(case):
    d, e = T.fqb_inputs(case), T.fqb_expect(case)
    cl = T.fqb_classes(case.rows, case.cols, case.n_scale, case.offs)
    for name in ("ts", "to"):
        t = np.nan_to_num(e[name].astype(F64), nan=0.0)
        r, where = T.sensitivity(t, e["bar_" + name], d["group"], cl)
        assert r >= T.SENS, (name, r, where)


def _torch_fq(x, s, o, qmin, qmax):
    t = x / s
    return ((((t.round() - t).detach() + t) + o).clamp(qmin, qmax) - o) * s


@pytest.mark.parametrize("case", [c for c in SMALL_FQB if not c.nonfinite], ids=lambda c: c.name)
def test_fake_quant_backward_oracle_is_torch_autograd_of_the_reference_expression(case):
    """fp32 autograd: grad_x bit for bit on every grid.  float64 autograd on the power-of-two scales, where the quotient is exact in both
    precisions: the two sums to u sum|term| (the oracle's terms are fp32 products, rounded once each)."""
    d, e = T.fqb_inputs(case), T.fqb_expect(case)
    per_row = d["n_group"] > 1
    for dt in (torch.float32, torch.float64):
        x = torch.from_numpy(d["x"]).to(dt).requires_grad_(True)
        s = torch.from_numpy(d["s2d"] if per_row else d["s2d"].reshape(())).to(dt).requires_grad_(True)
        o = torch.from_numpy(d["o2d"] if per_row else d["o2d"].reshape(())).to(dt).requires_grad_(True)
        (_torch_fq(x, s, o, d["qmin"], d["qmax"]) * torch.from_numpy(d["g"]).to(dt)).sum().backward()
        if dt == torch.float32:
            assert _same(x.grad.numpy(), e["gx"])
        elif np.log2(case.grid.scale) % 1 == 0 and not per_row:
            for got, name in ((s.grad, "ts"), (o.grad, "to")):
                tol = O.U32 * np.abs(e[name].astype(F64)).sum() + 1e-300
                assert abs(float(got) - float(e["sum_" + name][0])) <= tol, (name, float(got), e["sum_" + name])


# ---- mq_lwc_fake_quant(_backward) -----------------------------------------------------------------------------------------------------------
def test_lwc_widths_sit_on_both_sides_of_every_vpt_boundary_and_extremes_reach_every_class():
    assert {T.lwc_vpt(c) for c in T.LWC_COLS} == {2, 4, 6, 8, 16}
    for edge in (2048, 4096, 6144, 8192):
        assert edge in T.LWC_COLS and edge + 4 in T.LWC_COLS and T.lwc_vpt(edge) != T.lwc_vpt(edge + 4)
    assert {4, 64, 1020, 1024, 16384} <= set(T.LWC_COLS) and set(T.LWC_ROWS) == {1, 5, 33}
    assert set(T.LWC_GRIDS) == {(b, s) for b in (2, 4, 8, 16) for s in (False, True)}
    assert set(T.LWC_KINDS[33]) == {"plant", "tie2", "tie3", "const", "zero", "negzero_min", "nan", "pinf"}
    for cols in T.LWC_COLS:
        pos = T.lwc_positions(cols)
        nvec = cols // 4
        assert all(0 <= c < cols for c in pos)
        assert {v for v in pos.values() if v.startswith("wave")} == {"wave%d_k%d" % ((j % 256) // 64, j // 256) for j in range(nvec)}
        for k in range(1, T.cdiv(cols, 1024) + 1):
            assert {c for c, v in pos.items() if v == "slice%d_last" % k} | {c for c, v in pos.items() if v.startswith("wave")} >= set(
                range(1024 * k - 4, min(1024 * k, cols)))
        assert set(range(cols - 4, cols)) <= set(pos)
        seen_mx, seen_mn = set(), set()
        for bits, sym in T.LWC_GRIDS:
            for rows in T.LWC_ROWS:
                for r, kind in enumerate(T.LWC_KINDS[rows]):
                    if kind == "plant":
                        a, b = T.lwc_plants(cols, bits, sym, rows, r)
                        assert a != b
                        seen_mx.add(a)
                        seen_mn.add(b)
        assert seen_mx == set(pos) == seen_mn, (cols, set(pos) - seen_mx, set(pos) - seen_mn)


@pytest.mark.parametrize("cols", T.LWC_COLS)
def test_lwc_rows_are_what_their_kind_says_and_a_lost_slice_or_wave_shows(cols):
    for bits, sym in T.LWC_GRIDS:
        for rows in T.LWC_ROWS:
            d = T.lwc_inputs(cols, bits, sym, rows)
            w, f = d["w"], d["fwd"]
            b = O.lwc_fused_backward(w, d["g"], d["sig_lo"], d["sig_hi"], f["row_min"], f["row_max"], bits, sym)
            for r, kind in enumerate(d["kinds"]):
                if kind in ("plant", "tie2", "tie3"):
                    mxc, mnc = d["ext"][r]
                    assert tuple(np.flatnonzero(w[r] == w[r].max())) == tuple(sorted(mxc)) and tuple(np.flatnonzero(w[r] == w[r].min())) == tuple(sorted(mnc))
                    assert len(mxc) == (2 if kind == "tie2" else 1) and len(set(mnc)) == (min(3, len(set(mnc))) if kind == "tie3" else 1)
                elif kind == "const":
                    assert b["extreme"][r].all()
                elif kind == "zero":
                    assert not b["passes"][r] and f["scale"][r] == O.CLIPMIN and b["grad_sig_lo"][r] == 0 and b["grad_sig_hi"][r] == 0
                    assert _same(b["grad_w"][r], b["gx"][r]), "the CLIPMIN clamp blocks the range gradient"
                elif kind == "negzero_min":
                    assert f["row_min"][r] == 0 and np.signbit(w[r]).any() and np.count_nonzero(w[r] == 0) >= 3
                elif kind == "nan":
                    assert np.isnan(f["row_min"][r]) and np.isnan(f["y"][r]).all() and np.isnan(b["grad_sig_lo"][r]) and np.all(b["grad_w"][r] == 0)
                elif kind == "pinf":
                    assert np.isposinf(f["row_max"][r]) and np.isnan(f["y"][r]).sum() == 1 and f["scale"][r] == O.CLIPMAX
            bars = np.where(b["passes"], T.gamma(T.lwc_n(cols)) * np.nan_to_num(b["sumabs"]), 0.0)
            r, where = T.sensitivity(np.nan_to_num(b["ts"].astype(F64)), bars, d["group"], T.lwc_classes(rows, cols))
            assert r >= T.SENS, (cols, bits, sym, rows, r, where)


@pytest.mark.parametrize("cols,bits,sym", [(64, 4, False), (1020, 8, True), (2052, 2, False), (6148, 16, False), (64, 16, True)])
def test_lwc_oracle_is_torch_fp32_autograd_of_the_reference_expression(cols, bits, sym):
    """The reference's expression in fp32 under autograd, as test_gpu_round4.py writes it: forward and grid bit for bit, grad_w bit for bit
    off the extremes; the row sums within torch's own summation error, gamma_cols |c| sum|term| (sequential at worst)."""
    rows = 33
    d = T.lwc_inputs(cols, bits, sym, rows)
    f = d["fwd"]
    qmin, qmax = O.qrange(bits, sym)
    keep = np.array([k not in ("nan", "pinf") for k in d["kinds"]])
    w = torch.from_numpy(d["w"][keep]).requires_grad_(True)
    slo = torch.from_numpy(d["sig_lo"][keep]).view(-1, 1).requires_grad_(True)
    shi = torch.from_numpy(d["sig_hi"][keep]).view(-1, 1).requires_grad_(True)
    lo, hi = slo * w.amin(-1, keepdim=True), shi * w.amax(-1, keepdim=True)
    alpha, beta = (torch.maximum(lo.abs(), hi.abs()), 0 * lo) if sym else (hi - lo, lo)
    scale = (alpha / qmax).clamp(min=1e-5, max=1e6)
    offset = -(beta / scale).round()
    y = _torch_fq(w, scale, offset, qmin, qmax)
    (y * torch.from_numpy(d["g"][keep])).sum().backward()
    assert _same(y.detach().numpy(), f["y"][keep]) and _same(scale.detach().view(-1).numpy(), f["scale"][keep])
    assert _same(offset.detach().view(-1).numpy(), f["offset"][keep])
    b = O.lwc_fused_backward(d["w"], d["g"], d["sig_lo"], d["sig_hi"], f["row_min"], f["row_max"], bits, sym)
    off = ~b["extreme"][keep]
    assert _same(w.grad.numpy()[off], b["gx"][keep][off])
    gm = T.gamma(cols + 16)
    for got, name, c in ((slo.grad, "grad_sig_lo", "c_sig_lo"), (shi.grad, "grad_sig_hi", "c_sig_hi")):
        err = np.abs(got.view(-1).numpy().astype(F64) - b[name][keep])
        assert np.all(err <= gm * b[c][keep] * b["sumabs"][keep] + 1e-300), (name, err.max())
    err = np.abs(w.grad.numpy().astype(F64) - b["grad_w"][keep])
    assert np.all(err <= gm * (np.abs(b["gx"][keep]) + b["c_scat"][keep] * b["sumabs"][keep][:, None]) + 1e-300)


# ---- mq_attention_probs_train(_backward) ----------------------------------------------------------------------------------------------------
def test_attention_cases_reach_every_vpt_both_row_layouts_every_trip_mask_and_body():
    edge = [c for c in T.ATTN_CASES if c.name.startswith("keys")]
    assert {c.cols for c in edge} == {4, 252, 256, 260, 512, 516, 1024, 1028, 2048, 2052, 4096}
    assert {T.attn_fwd_geom(c.rows, c.cols).vpt for c in edge} == {1, 2, 4, 8, 16}
    assert {(g.vpt, g.tpr) for g in (T.attn_bwd_geom(c.rows, c.cols) for c in edge)} == {(1, 64), (2, 64), (1, 256), (2, 256), (4, 256)}
    assert all(c.rows >= 9 and c.rows % 4 for c in edge), "a partial last group of four rows"
    for keys in {c.cols for c in edge}:
        cs = [c for c in edge if c.cols == keys]
        assert {float(c.sqrt_d) for c in cs} == set(T.SQRT_D)
        assert {T.attn_fast(*[T.attn_grids(c)[i][0] for i in (0, 1)], c.sqrt_d) for c in cs} == {True, False}
    assert {c.mask for c in edge} == set(T.ATTN_MASKS)
    assert all(c.rows % c.mask_rows == 0 for c in T.ATTN_CASES if c.mask != "none")
    assert any(c.mask == "wrap" and 1 < c.mask_rows < c.rows for c in edge) and any(c.mask == "full" and c.mask_rows == c.rows for c in edge)
    assert T.attn_fast(1.0, 1.0, 8.0) and not T.attn_fast(1.0, 1.0, T.SQRT_D[1]) and not T.attn_fast(2.0 ** 61, 1.0, 8.0) and not T.attn_fast(1.0, 2.0 ** -61, 8.0)
    c = ATTN["s1_2p61"]
    assert not T.attn_fast(T.attn_grids(c)[0][0], T.attn_grids(c)[1][0], c.sqrt_d) and T.attn_fast(1.0, 1.0, c.sqrt_d), "!FAST by the scale alone"
    c = ATTN["fwd_trips"]
    assert (c.rows, c.cols) == (32768 + 6, 4) and T.attn_fwd_geom(c.rows, c.cols) == T.AttnFwdGeom(1, 8192, 2, 10)
    c = ATTN["bwd_wave_trips"]
    g = T.attn_bwd_geom(c.rows, c.cols)
    assert (c.rows, c.cols) == (2 * 8192 + 5, 8) and (g.tpr, g.grid, g.iters) == (64, 2048, 3) and g.dead > 0
    c = ATTN["bwd_wg_trips"]
    g = T.attn_bwd_geom(c.rows, c.cols)
    assert (c.rows, c.cols) == (2 * 2048 + 3, 516) and (g.vpt, g.tpr, g.grid, g.iters, g.dead) == (1, 256, 2048, 3, 2045), "trip 2 reuses trip 0's LDS slots"
    assert g.n_grid == 3 * 4 + 8 + 2048 and g.n_l == 4 + 6 + 2


@pytest.mark.parametrize("case", T.ATTN_CASES, ids=lambda c: c.name)
def test_attention_case_clamps_caps_and_sensitivity(case):
    d = T.attn_inputs(case)
    f, b = d["fwd"], d["bwd"]
    live = ~f["nan_row"]
    if case.s1 is None:
        t1 = f["t1"]
        assert (~f["in1"] & (t1 > 0)).any() and (~f["in1"] & (t1 < 0)).any(), "Q1 clamps on both sides"
        assert (~f["in2"][live]).any(), "some row is peaked enough that Q2 clamps"
    else:
        assert np.all(f["x"] == 0) and _same(f["p"], np.full(f["p"].shape, 1.0 / case.cols)), "every score quantizes to 0"
        assert len(np.unique(f["out"])) == 1 and not f["undecided"].any()
    assert f["nan_row"].sum() == (1 if case.mask == "nanrow" else 0)
    if case.mask == "causal" or (case.mask in ("full", "wrap") and case.cols > 4):    # the one vector of a 4-key row holds the peak: nothing is hidden
        assert f["masked"][live].any() and np.all(f["out"][f["masked"] & live[:, None]] == 0)
    for r in (f, b["fwd"]):                                   # forward and backward envelopes differ by the summation length
        assert r["undecided"][live].mean() <= 0.01, r["undecided"][live].mean()
        assert not r["edge"].any()
    vals, bars = T.attn_bwd_sums(case, d)
    cl = T.attn_bwd_classes(case.rows, case.cols)
    ge = T.attn_bwd_geom(case.rows, case.cols)
    assert set(cl["trip"].tolist()) == set(range(ge.iters))
    grp = np.zeros(case.rows * case.cols, np.int64)
    for name, t, v, bar in zip(("d s1", "d o1", "d s2", "d o2"), b["terms"], vals, bars):
        if np.isfinite(v):                                    # a NaN row makes the sum NaN: there the check is that it is NaN
            r, where = T.sensitivity(np.nan_to_num(t), [bar], grp, cl)
            assert r >= T.SENS, (name, r, where)
        else:
            assert case.mask == "nanrow"
    # the row sum dot = sum(gp p): in every slice and wave of the row layout some row moves a grad_raw element by eight of its bars
    with np.errstate(all="ignore"):
        per_el = np.where(f["in1"] & (b["p"] > 0), b["e_raw"] * float(F32(case.sqrt_d)) / b["p"], np.inf)
    row_bar = np.nan_to_num(per_el, nan=np.inf).min(axis=1)
    rows_i = np.repeat(np.arange(case.rows), case.cols)
    within = {k: v for k, v in cl.items() if k == "k" or (k == "wave" and ge.tpr == 256)}
    for name, ids in within.items():
        key = T.class_keys(rows_i, ids, case.rows)
        cs = np.abs(np.bincount(key, weights=np.nan_to_num(b["prod"]).reshape(-1), minlength=(int(ids.max()) + 1) * case.rows)).reshape(-1, case.rows)
        ratio = np.where(np.isfinite(row_bar) & live, cs / np.where(np.isfinite(row_bar), row_bar, 1.0), 0.0).max(axis=1)
        assert np.all(ratio >= T.SENS), (name, ratio)


@pytest.mark.parametrize("name", ["keys4_sd0_none", "keys260_sd1_none", "keys516_sd1_wrap", "keys1028_sd2_full", "keys252_sd1_causal", "s1_2p61"])
def test_attention_oracles_are_torch_autograd_of_the_reference_expression(name):
    """Forward, fp32 torch as test_gpu_round4.py writes it: x bit for bit; the probabilities equal the oracle's grid value wherever decided
    under torch's own summation length (cols) and are one of the two neighbours elsewhere.  Backward: the softmax / Q2 stage in float64
    autograd from the oracle's x (to 1e-11), the Q1 stage in fp32 autograd (grad_raw to 4 u, its two sums within torch's summation error)."""
    case = ATTN[name]
    d = T.attn_inputs(case)
    g1, g2 = d["grid1"], d["grid2"]
    raw, gy, mask = d["raw"], d["gy"], d["mask"]
    mrow = None if mask is None else torch.from_numpy(mask[np.arange(case.rows) % mask.shape[0]])
    f = O.train_attn_probs(raw, mask, g1, g2, case.sqrt_d, case.cols + 8)
    t_raw = torch.from_numpy(raw)
    a = _torch_fq(t_raw, torch.tensor(g1[0]), torch.tensor(g1[1]), g1[2], g1[3]) / float(F32(case.sqrt_d))
    x = a if mrow is None else a + mrow
    assert _same(x.numpy(), f["x"])
    p = _torch_fq(torch.softmax(x, dim=-1, dtype=torch.float32), torch.tensor(g2[0]), torch.tensor(g2[1]), g2[2], g2[3]).numpy()
    und = f["undecided"]
    assert _same(p[~und], f["out"][~und]) and np.all((p[und] == f["out"][und]) | (p[und] == f["out_alt"][und]))
    # softmax and Q2 backward, float64 from the oracle's own x
    b = d["bwd"]
    x64 = torch.from_numpy(b["fwd"]["x"].astype(F64)).requires_grad_(True)
    s2 = torch.tensor(float(F32(g2[0])), dtype=torch.float64, requires_grad=True)
    o2 = torch.tensor(float(F32(g2[1])), dtype=torch.float64, requires_grad=True)
    (_torch_fq(torch.softmax(x64, dim=-1), s2, o2, g2[2], g2[3]) * torch.from_numpy(gy.astype(F64))).sum().backward()
    sd = float(F32(case.sqrt_d))
    in1 = b["fwd"]["in1"]
    scale = max(1.0, float(np.abs(gy).max()))
    assert np.abs(x64.grad.numpy()[in1] / sd - b["grad_raw"][in1]).max() <= 1e-11 * scale
    assert abs(float(s2.grad) - b["terms"][2].sum()) <= 1e-11 * np.abs(b["terms"][2]).sum() + 1e-300
    assert abs(float(o2.grad) - b["terms"][3].sum()) <= 1e-11 * np.abs(b["terms"][3]).sum() + 1e-300
    # Q1 backward, fp32 autograd with the gradient that reaches it
    up = (x64.grad.numpy() / sd).astype(F32)
    r1 = t_raw.clone().requires_grad_(True)
    s1, o1 = torch.tensor(g1[0], requires_grad=True), torch.tensor(g1[1], requires_grad=True)
    (_torch_fq(r1, s1, o1, g1[2], g1[3]) * torch.from_numpy(up)).sum().backward()
    assert np.all(r1.grad.numpy()[~in1] == 0)
    assert np.all(np.abs(r1.grad.numpy().astype(F64) - b["grad_raw"]) <= 4 * O.U32 * np.abs(b["grad_raw"]) + 1e-11 * scale)
    gm = T.gamma(raw.size + 16)
    for got, i in ((s1.grad, 0), (o1.grad, 1)):
        assert abs(float(got) - b["terms"][i].sum()) <= gm * np.abs(b["terms"][i]).sum() + 1e-300, (i, float(got), b["terms"][i].sum())


# ---- deliberately broken oracles -------------------------------------------------------------------------------------------------------------
def test_broken_oracles_are_seen_to_differ():
    """Round half away, an exclusive clamp mask, a tie given to one extreme only, the mask row taken without the modulo: each changes what
    the GPU file would expect of at least one case, by more than the bar where the quantity is bounded."""
    case = FQB["scalar_1152_grid3"]                            # 8-bit symmetric, scale 2^-5: planted ties are exact
    good = T.fqb_expect(case)
    for m in ("half_away", "exclusive_mask"):
        bad = T.fqb_expect(case, mutation=m)
        assert not _same(bad["gx"], good["gx"]), m
        assert abs(bad["sum_ts"][0] - good["sum_ts"][0]) > good["bar_ts"][0], m
    d = T.lwc_inputs(64, 4, False, 33)
    f = d["fwd"]
    args = (d["w"], d["g"], d["sig_lo"], d["sig_hi"], f["row_min"], f["row_max"], 4, False)
    good, bad = O.lwc_fused_backward(*args), O.lwc_fused_backward(*args, mutation="tie_one")
    r = d["kinds"].index("tie2")
    bar = T.gamma(T.lwc_n(64) + 8) * (np.abs(good["gx"][r]) + good["c_scat"][r] * good["sumabs"][r])
    assert (np.abs(bad["grad_w"][r] - good["grad_w"][r]) > bar).sum() == 2, "both tied maxima move: one takes all, one nothing"
    assert _same(bad["grad_w"][d["kinds"].index("plant")], good["grad_w"][d["kinds"].index("plant")])
    case = ATTN["keys516_sd1_wrap"]
    d = T.attn_inputs(case)
    bad = O.train_attn_probs(d["raw"], d["mask"], d["grid1"], d["grid2"], case.sqrt_d, 14, mutation="mask_no_mod")
    rows_bad = np.flatnonzero([not _same(bad["out"][r], d["fwd"]["out"][r]) for r in range(case.rows)])
    assert len(rows_bad) and rows_bad.min() >= case.mask_rows, "only the rows past the first wrap differ"
    for m in ("half_away", "exclusive_mask"):
        b2 = O.train_attn_probs_backward(d["raw"], d["gy"], d["mask"], d["grid1"], d["grid2"], case.sqrt_d, 14, mutation=m)
        vals, bars = T.attn_bwd_sums(case, d)
        assert any(abs(t.sum() - v) > bar for t, v, bar in zip(b2["terms"], vals, bars)) or m == "half_away"
