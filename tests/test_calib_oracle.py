"""CPU: the case lists of the calibration / min-max pin (calib_cases.py) reach the branches of csrc/mq_reduce.hip they exist for, the
planted extremes cover what they claim, and the oracles (oracle.mq_oracle calib_*) agree with independent restatements -- torch-CPU
softmax / layer_norm / silu / gelu at float64, llama.apply_rope bit for bit.  The replay search of the norm admits the true fp32 statistic
and rejects a row moved by one ulp, with a candidate count capped from gamma_n."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import calib_cases as C  # noqa: E402
from oracle import mq_oracle as O  # noqa: E402

F32, F16 = np.float32, np.float16


# ---- geometry: every list reaches its branches ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_tensor_sizes_reach_every_branch_of_launch_tensor(dtype):
    n = C.VEC[dtype]
    offs = C.tensor_offsets(dtype)
    assert offs == tuple(range(16 // C.SIZE[dtype]))
    geoms = {(s, o): C.tensor_geom(s, o, dtype) for s in C.tensor_sizes(dtype) for o in offs}
    gs = {g.g for g in geoms.values()}
    assert 1 in gs and 512 in gs and any(1 < g < 512 for g in gs)
    assert {g.head for g in geoms.values()} >= set(range(n)), "every head length 0 .. N - 1"
    assert {g.tail for g in geoms.values()} >= set(range(n)), "every tail length 0 .. N - 1"
    assert any(g.nvec == 0 for g in geoms.values()) and any(g.head == s for (s, o), g in geoms.items()), "all-scalar tensors"
    big = C.tensor_geom(C.tensor_sizes(dtype)[-1], 0, dtype)
    four, one = C.tensor_trips(big)
    assert big.g == 512 and four >= 2 and 1 <= one <= 3, (big, four, one)
    assert big.nvec % big.stride not in (0,) and big.tail > 0            # the last single trip is partial: some lanes idle
    classes = set()
    for (s, o), g in geoms.items():
        pos = C.tensor_positions(s, o, dtype)
        assert all(0 <= p < s for p in pos)
        assert sum(1 for c in pos.values() if c == "head") == g.head and sum(1 for c in pos.values() if c == "tail") == g.tail
        classes |= set(pos.values())
        plants = C.tensor_plants(s, o, dtype)
        assert {p[0] for p in plants} == set(pos) == {p[1] for p in plants}, "every position holds the maximum once and the minimum once"
    want = {"head", "tail", "vec0_first", "vec0_last", "vecN_first", "vecN_last"} | {"stride%d_%s" % (k, w) for k in (1, 2, 3) for w in ("before", "at")}
    assert classes == want, classes ^ want


def test_rows_cases_cover_both_paths_every_lane_and_the_tail():
    for dt in ("f32", "f16"):
        cs = [c for c in C.ROWS_CASES if c.dtype == dt]
        assert {C.rows_vec_ok(c.cols, c.off, dt) for c in cs} == {True, False}
        assert any(c.off and c.cols % C.VEC[dt] == 0 for c in cs), "a pointer offset that defeats vec_ok"
        assert any(C.rows_vec_ok(c.cols, c.off, dt) and c.cols // C.VEC[dt] > 64 for c in cs), "a second sweep of the wave"
        assert any(c.rows % 4 for c in cs) and any(c.rows > 4 for c in cs), "a partial workgroup and more than one"
    for c in C.ROWS_CASES:
        vec = C.rows_vec_ok(c.cols, c.off, c.dtype)
        units = c.cols // C.VEC[c.dtype] if vec else c.cols
        lanes = set(range(min(64, units)))
        ls = C.rows_launches(c)
        for kind in (0, 1):
            got = {C.rows_lane(p[kind], c) for row in ls for p in row}
            assert got >= lanes, (c.id, kind, sorted(lanes - got))
        assert any(p[0] == c.cols - 1 for row in ls for p in row), "the last scalar"
        if vec:
            assert any(p[1] // C.VEC[c.dtype] == units - 1 for row in ls for p in row), "the last vector"
        for j in range(len(ls)):
            x = C.rows_input(c, j)
            for r, (mx, mn) in enumerate(ls[j]):
                assert x[r].argmax() == mx and (x[r] == x[r, mx]).sum() == 1
                assert c.cols == 1 or (x[r].argmin() == mn and (x[r] == x[r, mn]).sum() == 1)
            assert x.dtype == C.NP[c.dtype] and np.array_equal(x.astype(np.float64).astype(x.dtype), x)


def test_cols_cases_cover_both_kernels_every_row_and_ragged_chunks():
    for dt in ("f32", "f16"):
        cs = [c for c in C.COLS_CASES if c.dtype == dt]
        ge = {c: C.cols_geom(c.rows, c.cols, c.off, dt) for c in cs}
        n = C.VEC[dt]
        assert {c.cols for c in cs if ge[c].vec} == {n, 64 * n, 64 * n + n, 5 * 64 * n}
        assert {c.cols for c in cs if not ge[c].vec and not c.off} == {1, 7, 255, 257, 1001}
        assert any(c.off and c.cols % n == 0 and not ge[c].vec for c in cs), "an unaligned pointer with vector-friendly cols"
        assert any(ge[c].vec and ge[c].ctiles > 1 for c in cs) and any(not ge[c].vec and ge[c].ctiles > 1 for c in cs)
        assert any(ge[c].chunks >= 3 and c.rows % ge[c].rpb for c in cs if ge[c].vec), "three row chunks, the last ragged (vector)"
        assert any(ge[c].chunks >= 3 and c.rows % ge[c].rpb for c in cs if not ge[c].vec), "three row chunks, the last ragged (scalar)"
        assert {c.rows for c in cs} == {1, 3, 63, 64, 65, 257}
    for c in C.COLS_CASES:
        hit = set()
        for j in (0, 1):
            mx, mn = C.cols_plants(c, j)
            hit |= set(mx.tolist()) | (set(mn.tolist()) if c.rows > 1 else set())
            x = C.cols_input(c, j)
            assert np.array_equal(x.argmax(axis=0), mx) and np.array_equal((x == x.max(axis=0)).sum(axis=0), np.ones(c.cols))
            if c.rows > 1:
                assert np.array_equal(x.argmin(axis=0), mn) and np.array_equal((x == x.min(axis=0)).sum(axis=0), np.ones(c.cols))
        if 4 * c.cols >= c.rows:
            assert hit == set(range(c.rows)), (c.id, sorted(set(range(c.rows)) - hit))
        else:
            assert {0, min(4 * c.cols, c.rows) - 1} <= hit


def test_planted_values_survive_fp16():
    for v in [2 + r / 8 for r in range(16)] + [k / 1024 for k in (-1000, -1, 1, 999, 1000)]:
        assert float(F16(v)) == v and float(F16(-v)) == -v
    for dt in ("f16", "f32"):
        k = C.base_values(4096, dt).astype(np.float64) * 1024
        assert np.array_equal(k, np.rint(k)) and np.abs(k).max() <= 1000


def test_score_chain_lists_reach_every_vpt_and_the_grid_stride_trips():
    vp = {}
    for c in C.PROBS_CASES:
        vp.setdefault(C.probs_geom(c.rows, c.cols)[0], set()).add(c.cols)
    assert vp == {1: {4, 256}, 2: {260, 512}, 4: {516, 1024}, 8: {1028, 2048}, 16: {2052, 4096}}, vp
    multi = [c for c in C.PROBS_CASES if C.probs_geom(c.rows, c.cols)[3] > 1]
    assert multi and all(c.rows > 8192 and c.rows % 8192 and c.mask_rows and c.rows % c.mask_rows == 0 and 8192 % c.mask_rows for c in multi)
    cv = {}
    for c in C.CAUSAL_CASES:
        v, grid, per_trip, trips = C.causal_geom(c.seq * c.blocks, c.seq)
        cv.setdefault(v, []).append(trips)
        assert grid * 4 == per_trip * c.seq and grid * 4 <= max(8192, c.seq)
    for v in (1, 2, 8, 16):
        assert any(len(t) >= 3 and t[-1] < t[0] for t in cv[v]), "VPT %d: an odd trip and a partial last trip" % v
    assert any(len(t) == 1 for t in cv[1]) and any(len(t) == 1 for t in cv[2])
    assert {c.seq for c in C.CAUSAL_CASES if len(C.causal_geom(c.seq * c.blocks, c.seq)[3]) == 1} == {4, 64, 100, 256, 260}
    want = {64: [128, 128, 4], 100: [81, 81, 38], 260: [31, 31, 8], 1028: [7, 7, 2], 2052: [3, 3, 1]}
    for c in C.CAUSAL_CASES:
        trips = C.causal_geom(c.seq * c.blocks, c.seq)[3]
        if len(trips) > 1:
            assert trips == want[c.seq], (c.id, trips)
            rows = c.seq * c.blocks
            first, odd, last = [p[0] for p in C.causal_plants(c)]
            nw = trips[0] * c.seq
            assert first < nw <= odd < 2 * nw <= last < rows
            assert odd % c.seq == c.seq - 1 and odd - (c.seq - 1) == nw, "the row the first wave of the odd trip visits first"
            assert all(r % c.seq >= 2 for r in (first, odd, last)), "columns 0 and 1 are live"
    assert max(c.seq * c.seq * c.blocks * 4 for c in C.CAUSAL_CASES) < 120e6


def test_odd_rows_and_the_all_ones_rows():
    for seq in C.ODD_SEQ:
        raw, marks = C.odd_input(seq)
        o = O.calib_probs(raw, C.INV_SQRT_D, causal=True)
        o2 = O.calib_probs(raw, C.INV_SQRT_D, mask=C.odd_mask(seq))
        assert np.array_equal(o["nan_row"], o2["nan_row"]) and np.array_equal(o["p"], o2["p"], equal_nan=True)
        names = {m[1] for m in marks}
        assert names == {r[0] for r in C.ODD_ROWS}
        marked = {m[0]: m[2] for m in marks}
        for r in range(raw.shape[0]):
            assert bool(o["nan_row"][r]) == marked.get(r, False), (seq, r, marked.get(r))
        diag_blocks = {(m[0] % seq) >> 8 for m in marks}
        assert len(diag_blocks) >= 2, "odd rows whose diagonal lies in different 256-column blocks"
    raw, mask, info = C.allones_input()
    o = O.calib_probs(raw, C.INV_SQRT_D, mask=mask)
    assert not o["nan_row"].any() and all((~o["masked"][r]).sum() == 2 for r, *_ in info)
    for r, k, c0, c1 in info:
        assert o["x"][r, c0] == 0 and o["x"][r, c1] == F32(-k * 2.0 ** -23)
    ex = np.exp(np.float64(-2.0 ** -23)).astype(F32)                  # correctly rounded: 1 - 2^-23
    assert (F32(1) + ex).view(np.uint32) == 0x3fffffff
    tab = C.allones_table()
    # RN(1 / l) alone does not name l (0x3fffffff and 0x3ffffffe share 0x3f000001), and the pair leaves one ambiguity per all-ones l: an
    # expf one ulp low (odd j) ties 1 + ex down to the even neighbour and yields the same two quotients.  A correctly rounded expf is j = 2 k.
    ones = [k for k, v in tab.items() if any(l & 0x7fffff == 0x7fffff for _, l in v)]
    assert ones and all(len(tab[k]) == 2 and tab[k][0][0] % 2 == 0 and tab[k][1][0] % 2 == 1 for k in ones)
    assert [j for j, l in tab[ones[0]]][0] == 2, "k = 1 with a correctly rounded expf"
    assert {(c0 // 4) // 64 for _, _, c0, _ in info} == {0, 1} and {c0 % 4 for _, _, c0, _ in info} >= {0, 2, 3}


def test_norm_gated_rope_lists_reach_their_branches():
    vp = {}
    for c in C.NORM_CASES:
        vp.setdefault(C.norm_geom(c.rows, c.cols)[0], set()).add(c.cols)
    assert vp == {1: {4, 12, 1000, 1024}, 2: {1028, 2048}, 4: {2052, 4096}, 8: {4100, 8192}}, vp
    for cols in (4, 1000, 1024, 1028, 2048, 2052, 4096, 4100, 8192):
        got = {(c.ln, c.delta, c.slots, c.bias) for c in C.NORM_CASES if c.cols == cols}
        assert got == {(ln, d, s, b) for ln, b in ((0, 0), (1, 0), (1, 1)) for d, s in ((0, 0), (1, 0), (1, 1))}
    wrap = [c for c in C.NORM_CASES if c.rows > 8192]
    assert {c.ln for c in wrap} == {0, 1} and all(c.rows == 8192 + 37 and C.norm_geom(c.rows, c.cols)[1] == 8192 for c in wrap)
    for c in wrap:
        x, d, w, b = C.norm_input(c)
        o = O.calib_norm_rows(x[list(C.NORM_WRAP_ROWS)], d[list(C.NORM_WRAP_ROWS)], w, b, C.NORM_EPS, c.ln)
        h = (x + d).astype(F32)
        assert {int(np.argmax(h.max(axis=1))), int(np.argmin(h.min(axis=1)))} <= set(C.NORM_WRAP_ROWS)
        assert {int(np.argmax(d.max(axis=1))), int(np.argmin(d.min(axis=1)))} <= set(C.NORM_WRAP_ROWS)
        y64 = O.calib_norm_rows(x, d, w, b, C.NORM_EPS, c.ln)["y64"] if c.id.endswith("v0") else None
        if y64 is not None:
            assert {int(np.argmax(y64.max(axis=1))), int(np.argmin(y64.min(axis=1)))} <= set(C.NORM_WRAP_ROWS)
    hi = {(int(c.id[-1]), c.ln): int(np.argmax((C.norm_input(c)[1]).max(axis=1))) for c in wrap}
    assert {hi[(v, 0)] for v in range(3)} == set(C.NORM_WRAP_ROWS)
    assert [C.gated_geom(n) for n in C.GATED_SIZES] == [(1, 1), (2, 1), (4, 1), (4096, 2)]
    assert C.gated_quads(C.GATED_SIZES[-1]) == [0, 4096 * 256 - 1, C.GATED_SIZES[-1] // 4 - 1] and C.GATED_SIZES[-1] == 4194304 + 4 * 777
    for act in (0, 1):
        a = np.linspace(-3, 3, 600001)
        s = O.calib_gated(a.astype(F32), np.ones_like(a, dtype=F32), act)[1]
        assert abs(float(F32(a[np.argmin(s)])) - C.GATED_ARGMIN[act]) < 2e-5
    ge = {c.id: C.rope_geom(c) for c in C.ROPE_CASES}
    for qkv in (0, 1):
        g = [ge[c.id] for c in C.ROPE_CASES if c.qkv == qkv]
        assert any(x.trips == 2 for x in g) and any(x.dq == 256 and x.hstep == 1 for x in g)
        assert any(x.dq == 3 and x.dq_shift == -1 and 256 % x.dq for x in g) and any(x.dq_shift >= 0 for x in g), "dq = 3: no shift, an idle partial head slot"
    for c in C.ROPE_CASES:
        if ge[c.id].trips == 2:
            assert C.rope_plant_rows(c) == [8191, c.B * c.S - 1]
            q = C.rope_input(c)[0].reshape(c.B * c.S, -1)
            assert int(np.argmax(q.max(axis=1))) == 8191 and int(np.argmin(q.min(axis=1))) == c.B * c.S - 1


# ---- oracles against independent restatements -------------------------------------------------------------------------------------------
def test_calib_probs_is_torch_softmax_at_float64():
    for c in (C.PROBS_CASES[4], C.PROBS_CASES[5]):
        raw, mask = C.probs_input(c)
        o = O.calib_probs(raw, C.INV_SQRT_D, mask=mask)
        x = (torch.from_numpy(raw.copy()) * float(C.INV_SQRT_D))
        assert x.dtype == torch.float32
        if mask is not None:
            x = x + torch.from_numpy(mask).repeat(c.rows // c.mask_rows, 1)
        assert np.array_equal(x.numpy().view(np.uint32), o["x"].view(np.uint32))
        want = torch.softmax(x.double(), -1).numpy()
        assert np.abs(o["p"] - want).max() <= 4e-16 and np.abs(o["p"].sum(axis=1) - 1).max() < 1e-14
        assert np.array_equal(o["p"] == 0, o["masked"])
    c = C.CAUSAL_CASES[2]
    raw = C.causal_base(c)
    o = O.calib_probs(raw, C.INV_SQRT_D, causal=True)
    S = c.seq
    x = torch.from_numpy(raw.copy()).view(c.blocks, S, S) * float(C.INV_SQRT_D) + torch.full((S, S), float("-inf")).triu(1)
    want = torch.softmax(x.double(), -1).numpy().reshape(-1, S)
    assert np.abs(o["p"] - want).max() <= 4e-16 and not o["nan_row"].any()
    for seq in C.ODD_SEQ:                                             # the NaN disposition is torch's
        raw, _ = C.odd_input(seq)
        o = O.calib_probs(raw, C.INV_SQRT_D, causal=True)
        x = torch.from_numpy(raw).view(3, seq, seq) * float(C.INV_SQRT_D) + torch.full((seq, seq), float("-inf")).triu(1)
        t = torch.softmax(x.double(), -1).numpy().reshape(-1, seq)
        assert np.array_equal(np.isnan(t).all(axis=1), o["nan_row"]) and np.array_equal(np.isnan(t).any(axis=1), o["nan_row"])


def test_calib_norm_and_gated_are_torch_at_float64():
    for c in (C.NORM_CASES[0], C.NORM_CASES[14], C.NORM_CASES[17], C.NORM_CASES[35]):
        x, d, w, b = C.norm_input(c)
        o = O.calib_norm_rows(x, d, w, b, C.NORM_EPS, c.ln)
        h = torch.from_numpy(x) + torch.from_numpy(d) if d is not None else torch.from_numpy(x)
        assert np.array_equal(h.numpy().view(np.uint32), o["h"].view(np.uint32))
        h64, w64 = h.double(), torch.from_numpy(w).double()
        if c.ln:
            want = torch.nn.functional.layer_norm(h64, (c.cols,), w64, torch.from_numpy(b).double() if b is not None else None, float(F32(C.NORM_EPS)))
        else:
            want = w64 * (h64 * torch.rsqrt(h64.pow(2).mean(-1, keepdim=True) + float(F32(C.NORM_EPS))))
        assert np.abs(o["y64"] - want.numpy()).max() <= 1e-14 * max(1.0, float(want.abs().max()))
    a, b = (t.copy() for t in C.gated_base(1028))
    for act, fn in ((0, torch.nn.functional.silu), (1, torch.nn.functional.gelu)):
        p, s = O.calib_gated(a, b, act)
        ws = fn(torch.from_numpy(a).double())
        assert np.abs(s - ws.numpy()).max() <= 1e-15 * 8 and np.abs(p - (ws * torch.from_numpy(b).double()).numpy()).max() <= 1e-13


def test_calib_rope_is_apply_rope_bit_for_bit():
    from mobilequant_amd import llama
    for c in C.ROPE_CASES:
        if c.B * c.S > 1000:
            continue
        q, k, v, cos, sin = C.rope_input(c)
        tc, ts = torch.from_numpy(cos), torch.from_numpy(sin)
        rep = c.H // c.KV if c.qkv else 1
        for x, H, r in ((q, c.H, 1), (k, c.KV, rep)):
            want = llama.apply_rope(torch.from_numpy(x).view(c.B, c.S, H, c.D).transpose(1, 2), tc, ts)
            want = want[:, :, None].expand(c.B, H, r, c.S, c.D).reshape(c.B, H * r, c.S, c.D).contiguous().numpy()
            got = O.calib_rope(x, H, c.D, cos, sin, True, r)
            assert got.dtype == F32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), c.id
        if c.qkv:
            got = O.calib_rope(v, c.KV, c.D, cos, sin, False, rep)
            want = torch.from_numpy(v).view(c.B, c.S, c.KV, c.D).transpose(1, 2).repeat_interleave(rep, dim=1).numpy()
            assert np.array_equal(got, want)


# ---- the replay search --------------------------------------------------------------------------------------------------------------------
def _block_sum(t, vpt):
    """The kernel's summation shape in fp32: t [nvec, 4] -> (a + b) + (c + d) per vector, a lane's vectors (lane + 256 k) one after the
    other, a pairwise tree over the 64 lanes of a wave, (s0 + s1) + (s2 + s3) over the waves."""
    q = ((t[:, 0] + t[:, 1]).astype(F32) + (t[:, 2] + t[:, 3]).astype(F32)).astype(F32)
    lanes = np.zeros((vpt, 256), F32)
    lanes.reshape(-1)[:q.size] = q
    acc = lanes[0].copy()
    for k in range(1, vpt):
        acc = (acc + lanes[k]).astype(F32)
    acc = acc.reshape(4, 64)
    while acc.shape[1] > 1:
        acc = (acc[:, 0::2] + acc[:, 1::2]).astype(F32)
    return F32(F32(acc[0, 0] + acc[1, 0]) + F32(acc[2, 0] + acc[3, 0]))


def _fp32_row_scalars(h, cols, eps, ln):
    """The row scalars in fp32 with the kernel's reduction shape (the order inside the wave tree is one of the orders the bound covers)."""
    vpt = C.norm_geom(1, cols)[0]
    t = h.reshape(-1, 4)
    if not ln:
        return F32(0), F32(F32(1) / np.sqrt(F32(F32(_block_sum((t * t).astype(F32), vpt) / F32(cols)) + F32(eps))))
    mu = F32(_block_sum(t, vpt) / F32(cols))
    d = (t - mu).astype(F32)
    return mu, F32(F32(1) / np.sqrt(F32(F32(_block_sum((d * d).astype(F32), vpt) / F32(cols)) + F32(eps))))


@pytest.mark.parametrize("idx", [1, 4, 7, 29, 31, 80])
def test_norm_replay_admits_the_fp32_statistic_and_rejects_one_ulp(idx):
    c = C.NORM_CASES[idx]
    x, d, w, b = C.norm_input(c)
    o = O.calib_norm_rows(x, d, w, b, C.NORM_EPS, c.ln)
    n_mu, n_r = O.calib_norm_n_red(c.cols, c.ln)
    for i in range(c.rows):
        h = o["h"][i]
        cand = o["cand"][i]
        assert all(len(rs) <= n_r + 8 for _, rs in cand), "r candidates capped by gamma(n_r + 2) / 2 + 2 u"
        if c.ln:
            cap = 2 * O._gamma(n_mu) * 1.001 * np.abs(h.astype(np.float64)).sum() / c.cols / np.spacing(np.abs(F32(h.astype(np.float64).mean()))) + 2
            assert len(cand) <= cap and len(cand) <= 256, (len(cand), cap)
        else:
            assert len(cand) == 1
        mu, r = _fp32_row_scalars(h, c.cols, C.NORM_EPS, c.ln)
        y = O.calib_norm_emit(h, mu, r, w, b, c.ln)
        hits = O.calib_norm_replay(y, h, cand, w, b, c.ln)
        assert any(m == mu and rr == r for m, rr in hits), (c.id, i, mu, r)
        j = int(np.argmax(np.abs(y)))
        y2 = y.copy()
        y2[j] = np.nextafter(y[j], F32(np.inf))
        assert O.calib_norm_replay(y2, h, cand, w, b, c.ln) == [], (c.id, i, "one ulp moved")
