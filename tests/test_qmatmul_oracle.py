"""CPU checks of the mq_qmatmul and mq_w8a8_linear_grouped pins (no GPU): the case files qmatmul_cases.py / grouped_gemm_cases.py are held
to what test_gpu_qmatmul.py / test_gpu_gemm_grouped.py rely on.

  * the dispatch predicate qmatmul_cases.choose equals the library's own mq_qmatmul_geometry on every case and over a sweep of 27 000
    shapes, memory orders, alignments and x1 spans around every threshold of the launcher;
  * the case lists reach all 28 instantiations of mq_qmatmul, every (kernel family, epilogue cause) pair, and both instantiations of
    the grouped kernel;
  * every case meets its conditions: planted ties are ties (of both parities), their neighbours are 1 and 2 ulp away, the limit case's
    accumulators are the stated integers, grouped brackets fit int32 and sit on conversion ties, nothing passes through saturation;
  * every deliberate mutation of either oracle changes the expected output of a named case;
  * oracle.qmatmul_launch equals oracle.qmatmul_exact bit for bit on the inputs of test_gpu_round5.QMM_CASES."""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import grouped_gemm_cases as G  # noqa: E402
import qmatmul_cases as C  # noqa: E402
from oracle import mq_oracle as O  # noqa: E402

F32 = np.float32
GEOMETRY_FIELDS = ("panel", "a16", "bkm", "rf", "kc", "vec", "a_vec", "b_vec", "o_vec", "tiles_m", "tiles_n", "nsplit", "tiles_per_split", "nblk")
ORDINARY = ("u4", "u6", "u8", "u8b", "i8", "u12", "i12", "u16", "i16")
RANDOM = [c for c in C.CASES if c.content == "random"]


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _geometry(batch, M, N, K, kcontig, al1, al2, alo, span1):
    """(status, dict | None) from the library."""
    from mobilequant_amd import _lib as L
    lib = L.load()
    ch = L.MqQmatmulChoice()
    rc = lib.mq_qmatmul_geometry(batch, M, N, K, int(kcontig), int(al1), int(al2), int(alo), float(span1), ctypes.byref(ch))
    return rc, ({f: int(getattr(ch, f)) for f in GEOMETRY_FIELDS} if rc == 0 else None)


# ---- the predicate against the library ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", C.CASES, ids=lambda c: c.id)
def test_kernel_of_matches_the_library(c):
    g1 = C.GRIDS[c.g1]
    rc, got = _geometry(c.batch, c.M, c.N, c.K, c.kcontig, c.a_off % 16 == 0, c.b_off % 16 == 0, c.o_off % 16 == 0, g1[3] - g1[2])
    want = C.kernel_of(c)
    assert rc == 0 and got == {f: want[f] for f in GEOMETRY_FIELDS}, (c.id, got, want)
    assert c.kcontig or (c.N % 4 == 0 and c.b_off % 16 == 0)       # what the launcher requires of an N-contiguous x2


def test_predicate_matches_the_library_over_a_sweep_of_thresholds():
    """M 64 / 65 / 255 / 256, N 64 / 65, K 64 / 65 / 128 / 129 / 256 / 257, the 512-tile switch to 128-row tiles (batch 170 / 171 at M 257,
    255 / 256 at M 256) and the 2048-workgroup column split (batch 512 ... 2049 against one row panel and five column tiles); memory
    order, the three alignments and the x1 span cycle through all their combinations."""
    Ms = [1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 384]
    Ns = [4, 63, 64, 65, 128, 132, 260, 516]
    Ks = [4, 9, 63, 64, 65, 127, 128, 129, 255, 256, 257]
    Bs = [1, 2, 128, 170, 171, 255, 256, 512, 682, 683, 1024, 2047, 2048, 2049]
    combos = list(itertools.product((0, 1), (0, 1), (0, 1), (0, 1), (15.0, 255.0, 256.0, 65535.0)))      # kcontig, al1, al2, alo, span
    n = served = refused = 0
    seen = set()
    for i, (B, M, N, K) in enumerate(itertools.product(Bs, Ms, Ns, Ks)):
        for rep in range(2):
            kc, al1, al2, alo, span = combos[(7 * i + 31 * rep) % len(combos)]
            if not kc:
                al2 = 1                                             # (an unaligned N-contiguous x2 is an argument error)
            rc, got = _geometry(B, M, N, K, kc, al1, al2, alo, span)
            n += 1
            if not kc and N % 4:
                assert rc == 3, (B, M, N, K, rc)                    # MQ_EUNSUPPORTED, as mq_qmatmul itself answers
                refused += 1
                continue
            want = C.choose(B, M, N, K, kc, al1, al2, alo, span)
            assert rc == 0 and got == {f: want[f] for f in GEOMETRY_FIELDS}, ((B, M, N, K, kc, al1, al2, alo, span), got, want)
            seen.add(C.kernel_name(want))
            served += 1
    assert n > 5000 and refused > 100 and sorted(seen) == C.ALL_KERNELS, (n, refused, sorted(set(C.ALL_KERNELS) - seen))


def test_k_beyond_the_accumulators_is_refused_before_any_launch():
    """K = 131071 is the last K the int32 accumulators hold (K x 128 x 128 < 2^31); 131072 is MQ_EUNSUPPORTED from both entry points."""
    from mobilequant_amd import _lib as L
    lib = L.load()
    assert _geometry(1, 3, 4, 131071, 1, 1, 1, 1, 255.0)[0] == 0 and _geometry(1, 3, 4, 131072, 1, 1, 1, 1, 255.0)[0] == 3
    p = ctypes.c_void_p(0x10000)
    g = L.MqGrid(p, p, 0.0, 255.0)
    assert lib.mq_qmatmul(p, p, p, 1, 3, 4, 131072, 1, ctypes.byref(g), ctypes.byref(g), None, None) == 3
    assert b"131071" in lib.mq_last_error()


# ---- coverage ---------------------------------------------------------------------------------------------------------------------------
def test_the_case_list_reaches_every_instantiation_and_every_epilogue_route():
    reached = sorted({C.kernel_of(c)["name"] for c in C.CASES})
    assert reached == C.ALL_KERNELS and len(reached) == 28, sorted(set(C.ALL_KERNELS) - set(reached))
    pairs = set().union(*(C.route_pairs(c) for c in C.CASES))
    assert sorted(pairs & set(C.REQUIRED_ROUTES)) == C.REQUIRED_ROUTES, sorted(set(C.REQUIRED_ROUTES) - pairs)
    plains = {(("panel" if C.kernel_of(c)["panel"] else "tile"), C.epilogue_route(c)[0]) for c in C.CASES}
    assert plains == {(f, p) for f in ("panel", "tile") for p in (0, 1, 2)}
    g = [C.kernel_of(c) for c in C.CASES]
    # the shape facts the issue names
    assert any(k["panel"] and k["nsplit"] > 1 for k in g) and any(k["panel"] and k["tiles_m"] > 1 and k["tiles_per_split"] > 1 for k in g)
    assert {k["nblk"] % 8 == 0 for k in g if k["panel"]} == {True, False}
    assert any(not k["panel"] and k["rf"] == 2 and 0 < (c.M - 1) % 128 + 1 <= 64 for c, k in zip(C.CASES, g))       # the break on row blocks
    assert any(not k["panel"] and c.K % 64 and (c.K + 63) // 64 > 2 and k["nblk"] > 1 for c, k in zip(C.CASES, g))    # partial chunk mid-loop
    for bkm in (0, 1):       # panel, not VEC: once through K % 4, once through a base 4 bytes past a 16-byte boundary
        nv = [c for c, k in zip(C.CASES, g) if k["panel"] and not k["vec"] and k["bkm"] == bkm]
        assert any(c.K % 4 for c in nv) and any(c.K % 4 == 0 and c.N % 4 == 0 and (c.a_off or c.o_off) for c in nv), bkm
    used = {c.g1 for c in C.CASES} | {c.g2 for c in C.CASES}
    assert set(ORDINARY) <= used
    assert sorted({G.kernel_of(c) for c in G.CASES}) == G.ALL_KERNELS


def test_no_operand_scale_is_a_power_of_two():
    for name, g in C.GRIDS.items():
        assert (F32(g[0]).view(np.uint32) & 0x007FFFFF) != 0, name
        assert g[3] - g[2] <= 255 or name in ("u12", "i12", "u16", "i16")


# ---- every case meets its conditions ----------------------------------------------------------------------------------------------------
def _tie_census(x, s):
    """(ties of even floor, ties of odd floor, elements 1 ulp from a tie, 2 ulp from a tie) of the fp32 quotients x / s."""
    x = np.asarray(x, F32).reshape(-1)
    x = x[np.isfinite(x)]

    def ties(v):
        with np.errstate(all="ignore"):
            t = (v / F32(s)).astype(F32).astype(np.float64)
            return np.isfinite(t) & (t - np.floor(t) == 0.5), t
    is_tie, t = ties(x)
    b = x.view(np.int32).astype(np.int64)
    near = []
    for d in (1, 2):
        hit = np.zeros(x.shape, bool)
        for sgn in (d, -d):
            nb = (b + sgn).astype(np.int32).view(F32)
            hit |= ties(nb)[0] & ~is_tie
        near.append(int(hit.sum()))
    fl = np.floor(t[is_tie]).astype(np.int64)
    return int((fl % 2 == 0).sum()), int((fl % 2 != 0).sum()), near[0], near[1]


@pytest.mark.parametrize("c", RANDOM, ids=lambda c: c.id)
def test_random_cases_hold_their_planted_values_and_do_not_saturate(c):
    g1, g2, go = C.grids_of(c)
    x1, x2m = C.operands(c.id)
    e = C.expect(c.id)
    for x, g, name in ((x1, g1, c.g1), (x2m, g2, c.g2)):
        assert C.clamped(x, g).mean() < 0.05, (c.id, name, C.clamped(x, g).mean())
        stored, _ = O.quantize_storage(x.reshape(-1, c.K) if x is x1 or c.kcontig else x.reshape(-1, c.N), np.array([g[0]], F32),
                                       np.array([g[1]], F32), int(g[2]), int(g[3]), 0)
        ref = e["ia"] if x is x1 else (np.swapaxes(e["ib"], 1, 2) if c.kcontig else e["ib"])
        assert np.array_equal(stored.reshape(ref.shape), ref)          # image_index IS quantize_storage's logic
        if x.size >= 4096 and name in ORDINARY:
            even, odd, one, two = _tie_census(x, g[0])
            assert even >= 1 and odd >= 1 and one >= 1 and two >= 1, (c.id, name, even, odd, one, two)
            assert np.isnan(x).any() and np.isposinf(x).any() and np.isneginf(x).any(), (c.id, name)
            idx = (e["ia"] if x is x1 else e["ib"])
            assert (idx == g[2]).any() and (idx == g[3]).any()
    if x1.shape[1] * c.K >= 64:          # planted in the last real k of the last row (x1) / of the last column (x2)
        sp1 = np.array(C._specials(g1), F32).view(np.uint32)
        assert all(x1[b, -1, -1].view(np.uint32) in sp1 for b in range(c.batch)), c.id
    if c.N * c.K >= 64:
        x2 = C.logical_x2(c)
        sp2 = np.array(C._specials(g2), F32).view(np.uint32)
        assert all(x2[b, -1, -1].view(np.uint32) in sp2 for b in range(c.batch)), c.id
    if go is not None and c.degenerate is None:
        idx = e["idx"]
        assert np.isfinite(idx).all(), c.id
        on_clamp = np.mean((idx == go[2]) | (idx == go[3]))
        distinct = np.unique(idx).size
        assert on_clamp < 0.02 and distinct >= min(64, (go[3] - go[2] + 1) / 4), (c.id, on_clamp, distinct)


def test_degenerate_cases_are_what_they_say():
    for c in C.CASES:
        if c.degenerate is None:
            continue
        out = C.expect(c.id)["out"]
        if "NaN" in c.degenerate and "most" not in c.degenerate:
            assert np.isnan(out).all(), c.id
        elif "most" in c.degenerate:
            assert 0.5 < np.isnan(out).mean() < 1.0 and np.isinf(C.expect(c.id)["v"]).any(), c.id
        else:
            assert np.all(out == 0), c.id
    plain = C.expect("tile-overflow-plain")["out"]
    assert np.isposinf(plain).any() and np.isneginf(plain).any() and np.isfinite(plain).any()


def test_alpha_cases_straddle_the_bound():
    for cid, above in (("panel-alpha-below", False), ("tile-alpha-below", False), ("panel-alpha-above", True), ("tile-alpha-above", True)):
        a = float(C.expect(cid)["alpha"])
        assert (a > 2.0 ** 30) == above and abs(a / 2.0 ** 30 - 1) < 1e-4, (cid, a)


@pytest.mark.parametrize("cid", ["panel-out-ties", "tile-out-ties"])
def test_output_tie_cases_put_every_odd_bracket_on_an_exact_tie(cid):
    c = C.BY_ID[cid]
    e = C.expect(cid)
    g1, g2, go = C.grids_of(c)
    assert float(e["alpha"]) == g1[0] * g2[0] == 15 * 2.0 ** -15 and go[0] == 2 * float(e["alpha"])
    odd = e["t"] % 2 != 0
    assert np.array_equal(e["tie"] == 0, odd) and np.array_equal(e["q"].astype(np.float64), e["t"] / 2.0)
    fl = np.floor(e["q"][odd].astype(np.float64)).astype(np.int64)
    assert (fl % 2 == 0).sum() > 100 and (fl % 2 != 0).sum() > 100
    assert not np.any((e["idx"] == go[2]) | (e["idx"] == go[3]))


@pytest.mark.parametrize("cid", ["limit-8bit", "limit-16bit"])
def test_limit_cases_fill_the_accumulators_to_the_stated_integers(cid):
    c = C.BY_ID[cid]
    e = C.expect(cid)
    a1, b1 = C.stored_operands(c, e)
    K = 131071
    assert c.K == K
    if cid == "limit-16bit":            # two byte planes, each minus 128
        u = a1 + 32896
        planes = [(u & 255) - 128, (u >> 8) - 128]
    else:
        planes = [a1]
    for p in planes:
        assert p.min() >= -128 and p.max() <= 127
        acc = np.matmul(p.astype(np.float64), b1.astype(np.float64)).astype(np.int64)[0]
        assert acc[0, 0] == K * 2 ** 14 == 2 ** 31 - 2 ** 14 and acc[0, 1] == -K * 128 * 127          # a' = b' = -128; the mixed-sign twin
        assert acc[-1, 0] == -K * 128 * 127 and acc[-1, 1] == K * 127 * 127
        assert np.abs(acc).max() < 2 ** 31
    assert np.isfinite(e["out"]).all()


# ---- mutations -------------------------------------------------------------------------------------------------------------------------
QMM_DETECTED_BY = {"scale64": "panel-fits32-offsets", "in_half_up": "panel-kT-kc1-vec", "out_half_up": "panel-out-ties",
                   "nan_qmax": "tile-kT-K260", "no_zero_row": "panel-kn-kc1-vec"}
GROUPED_DETECTED_BY = {"mul_add": "g64-G2", "reverse": "g256-G3", "bracket_f64": "ties-g2048-G3"}


def test_every_mutation_of_the_qmatmul_oracle_is_detected():
    assert sorted(QMM_DETECTED_BY) == sorted(O.QMATMUL_MUTATIONS)
    for m, cid in QMM_DETECTED_BY.items():
        assert not _same_bits(C.expect(cid, m)["out"], C.expect(cid)["out"]), (m, cid)
    assert not _same_bits(C.expect("tile-out-ties", "out_half_up")["out"], C.expect("tile-out-ties")["out"])
    assert not _same_bits(C.expect("tile-fits32-offsets", "scale64")["out"], C.expect("tile-fits32-offsets")["out"])


def test_every_mutation_of_the_grouped_oracle_is_detected():
    assert sorted(GROUPED_DETECTED_BY) == sorted(O.GROUPED_MUTATIONS)
    for m, cid in GROUPED_DETECTED_BY.items():
        assert not _same_bits(G.expect(cid, m)["out"], G.expect(cid)["out"]), (m, cid)
    for cid in ("ties-g2112-G2", "mul24-g64-G3", "big-g32768-G2"):
        assert not _same_bits(G.expect(cid, "bracket_f64")["out"], G.expect(cid)["out"]), cid


# ---- the new oracle against the existing one -------------------------------------------------------------------------------------------
def test_qmatmul_launch_equals_qmatmul_exact_on_the_round5_inputs():
    import test_gpu_round5 as R5
    for case in R5.QMM_CASES:
        lead, M, N, K, kt, (b1, s1), (b2, s2), bo = case
        rng = np.random.default_rng(1000 * M + N + K)               # the generation of test_integer_qmatmul_..., line for line
        if b1 > 8 and not s1:
            a = rng.random(lead + (M, K), dtype=np.float32) ** 4
            a /= a.sum(-1, keepdims=True)
            g1 = R5._grid(b1, s1, 0.0, float(a.max()))
        else:
            a = (rng.standard_normal(lead + (M, K), dtype=np.float32) * 1.3 + 0.2).astype(np.float32)
            g1 = R5._grid(b1, s1, float(a.min()) * 0.9, float(a.max()) * 0.9)
        b = (rng.standard_normal(lead + (K, N), dtype=np.float32) * 0.8 - 0.1).astype(np.float32)
        g2 = R5._grid(b2, s2, float(b.min()) * 0.95, float(b.max()) * 0.95)
        fp = np.matmul(a, b)
        go = None if bo is None else R5._grid(bo[0], bo[1], float(np.percentile(fp, 0.5)), float(np.percentile(fp, 99.5)))
        want = O.qmatmul_exact(a, b, g1, g2, go)
        t = lambda g: None if g is None else (float(g.scale), float(g.offset), float(g.qmin), float(g.qmax))      # noqa: E731
        got = O.qmatmul_launch(a.reshape(-1, M, K), b.reshape(-1, K, N), t(g1), t(g2), t(go))["out"].reshape(want.shape)
        assert _same_bits(got, want), case


# ---- grouped GEMM cases ----------------------------------------------------------------------------------------------------------------
def test_grouped_cases_cover_the_issue_and_stay_inside_the_domain():
    by_kernel = {k: [c for c in G.CASES if G.kernel_of(c) == k] for k in G.ALL_KERNELS}
    assert {64, 192, 320} <= {c.gs for c in by_kernel["bks64"]} and {128, 256, 384} <= {c.gs for c in by_kernel["bks128"]}
    for cs in by_kernel.values():
        gs_ = {c.G for c in cs}
        assert {1, 2, 3} <= gs_ and max(gs_) >= 5 and {c.bias for c in cs} == {True, False}
    assert {1, 127, 128, 129, 300} <= {c.M for c in G.CASES} and {128, 384} <= {c.N for c in G.CASES}
    big = G.BY_ID["big-g32768-G2"]
    assert (big.gs, big.N, big.M) == (32768, 128, 16)
    for c in G.CASES:
        p, e = G.problem(c.id), G.expect(c.id)                      # grouped_linear asserts |cw|, |a_gsum| < 2^23 and int32 brackets
        br = e["bracket"]
        assert br.shape == (c.G, c.M, c.N) and br.min() >= -2 ** 31 and br.max() < 2 ** 31 and np.isfinite(e["out"]).all(), c.id
        if c.content == "ties":
            assert c.gs >= 2048
            sat = br[:, :G.SAT_ROWS, :]
            assert np.array_equal(sat, np.broadcast_to(G.tie_targets(c.G, c.N)[:, None, :], sat.shape)) and G.is_conversion_tie(sat).all(), c.id
            assert np.abs(sat).min() > 2 ** 24
            f = sat.astype(F32).astype(np.int64)                    # the two parities: ties that round down in magnitude and up
            assert (np.abs(f) < np.abs(sat)).any() and (np.abs(f) > np.abs(sat)).any() and (sat > 0).any() and (sat < 0).any()
        if c.content == "mul24":
            prod = p["cw"].astype(np.int64)[:, None, :] * p["a_gsum"].astype(np.int64)[:, :, None]
            assert set(np.unique(p["cw"])) == {-(2 ** 23 - 1), 2 ** 23 - 1} and 2 ** 30 < np.abs(prod).max() < 2 ** 31
        if c.content == "big":
            assert br[:, 0, 0].min() > 2 ** 29 - 2 ** 28 and p["a_gsum"].min() == -2 ** 22
