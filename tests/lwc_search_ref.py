"""The clip search (mq_lwc_search) restated in numpy from its definition, and the case list of its GPU test.  A helper, not a test.

Definition (csrc/mq_lwc_search.hip).  For row r of w [rows, cols] and candidate c:
    y      = oracle.lwc_fused_forward(w, sig_lo[c], sig_hi[c], bitwidth, is_symmetric)["y"]   -- the bits mq_lwc_fake_quant writes
    e      = float32(y - w)                                    on the rounded y
    term   = (float64(e) * float64(e)) * float64(col_weight[(r % (cw_len / cols)) * cols + k])   (no col_weight: the square alone)
    cost   = the sum of the row's terms -- here math.fsum, the correctly rounded sum
Selection: candidate 0 is the incumbent, a later candidate replaces the best so far only if its cost is strictly smaller; NaN never wins.

Tolerance (derived, not measured).  The kernel's terms are the helper's bit for bit: e is one fp32 subtraction of the same operands, its
square is exact in fp64 (48 significant bits), the weighting is one fp64 multiplication of the same operands.  Only the order of the
sum over L = cols non-negative terms differs: any order of fp64 additions is within (L - 1) * 2^-53 * sum (1 + O(L * 2^-53)) of the exact
sum, fsum within 2^-53 of it, hence |cost - ref| <= 2 * L * 2^-53 * ref =: TOL(L) * ref.
"""
import functools
import math

import numpy as np

from oracle import mq_oracle as O

F32 = np.float32


def TOL(L: int) -> float:
    return 2.0 * L * 2.0 ** -53


def row_cw_index(rows: int, cols: int, cw_len: int):
    """[rows, cols] indices into col_weight: row r uses (r % (cw_len / cols)) * cols + i."""
    per = cw_len // cols
    return (np.arange(rows)[:, None] % per) * cols + np.arange(cols)[None, :]


def cost_table(w, sig_lo, sig_hi, bitwidth, is_symmetric, col_weight=None):
    """costs [rows, C] float64 by the definition above (NaN where the row holds a NaN)."""
    w = np.asarray(w, F32)
    rows, cols = w.shape
    sig_lo, sig_hi = np.asarray(sig_lo, F32), np.asarray(sig_hi, F32)
    cw = None
    if col_weight is not None:
        col_weight = np.asarray(col_weight, F32)
        assert col_weight.size % cols == 0
        cw = col_weight[row_cw_index(rows, cols, col_weight.size)].astype(np.float64)
    out = np.empty((rows, sig_lo.size), np.float64)
    for c in range(sig_lo.size):
        y = O.lwc_fused_forward(w, np.full(rows, sig_lo[c], F32), np.full(rows, sig_hi[c], F32), bitwidth, is_symmetric)["y"]
        with np.errstate(all="ignore"):
            e = (y - w).astype(F32).astype(np.float64)
            t = e * e
            if cw is not None:
                t = t * cw
        for r in range(rows):
            out[r, c] = math.fsum(t[r]) if np.isfinite(t[r]).all() else float(np.sum(t[r]))
    return out


def first_min(costs):
    """The selection rule on a cost table: index [rows] of the first strict minimum, scanning from candidate 0."""
    costs = np.asarray(costs, np.float64)
    idx = np.zeros(costs.shape[0], np.int32)
    for r in range(costs.shape[0]):
        best = costs[r, 0]
        for c in range(1, costs.shape[1]):
            if costs[r, c] < best:
                best, idx[r] = costs[r, c], c
    return idx


def classify(costs, L):
    """Per row: 'nan' (a NaN cost), 'tie' (all candidates cost the same), 'clear' (the best DIFFERENT cost is more than 4 * TOL(L) above
    the best, relatively) or 'ambiguous'."""
    out = []
    for row in np.asarray(costs, np.float64):
        if np.isnan(row).any():
            out.append("nan")
            continue
        best = row.min()
        others = row[row != best]
        if others.size == 0:
            out.append("tie")
        elif others.min() - best > 4.0 * TOL(L) * best:
            out.append("clear")
        else:
            out.append("ambiguous")
    return out


# ---- data ---------------------------------------------------------------------------------------------------------------------------
N_SPECIAL = 5
OUTLIER = 0.3          # ~ 10 sigma of the Student-t(4) * 0.02 bulk: clipping it pays on 4-bit rows of >= 1024 columns (checked by the host test)


def make_weight(rows, cols, seed, specials=False):
    """Student-t(4) * 0.02; with specials the first five rows are: all-zero, constant, all-positive, one outlier, one NaN."""
    rng = np.random.default_rng(seed)
    w = (rng.standard_t(4, size=(rows, cols)) * 0.02).astype(F32)
    if specials:
        assert rows > N_SPECIAL
        w[0] = 0.0
        w[1] = F32(0.0371)
        w[2] = np.abs(w[2]) + F32(1e-3)
        w[3, cols // 3] = F32(OUTLIER)
        w[4, cols - 2] = np.nan
    return w


def ratio_table(C, lo=0.5):
    """C ratios from sigmoid(4) down to lo, fp32 (C = 1: the init alone)."""
    top = 1.0 / (1.0 + math.exp(-4.0))
    return np.linspace(top, lo, C).astype(F32) if C > 1 else np.array([top], F32)


def make_col_weight(cols, mode, seed):
    """None | 'row' (one vector [cols]) | 'grouped' ([4 * cols]: row r uses block r % 4) -- squares of positive scales, two decades wide."""
    if mode is None:
        return None
    rng = np.random.default_rng(seed + 7)
    n = cols if mode == "row" else 4 * cols
    s = np.exp(rng.uniform(np.log(0.05), np.log(5.0), size=n)).astype(F32)
    return (s * s).astype(F32)


# ---- the GPU test's cases -------------------------------------------------------------------------------------------------------------
# geometry switches of csrc/mq_lwc_search.hip: lane form <= 128 < wave form <= 1024 < workgroup form (4 vectors / thread) <= 4096 < (16)
SWITCHES = (128, 1024, 4096)
GRIDS = ((2, False), (2, True), (4, False), (4, True), (8, False), (8, True))
NOT_4BIT = ((2, False), (8, True), (2, True), (8, False))
CW_MODES = (None, "row", "grouped")
# one representative per geometry takes every grid x every col_weight mode at C = 64 and every other C on both 4-bit grids
REPRESENTATIVES = ((8, 64), (3, 1024), (2, 2052), (1, 16384))
# (rows, cols): the issue's shapes, both sides of every switch +-4, and row counts that leave a partly filled workgroup in the
# several-rows-per-workgroup forms (lane form: 64 rows per workgroup -> 70, 67, 8, 5; wave form: 4 -> 6, 3, 7)
SHAPES = ((8, 16), (5, 128), (70, 124), (67, 128), (6, 132), (3, 1020), (7, 1024), (6, 1028), (2, 4092), (2, 4096), (6, 4100))


def _case(rows, cols, bits, sym, C, cw, mode="joint", specials=False):
    return dict(rows=rows, cols=cols, bits=bits, sym=sym, C=C, cw=cw, mode=mode, specials=specials)


def build_cases():
    cases = []
    for rows, cols in REPRESENTATIVES:
        for bits, sym in GRIDS:
            for cw in CW_MODES:
                cases.append(_case(rows, cols, bits, sym, 64, cw))
        for C in (1, 2, 1024):
            for sym in (False, True):
                cases.append(_case(rows, cols, 4, sym, C, None))
    for i, (rows, cols) in enumerate(SHAPES):
        sp = rows > N_SPECIAL
        cases.append(_case(rows, cols, 4, False, 64, CW_MODES[i % 3], specials=sp))
        cases.append(_case(rows, cols, 4, True, 64, CW_MODES[(i + 1) % 3], specials=sp))
        bits, sym = NOT_4BIT[i % 4]
        cases.append(_case(rows, cols, bits, sym, 64, None, specials=sp))
    for rows, cols in ((5, 128), (3, 1024)):                     # the cross product of an 8-entry table with itself, asymmetric 4 bits
        cases.append(_case(rows, cols, 4, False, 64, None, mode="independent"))
    return cases


CASES = build_cases()


def case_id(c):
    return (f"{c['rows']}x{c['cols']}-w{c['bits']}{'s' if c['sym'] else 'a'}-C{c['C']}-{c['cw'] or 'plain'}"
            + ("-indep" if c["mode"] == "independent" else "") + ("-special" if c["specials"] else ""))


def case_seed(c):
    return 1000 * c["cols"] + 10 * c["rows"] + c["bits"] + (5 if c["sym"] else 0)


def case_inputs(c):
    """(w, sig_lo, sig_hi, col_weight) of a case, numpy fp32."""
    seed = case_seed(c)
    w = make_weight(c["rows"], c["cols"], seed, c["specials"])
    if c["mode"] == "independent":
        n = int(round(math.sqrt(c["C"])))
        t = ratio_table(n)
        lo, hi = np.repeat(t, n), np.tile(t, n)
    else:
        lo = hi = ratio_table(c["C"])
    return w, lo, hi, make_col_weight(c["cols"], c["cw"], seed)


@functools.lru_cache(maxsize=None)
def _reference(i):
    c = CASES[i]
    w, lo, hi, cw = case_inputs(c)
    costs = cost_table(w, lo, hi, c["bits"], c["sym"], cw)
    costs.setflags(write=False)
    idx = first_min(costs)
    idx.setflags(write=False)
    return costs, idx, tuple(classify(costs, c["cols"]))


def reference(i):
    """(costs [rows, C] float64, best_idx [rows], classes) of CASES[i]: computed once per process, shared, read-only."""
    return _reference(i)
