"""Operands, grids, case lists and the restated launch geometry of the M <= 8 weight-streaming GEMV pin (gemv_i8_fat_kernel of
csrc/mq_gemv.hip behind mq_w8a8_linear, mq_w4a8_linear and their _f32in forms), built once for the CPU checks (test_gemv_oracle.py) and
the GPU comparison (test_gpu_linear_gemv.py): both files take every tensor, grid and case from here.

Columns, by n % 32 (gemm_cases.COL_CLASS), in the GEMV's own form  q = rint(fl(fl(fl(float(tt) alpha) + bias) fl(1 / s))) + o:
  tie (0..5)     few non-zero effective weights in -8..7, alpha = (c / 2^k) s and bias = b s with c odd and b an integer: under a
                 power-of-two scale (Case.p2) every step is exact, f inv = tt c / 2^k + b, a half-integer whenever tt c = 2^(k-1) mod 2^k
  near (6..9)    the tie column n - 6 again with the bias moved by -2, -1, +1, +2 ulp
  generic (10..19)  full-range weights, zero points at both extremes (+-255, packed weights 0 / 15), non-dyadic alpha, random bias
  sat (20..25)   an alpha four grid widths wide: both clamps; the zero row lands one step outside, on and one step inside either end
  big (26..31)   col_term of +-(2^25 .. 2^30): |tt| > 2^24, the int32 -> fp32 conversion rounds; in column 31 col_term is chosen so that
                 row 0's exact sum leaves int32 and wraps
Rows (ROW_CLASS): low magnitude (-2..1), the full int8 range with both extremes, row 2 all zero.
The _f32in cases build x from the same target image on the activation grid, then overwrite SPECIALS per row: exact ties of x / s of
both parities, one ulp either side (toward and away from zero), both clamps, NaN, +-inf, -0.0.

geometry() restates run_gemv and the kernel's loop bounds; locate() names where in the launch an output is produced."""
import functools
import zlib
from collections import namedtuple

import numpy as np

import gemm_cases as G
from oracle import mq_oracle as O

F32 = np.float32
GRIDS, NONE_STORAGE, COL_CLASS, COL_PERIOD = G.GRIDS, G.NONE_STORAGE, G.COL_CLASS, G.COL_PERIOD
TIE_CK, NEAR_ULPS, SAT_STEPS, col_classes = G.TIE_CK, G.NEAR_ULPS, G.SAT_STEPS, G.col_classes
BIG_CT = (2, -4, 9, -30, 70)                                       # col_term of big columns 26..30 in units of 2^24; 31 wraps
ROW_CLASS = np.array(["low", "full", "zero", "low", "full", "low", "full", "low"])
ZERO_ROW = 2
ROWSUM_DELTA = np.array([3, -7, 0, 1, 11, -2, 5, -1])              # "off": what the caller's a_rowsum differs by (0 on the zero row)
# the activation grids of the _f32in entries: (scale, offset, qmin, qmax, shift)
A_GRIDS = {"u8": (F32(0.0625), F32(131.0), 0, 255, 128), "s8": (F32(0.0371), F32(3.0), -128, 127, 0)}
ENTRIES = {"w8a8": (False, False), "w4a8": (False, True), "w8a8_f32in": (True, False), "w4a8_f32in": (True, True)}   # (FUSEQ, W4)
LDS_LIMIT = 64 * 1024 - 64                                         # M K at most this many bytes of staged activations

Case = namedtuple("Case", "id entry M N K grid p2 bias rowsum agrid")


def _case(entry, M, N, K, grid="u8", p2=False, bias=True, rowsum="true", agrid="u8"):
    fuse, _ = ENTRIES[entry]
    cid = "%s-%dx%dx%d-%s%s%s" % (entry, M, N, K, grid, "-p2" if p2 else "", "" if bias else "-nobias")
    cid += ("-a" + agrid) if fuse else ("" if rowsum == "true" else "-rs" + rowsum)
    return Case(cid, entry, M, N, K, grid, p2, bias, None if fuse else rowsum, agrid if fuse else None)


def fuse_of(c):
    return ENTRIES[c.entry][0]


def w4_of(c):
    return ENTRIES[c.entry][1]


def storage_of(c):
    g = GRIDS[c.grid]
    return NONE_STORAGE[c.grid] if g is None else g.storage


# ---- geometry, restated ---------------------------------------------------------------------------------------------------------
WAVES, INFLIGHT, MAX_SLOTS = 16, 8, 64
Geometry = namedtuple("Geometry", "kchunks cpl rows_per_wg grid nslots passes_per_row MT cus")


def takes_gemv(M, K):
    return M <= 8 and M * K <= LDS_LIMIT


def f32in_accepts(M, K):
    return takes_gemv(M, K) and K % 256 == 0


def instantiation(c):
    return (1 if c.M == 1 else 2 if c.M == 2 else 4, fuse_of(c), w4_of(c))


def geometry(c, cus=256):
    """run_gemv's launch and the kernel's loop bounds: 16-byte chunks per weight row, chunks per lane per row, rows per workgroup (one
    fat workgroup per CU, at most 16 waves x 64 row slots), workgroups, the row slots of wave 0 of workgroup 0 (the most any wave has),
    load passes a row's chunks touch at most."""
    kchunks = c.K >> 5 if w4_of(c) else c.K >> 4
    cpl = (kchunks + 63) >> 6
    rpw = min(-(-c.N // cus), WAVES * MAX_SLOTS)
    grid = -(-c.N // rpw)
    nslots = -(-min(rpw, c.N) // WAVES)
    spans = max(((t * cpl + cpl - 1) // INFLIGHT) - (t * cpl // INFLIGHT) + 1 for t in range(min(nslots, 8)))
    return Geometry(kchunks, cpl, rpw, grid, nslots, spans, instantiation(c)[0], cus)


def locate(c, n, cus=256):
    """(workgroup, wave, row slot, pass, chunk slot) in which output column n completes."""
    g = geometry(c, cus)
    r = n % g.rows_per_wg
    last = (r // WAVES) * g.cpl + g.cpl - 1
    return n // g.rows_per_wg, r % WAVES, r // WAVES, last // INFLIGHT, last % INFLIGHT


def geometry_classes(c, cus=256):
    """The branches of the launch that case c reaches on a device of `cus` compute units."""
    g = geometry(c, cus)
    out = set()
    if g.cpl > INFLIGHT:
        out.add("multi_pass")                                      # issue_pass and the consume loop continue in mid-row
        if g.cpl % INFLIGHT & 1:
            out.add("odd_phase")                                   # a row starts at an odd chunk slot of a pass
    if g.cpl == INFLIGHT:
        out.add("cpl8")
    if g.cpl == 16 and not w4_of(c):
        out.add("w8_cpl16")
    if g.kchunks % 64:
        out.add("partial_chunk_slot")
    if w4_of(c) and g.kchunks == 4:
        out.add("w4_four_lanes")
    if g.nslots == MAX_SLOTS:
        out.add("slots64")                                         # every lane of the parameter registers is read
    if g.nslots >= 9:
        out.add("slots9")
    if -(-c.N // cus) > WAVES * MAX_SLOTS:
        out.add("rows_clamp")
    if g.grid > cus:
        out.add("more_wgs_than_cus")
    if c.N < cus:
        out.add("fewer_rows_than_cus")                             # one row per workgroup: 15 waves leave after the barrier
    if c.N % g.rows_per_wg:
        out.add("ragged_last_wg")
    if g.MT == 4 and c.M > 4 and c.M % 4:
        out.add("partial_second_group")
    if not takes_gemv(c.M, c.K + (256 if fuse_of(c) else 128)):
        out.add("lds_limit")
    return out


# ---- operands -------------------------------------------------------------------------------------------------------------------
def _seed(*parts):
    return zlib.crc32(repr(parts).encode())


def _ulps(v, d):
    v = np.asarray(v, F32)
    return (v.view(np.int32) + np.where(v >= 0, d, -d).astype(np.int32)).view(F32)


def target_image(M, K):
    """int8 [M, K]: rows by ROW_CLASS."""
    rng = np.random.default_rng(_seed("a", M, K))
    a = rng.integers(-2, 2, size=(M, K), dtype=np.int8)
    for m in range(M):
        if ROW_CLASS[m] == "full":
            a[m] = rng.integers(-128, 128, size=K, dtype=np.int8)
            a[m, 0], a[m, K - 1] = -128, 127
        elif ROW_CLASS[m] == "zero":
            a[m] = 0
    return a


def _solve_div(target, s):
    """An fp32 x with fl(x / s) == target, or None."""
    x0 = F32(F32(target) * F32(s))
    for d in (0, 1, -1, 2, -2, 3, -3, 4, -4):
        x = _ulps(np.array([x0], F32), d)[0]
        if F32(x / F32(s)) == F32(target):
            return x
    return None


@functools.lru_cache(maxsize=2)
def specials(agrid):
    """[(name, fp32 x)] of the adversarial activations on grid `agrid`: t = x / s in front of rint(t) + o, clamp."""
    s, o, qmin, qmax, _ = A_GRIDS[agrid]
    out = []
    for e in (-40, -37, -4, -3, 2, 5, 30, 33):                      # floor of the tie: both parities, both signs
        x = _solve_div(e + 0.5, s)
        if x is not None:
            out.append(("tie_%s" % ("even" if e % 2 == 0 else "odd"), x))
            out.append(("tie_ulp_in", _ulps(np.array([x], F32), -1)[0]))
            out.append(("tie_ulp_out", _ulps(np.array([x], F32), 1)[0]))
    lo, hi = float(qmin) - float(o), float(qmax) - float(o)
    for name, t in (("lo_out", lo - 3), ("lo_on", lo), ("lo_in", lo + 1), ("hi_in", hi - 1), ("hi_on", hi), ("hi_out", hi + 5),
                    ("lo_far", -1e30), ("hi_far", 1e30)):
        out.append((name, F32(t * float(s))))
    out += [("nan", F32(np.nan)), ("pinf", F32(np.inf)), ("ninf", F32(-np.inf)), ("negzero", F32(-0.0))]
    return tuple(out)


N_SPECIAL_SLOTS = 40                                               # positions kept for SPECIALS in every row (at most this many)


def special_positions(K, n):
    return (np.arange(n) * 37 + 5) % K                             # (37 is coprime to every K here: distinct, spread over the lanes)


def activations_f32(M, K, agrid):
    """fp32 [M, K]: the target image placed on the grid, SPECIALS written over every row but the zero row."""
    s, o, _, _, shift = A_GRIDS[agrid]
    x = ((target_image(M, K).astype(np.float64) + shift - float(o)) * float(s)).astype(F32)
    sp = specials(agrid)
    assert len(sp) <= N_SPECIAL_SLOTS
    pos = special_positions(K, len(sp))
    for m in range(M):
        if ROW_CLASS[m] != "zero":
            x[m, pos] = np.array([v for _, v in sp], F32)
    return x


@functools.lru_cache(maxsize=2)
def weights(N, K, w4, span):
    """(w stored integers int8 [N, K] (packed weights: the unsigned nibbles 0..15), w_zp int32 [N], col_term int64 [N] -- column 31's
    is finished in problem())."""
    rng = np.random.default_rng(_seed("w", N, K, w4, span))
    cls = col_classes(N)
    j = np.arange(N) % COL_PERIOD
    lo, hi = (0, 16) if w4 else (-128, 128)
    w = rng.integers(lo, hi, size=(N, K), dtype=np.int8)
    zp = rng.integers(0, 16, size=N) if w4 else rng.integers(-255, 256, size=N)
    gen = np.flatnonzero(cls == "generic")
    zp[gen[0::10]], zp[gen[1::10]] = (15, 0) if w4 else (255, -255)
    ct = rng.integers(-4000, 4000, size=N).astype(np.int64)
    tie = np.flatnonzero(cls == "tie")
    ck = np.array(TIE_CK, np.float64)[j[tie]]
    target = span / 5.0 / (ck[:, 0] / 2.0 ** ck[:, 1])
    nnz = np.clip(np.rint((target / (1.1 * 4.6)) ** 2), 4, K)       # (gemm_cases._tie_nnz)
    eff = np.where(rng.random((len(tie), K)) < (nnz / K)[:, None], rng.integers(-8, 8, size=(len(tie), K)), 0)
    eff[:, special_positions(K, N_SPECIAL_SLOTS)] = 0                # the fused cases' adversarial activations stay out of the tie columns
    zp[tie] = 8 if w4 else rng.integers(-1, 2, size=len(tie))
    w[tie] = (eff + zp[tie][:, None]).astype(np.int8)
    ct[tie] = rng.integers(-3, 4, size=len(tie)) + np.rint(0.5 * eff.sum(axis=1)).astype(np.int64)
    near = np.flatnonzero(cls == "near")
    w[near], zp[near], ct[near] = w[near - 6], zp[near - 6], ct[near - 6]
    ct[cls == "sat"] = 0
    big = np.flatnonzero((cls == "big") & (j < 31))
    ct[big] = np.array(BIG_CT, np.int64)[j[big] - 26] * (1 << 24) + rng.integers(-(1 << 20), 1 << 20, size=len(big)) * 2 + 1
    assert w.min() >= lo and w.max() < hi
    return w, zp.astype(np.int32), ct


Problem = namedtuple("Problem", "a a_rowsum x agrid image rs_true w w_packed w_zp col_term alpha bias out_grid tt")


@functools.lru_cache(maxsize=2)
def problem(c):
    """Every operand of case c and its accumulators."""
    g = GRIDS[c.grid]
    M, N, K = c.M, c.N, c.K
    fuse, w4 = ENTRIES[c.entry]
    span = 255 if g is None else g.qmax - g.qmin
    if fuse:
        x, agrid = activations_f32(M, K, c.agrid), A_GRIDS[c.agrid]
        stored, _ = O.quantize_storage(x, agrid[0], agrid[1], agrid[2], agrid[3], agrid[4])
        image, a, a_rowsum = stored.astype(np.int8), None, None
    else:
        x, agrid = None, None
        image = a = target_image(M, K)
    rs_true = image.astype(np.int64).sum(axis=1)
    if fuse or c.rowsum == "true":
        rs = rs_true
    elif c.rowsum == "off":
        rs = rs_true + ROWSUM_DELTA[:M]
    else:
        rs = np.zeros(M, np.int64)
    if not fuse:
        a_rowsum = None if c.rowsum == "null" else rs.astype(np.int32)
    w, zp, ct = weights(N, K, w4, span)
    ct = ct.copy()
    cls = col_classes(N)
    low = ROW_CLASS[:M] == "low"
    tn = (cls == "tie") | (cls == "near")                            # keep the tie columns centred under a caller's row sum that is off
    ct[tn] += np.rint(zp[tn] * float((rs - rs_true)[low].mean())).astype(np.int64)
    base = O._contract_rows(image, w, False) - zp.astype(np.int64)[None, :] * rs[:, None]
    rng = np.random.default_rng(_seed("e", c.id))
    j = np.arange(N) % COL_PERIOD
    wrap = np.flatnonzero(j == 31)                                   # row 0's exact sum leaves int32 by 1 .. 50
    b0 = base[0, wrap]
    r = rng.integers(1, 51, size=len(wrap))
    ct[wrap] = np.where(b0 > 60, (1 << 31) - b0 + r - 1, np.where(b0 < -60, -(1 << 31) - b0 - r, 70 * (1 << 24) + 1))
    assert ct.min() >= -(1 << 31) and ct.max() < (1 << 31)
    tt = O._wrap32(base + ct[None, :])
    if g is None:
        sc, oo, qmin, qmax, out_grid = F32(0.0371), F32(128.0), 0.0, 255.0, None        # (only shape alpha and bias)
    else:
        sc, oo, qmin, qmax = F32(g.scale_p2 if c.p2 else g.scale), F32(g.offset), float(g.qmin), float(g.qmax)
        out_grid = (sc, oo, qmin, qmax)
    s64, o64, centre = float(sc), float(oo), (qmin + qmax) / 2
    tl = tt.astype(np.float64)
    floor = np.sqrt(K) * 1.1 * (4.6 if w4 else 74.0)
    mean, std = tl.mean(axis=0), np.maximum(tl.std(axis=0), floor)
    full = ROW_CLASS[:M] == "full"
    std_full = np.maximum(tl[full].std(axis=0), floor) if full.sum() > 1 else std * (64.0 if not full.any() else 1.0)
    # generic / big
    a1 = span / 4.0 / std * np.where(cls == "generic", 1.0 + 0.3 * rng.random(N), 1.0)
    b1 = centre - mean * a1 + np.where(cls == "generic", rng.standard_normal(N) * span / 10.0, 0.0)
    # sat
    sat = cls == "sat"
    step = np.array([(qmin if s[:2] == "lo" else qmax) + {"-1": -1, "": 0, "+1": 1}[s[2:]] + 0.3 for s in SAT_STEPS])
    a1 = np.where(sat, 4.0 * span / std_full, a1)
    b1 = np.where(sat, step[np.clip(j - 20, 0, 5)], b1)
    if not c.bias and g is not None:                                 # no bias to place a column with: col_term does it
        gen = cls == "generic"
        shift = np.where(gen, -np.rint(mean), 0.0)
        ct_n = np.rint((b1 - o64) / a1)
        ct_n = np.where(ct_n == 0, 1.0, ct_n)
        a1 = np.where(sat, (b1 - o64) / ct_n, a1)
        shift = np.where(sat, ct_n, shift).astype(np.int64)
        ct += shift
        tt = O._wrap32(tt.astype(np.int64) + shift[None, :])
    alpha = (a1 * s64).astype(F32)
    bias = ((b1 - o64) * s64).astype(F32)
    # tie / near
    jt = np.where(cls == "near", j - 6, j)[tn]
    ck = np.array(TIE_CK, np.float64)[jt]
    alpha[tn] = (ck[:, 0] / 2.0 ** ck[:, 1] * s64).astype(F32)
    b_int = np.rint(centre - o64) + (jt % 3) - 1
    b_int = np.where((span >= 255) & (np.abs(b_int) < 48), b_int + 64, b_int)
    b_int = np.where(b_int == 0, 1, b_int)
    bt = (b_int * s64).astype(F32)
    nr = cls[tn] == "near"
    bt[nr] = _ulps(bt[nr], np.array(NEAR_ULPS)[j[tn][nr] - 6])
    bias[tn] = bt
    if not c.bias:
        bias = None
    return Problem(a, a_rowsum, x, agrid, image, rs_true, w, O.pack_w4(w, 0) if w4 else None, zp, ct.astype(np.int32), alpha, bias,
                   out_grid, tt)


def oracle_args(c, p=None):
    """The keyword arguments of oracle.linear_gemv_launch for case c."""
    p = p or problem(c)
    w4 = w4_of(c)
    return dict(w=p.w_packed if w4 else p.w, alpha=p.alpha, w_zp=p.w_zp, col_term=p.col_term, bias=p.bias, a=p.a, a_rowsum=p.a_rowsum,
                x=p.x, a_grid=p.agrid, w4=w4, out_grid=p.out_grid, out_dtype=storage_of(c))


@functools.lru_cache(maxsize=2)
def expect(c):
    return O.linear_gemv_launch(**oracle_args(c))


def conditions(c):
    """What test_gemv_oracle.py holds the cases to, from the oracle alone (see gemm_cases.conditions)."""
    p, e = problem(c), expect(c)
    assert np.array_equal(e["tt"], p.tt)
    g = GRIDS[c.grid]
    cls = col_classes(c.N)
    t64 = p.tt.astype(np.int64)
    big = np.abs(t64) > (1 << 24)
    rs = np.zeros(c.M, np.int64) if (not fuse_of(c) and p.a_rowsum is None) else (p.rs_true if fuse_of(c) else p.a_rowsum.astype(np.int64))
    exact = O._contract_rows(p.image, p.w, False) - p.w_zp.astype(np.int64)[None, :] * rs[:, None] + p.col_term.astype(np.int64)[None, :]
    out = {"big": int(big.sum()), "big_rounds": int((big & (p.tt.astype(F32).astype(np.int64) != t64)).sum()),
           "wraps": int((exact != t64).sum()), "zp_hi": int((p.w_zp == (15 if w4_of(c) else 255)).sum()),
           "zp_lo": int((p.w_zp == (0 if w4_of(c) else -255))[cls == "generic"].sum()),
           "rowsum_off": int((rs != p.rs_true).sum())}
    if g is None:
        return out
    oo = float(g.offset)
    r = np.rint(e["v"]) + oo
    fl = np.floor(e["v"]) + oo
    is_tie = (e["tie"] == 0.0) & (fl >= g.qmin) & (fl + 1 <= g.qmax)
    out["tie_even"] = int((is_tie & (np.floor(e["v"]) % 2 == 0)).sum())
    out["tie_odd"] = int((is_tie & (np.floor(e["v"]) % 2 == 1)).sum())
    near = cls == "near"
    out["near_tie"] = int(((e["tie"][:, near] > 0) & (e["tie"][:, near] < 1e-3)).sum()) if near.any() else 0
    sat = cls == "sat"
    out["sat_lo"] = int((r[:, sat] < g.qmin).sum()) if sat.any() else 0
    out["sat_hi"] = int((r[:, sat] > g.qmax).sum()) if sat.any() else 0
    for name, v in (("lo-1", g.qmin - 1), ("lo", g.qmin), ("lo+1", g.qmin + 1), ("hi-1", g.qmax - 1), ("hi", g.qmax), ("hi+1", g.qmax + 1)):
        out[name] = int((r == v).sum())
    return out


# ---- case lists -----------------------------------------------------------------------------------------------------------------
INSTANTIATIONS = [(mt, fuse, w4) for mt in (1, 2, 4) for fuse in (False, True) for w4 in (False, True)]
ENTRY_OF = {v: k for k, v in ENTRIES.items()}
MT4_ROWS = (3, 4, 5, 6, 7, 8)
TYPE_SHAPE = (580, 256)                                            # 3 rows per workgroup at 256 CUs, 194 workgroups, the last with one row

TYPE_CASES = []                                                    # every instantiation meets every output grid of gemm_cases
for _i, (_mt, _fuse, _w4) in enumerate(INSTANTIATIONS):
    for _gi, _g in enumerate(GRIDS):
        _m = _mt if _mt < 4 else MT4_ROWS[(_gi + _i) % 6]
        TYPE_CASES.append(_case(ENTRY_OF[(_fuse, _w4)], _m, TYPE_SHAPE[0], TYPE_SHAPE[1], _g, p2=bool((_gi + _i) & 1) or _g == "u8",
                                bias=(_gi + _i) % 5 != 0, rowsum=("true", "off", "null")[(_gi + 2 * _i) % 3], agrid=("u8", "s8")[(_gi + _i // 2) & 1]))

GEOMETRY_CASES = [
    _case("w8a8", 1, 4, 128, "u8", p2=True),                                      # one workgroup per row, four of them
    _case("w4a8", 2, 180, 128, "i8u", rowsum="off"),                              # packed weights, four active lanes
    _case("w8a8_f32in", 4, 180, 256, "s8", agrid="s8"),
    _case("w4a8_f32in", 5, 4100, 256, "u16", agrid="s8"),
    _case("w8a8", 8, 4100, 1152, "u8", p2=True, rowsum="off"),                    # a partially filled last chunk slot
    _case("w4a8", 6, 4100, 1152, "f32_8"),
    _case("w8a8", 7, 580, 8192, "u8"),                                            # cpl = 8: a row is exactly one pass
    _case("w4a8", 3, 580, 16384, "s8", p2=True),
    _case("w8a8_f32in", 7, 580, 9216, "i16", agrid="u8"),                         # the largest M K of the _f32in entries; cpl = 9
    _case("w8a8", 1, 4100, 8320, "u8", p2=True),                                  # cpl = 9: rows straddle passes at an odd phase
    _case("w8a8", 2, 4100, 8320, "f16_8", rowsum="null"),
    _case("w8a8", 6, 4100, 8320, "i8u", p2=True, rowsum="off"),
    _case("w8a8", 7, 4100, 8320, "u16", bias=False),
    _case("w8a8_f32in", 1, 4100, 8448, "s8", agrid="s8"),
    _case("w8a8_f32in", 2, 4100, 8448, "u8", p2=True, agrid="u8"),
    _case("w8a8_f32in", 7, 4100, 8448, "none32", agrid="s8"),
    _case("w4a8", 1, 4100, 16640, "u8", p2=True),                                 # packed weights, cpl = 9
    _case("w4a8", 2, 4100, 16640, "i16", rowsum="off"),
    _case("w4a8", 3, 4100, 16640, "f32_16", p2=True),
    _case("w4a8_f32in", 1, 4100, 16640, "u4", agrid="u8"),
    _case("w4a8_f32in", 2, 4100, 16640, "none16", agrid="s8"),
    _case("w4a8_f32in", 3, 4100, 16640, "u8", p2=True, agrid="u8"),
    _case("w8a8", 3, 4100, 16384, "u8", p2=True),                                 # Gemma's w2: cpl = 16
    _case("w8a8_f32in", 1, 580, 16384, "i8u", agrid="u8"),
    _case("w8a8", 1, 180, 65408, "u8", p2=True),                                  # the largest K: M K + 64 = 65 472 bytes of LDS, cpl = 64
    _case("w4a8", 1, 180, 65408, "s8", rowsum="off"),
    _case("w8a8", 2, 32772, 256, "u8", p2=True),                                  # 9 row slots
    _case("w4a8_f32in", 3, 32772, 256, "f16_16", agrid="s8"),
    _case("w8a8", 2, 258052, 128, "u8", p2=True, rowsum="off"),                   # 1009 rows per workgroup: 64 row slots
    _case("w4a8_f32in", 1, 258052, 256, "i8u", agrid="u8"),
    _case("w8a8_f32in", 1, 262152, 256, "u8", p2=True, agrid="s8"),               # the rows_per_wg clamp: 257 workgroups
    _case("w4a8", 3, 262152, 256, "none32"),
]
ALL_CASES = TYPE_CASES + GEOMETRY_CASES
MULTI_PASS_CASES = [c for c in GEOMETRY_CASES if c.N == 4100 and c.K in (8320, 8448, 16640)]

# what the lists have to reach on a 256-CU device (and, re-evaluated with its own CU count, on the device in hand)
GEOMETRY_CLASSES = ("multi_pass", "odd_phase", "cpl8", "w8_cpl16", "partial_chunk_slot", "w4_four_lanes", "slots64", "slots9", "rows_clamp",
                    "more_wgs_than_cus", "fewer_rows_than_cus", "ragged_last_wg", "partial_second_group", "lds_limit")

# the M = 8 / M = 9 seam through mq_w8a8_linear: one operand set, the first eight rows equal
SEAM_SHAPE = (580, 256)
SEAM_GRIDS = (("none32", False), ("u8", True), ("u8", False), ("u16", False))
# over the limit from the other side: the int8 entries go to the GEMM, the _f32in entries refuse
OVER_LIMIT = ((1, 65536), (8, 8192), (7, 9472))

# Which cases a mutation of the oracle is BOUND to change (test_gemv_oracle.py holds each of them to a changed stored element).  A mutation
# can move other cases too; these are the ones where the operands force it:
#   fma               a bias (fma(t, alpha, 0) IS the rounded product) and an output that resolves the last bit of f: no grid, or a
#                     16-bit grid (on an 8-bit grid a changed ulp of f shows only next to a rounding boundary)
#   divide            a scale that is no power of two (fl(1 / s) is exact otherwise), a 16-bit grid and at least 16 384 outputs: f / s and
#                     f fl(1 / s) differ in the last bit of a value of up to 2^16, which crosses a boundary about once in 2^9 elements
#   half_up           exact ties above an even floor: the tie columns under a power-of-two scale
#   fold_offset       the same ties and an odd offset (rint(h + o) and rint(h) + o round a tie h to different parities); s8's offset is 0
#   gemm_form         a grid, unless every step of both forms is exact and the offset stays behind the rint (power-of-two scale, no bias,
#                     16-bit or offset 0): the near columns, the big columns and (8-bit) the folded odd offset differ
#   rowsum_recomputed the int8 entries with a caller's a_rowsum that is off or NULL
def _grid(c):
    return GRIDS[c.grid]


def _wide(c):
    return _grid(c) is not None and _grid(c).qmax - _grid(c).qmin > 255


MUTATION_BEARS = {
    "fma": lambda c: c.bias and c.N >= COL_PERIOD and (_grid(c) is None or _wide(c)),
    "divide": lambda c: _wide(c) and not c.p2 and c.M * c.N >= 16384,
    "half_up": lambda c: _grid(c) is not None and c.p2 and c.N >= COL_PERIOD,
    "fold_offset": lambda c: _grid(c) is not None and c.p2 and c.N >= COL_PERIOD and _grid(c).offset % 2 == 1,
    "gemm_form": lambda c: _grid(c) is not None and c.N >= COL_PERIOD and not (c.p2 and not c.bias and (_wide(c) or _grid(c).offset == 0)),
    "rowsum_recomputed": lambda c: not fuse_of(c) and c.rowsum != "true",
}
