"""Inputs, case lists and launch-geometry predicates of the training-pass pin (csrc/mq_fake_quant.hip: mq_fake_quant_backward,
mq_lwc_fake_quant(_backward), mq_attention_probs_train(_backward)), built once for the CPU checks (test_train_oracle.py) and the GPU
comparison (test_gpu_train.py): both files take every tensor, grid, case and count from here, so what runs on the GPU is what the CPU
file has checked.

The geometry functions (fqb_geom, lwc_vpt, attn_fwd_geom, attn_bwd_geom, attn_fast and the *_classes maps from an element to its trip,
unroll slot, wave and slice) restate the host launch code; test_train_oracle.py holds every case list to the branches it has to reach.

Sums.  A kernel's sum is held to gamma_n * sum|term| around the float64 sum of the oracle's terms, n counted here from the launch geometry
(adds per thread, 6 in the wave, 2 in the workgroup, one per workgroup for the atomics).  That bar looks loose -- 1e-4 of sum|term| behind
2048 atomics -- so the GRADIENTS ARE DESIGNED: the incoming gradient takes the sign that makes the terms of a sum agree, and `boost`
raises it by powers of two on every position class whose share would otherwise be small, until dropping any one class (a trip, an
unroll slot, a wave, a slice) moves the float64 sum by at least 8 bars.  sensitivity() measures exactly that and the CPU file asserts it."""
import functools
import math
import zlib
from collections import namedtuple

import numpy as np

from oracle import mq_oracle as O

F32, F64 = np.float32, np.float64
U = O.U32
SENS = 8.0                                  # a dropped class has to move a sum by this many bars
_TARGET = 2.0 * SENS                        # what boost() aims for


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def cdiv(a, b):
    return -(-a // b)


def gamma(n):
    return O._gamma(n)


# ---- the generic designed gradient ---------------------------------------------------------------------------------------------------------
def class_keys(group, cls, n_group):
    """One integer per element: (class, group) folded, so that np.bincount sums per class of every sum at once."""
    return cls.astype(np.int64) * n_group + group


def sensitivity(terms, bars, group, classes):
    """min over sums (groups) and position classes of |sum of the class's terms| / bar of its sum (float64 reference alone).  Classes without
    a non-zero term and sums whose bar is 0 (exact zeros) do not count.  -> (ratio, (class name, class id, group))."""
    t = np.asarray(terms, F64).reshape(-1)
    n_group = len(bars)
    worst, where = np.inf, None
    for name, cls in classes.items():
        key = class_keys(group, cls, n_group)
        cs = np.abs(np.bincount(key, weights=t))
        has = np.bincount(key, weights=(t != 0).astype(F64)) > 0
        ids = np.flatnonzero(has)
        b = np.asarray(bars, F64)[ids % n_group]
        ok = b > 0
        if not ok.any():
            continue
        r = cs[ids][ok] / b[ok]
        i = int(np.argmin(r))
        if r[i] < worst:
            worst, where = float(r[i]), (name, int(ids[ok][i] // n_group), int(ids[ok][i] % n_group))
    return worst, where


def boost(g, term_fn, group, n_group, classes, n_adds, rounds=8):
    """Multiply g by a power of two on every class whose signed share of a sum is under _TARGET bars, and again until none is.  term_fn(g)
    -> tuple of term arrays (each a sum per group); terms are linear in g, so a factor on g is the same factor on the class."""
    g = g.copy()
    gm = gamma(n_adds)
    for _ in range(rounds):
        changed = False
        for t in term_fn(g):
            t = np.nan_to_num(np.asarray(t, F64).reshape(-1), nan=0.0, posinf=0.0, neginf=0.0)
            need_g = _TARGET * gm * np.bincount(group, weights=np.abs(t), minlength=n_group)
            for cls in classes.values():
                key = class_keys(group, cls, n_group)
                cs = np.abs(np.bincount(key, weights=t))
                ca = np.bincount(key, weights=np.abs(t))
                need = need_g[np.arange(cs.size) % n_group]
                bad = (cs < need) & (ca > 0)
                if bad.any():
                    f = np.ones(cs.size)
                    f[bad] = np.exp2(np.clip(np.ceil(np.log2(need[bad] / np.maximum(cs[bad], 1e-300))) + 1, 1, 12))
                    g = (g.reshape(-1) * f[key].astype(F32)).astype(F32).reshape(g.shape)
                    changed = True
                    break
            if changed:
                break
        if not changed:
            return g
    return g


# ---- mq_fake_quant_backward -----------------------------------------------------------------------------------------------------------------
FqbGeom = namedtuple("FqbGeom", "kernel g stride trips n")
FqbGrid = namedtuple("FqbGrid", "bits sym scale offset")
FqbCase = namedtuple("FqbCase", "name rows cols n_scale offs grid nonfinite")

FQB_GRIDS = (FqbGrid(4, False, 2.0 ** -3, 6.0), FqbGrid(4, True, 0.0371, 0.0), FqbGrid(8, False, 0.0371, 101.0), FqbGrid(8, True, 2.0 ** -5, 0.0),
             FqbGrid(16, False, 2.0 ** -9, 26000.0), FqbGrid(16, True, 0.00113, 0.0), FqbGrid(8, False, 2.0 ** -5, -3.0))


def fqb_kernel(rows, cols, n_scale, offs=(0, 0, 0)):
    """Which of the three kernels mq_fake_quant_backward launches; offs: byte offsets of x, grad_y, grad_x past a 16-byte boundary."""
    if n_scale == rows and rows > 1:
        return "row"
    numel = rows * cols
    if numel >= 65536 and numel % 4 == 0 and all(o % 16 == 0 for o in offs):
        return "vec"
    return "scalar"


def fqb_geom(rows, cols, n_scale, offs=(0, 0, 0)):
    """kernel, workgroups g, stride of one trip (elements; vectors for the vector kernel, whose sweep is four strides), trips (sweeps) of
    lane 0 and n: the adds on the longest path of a sum -- per thread (one per element; four per vector and four vectors per sweep), 6 in
    the wave, 2 in the workgroup, one per workgroup in the atomics (1 for the per-row kernel: its slot starts at zero)."""
    k, numel = fqb_kernel(rows, cols, n_scale, offs), rows * cols
    if k == "row":
        trips = cdiv(cols, 256)
        return FqbGeom(k, rows, 256, trips, trips + 8 + 1)
    if k == "vec":
        nvec = numel // 4
        g = min(cdiv(nvec, 1024), 2048)
        sweeps = cdiv(nvec, 4 * g * 256)
        return FqbGeom(k, g, g * 256, sweeps, 16 * sweeps + 8 + g)
    g = min(max(cdiv(numel, 1024), 1), 512)
    trips = cdiv(numel, g * 256)
    return FqbGeom(k, g, g * 256, trips, trips + 8 + g)


def fqb_classes(rows, cols, n_scale, offs=(0, 0, 0)):
    """name -> class id of every element (flat order): the grid-stride trip (sweep), the unroll slot u of the vector kernel, the wave."""
    ge, numel = fqb_geom(rows, cols, n_scale, offs), rows * cols
    i = np.arange(numel, dtype=np.int64)
    if ge.kernel == "row":
        c = i % cols
        return {"trip": c // 256, "wave": (c % 256) // 64}
    if ge.kernel == "vec":
        j = i // 4
        return {"sweep": j // (4 * ge.stride), "u": (j // ge.stride) % 4, "wave": (j % 256) // 64}
    return {"trip": i // ge.stride, "wave": (i % 256) // 64}


def _fqb_cases():
    cs, k = [], 0

    def add(name, rows, cols, n_scale, offs=(0, 0, 0), grid=None, nonfinite=False):
        nonlocal k
        cs.append(FqbCase(name, rows, cols, n_scale, offs, FQB_GRIDS[k % len(FQB_GRIDS)] if grid is None else grid, nonfinite))
        k += 1
    for n in (1, 1023, 1152, 65535):
        add("scalar_%d" % n, 1, n, 1)
    for w, offs in (("x", (4, 0, 0)), ("gy", (0, 4, 0)), ("gx", (0, 0, 4))):
        add("scalar_65536_%s_off4" % w, 1, 65536, 1, offs)
    add("scalar_65538", 1, 65538, 1)
    add("scalar_trips", 1, 2 * 524288 + 259, 1)
    for n in (65536, 65540, 262148):
        add("vec_%d" % n, 4, n // 4, 1)
    add("vec_capped", 1, 8388608 + 4 * 524365, 1)
    for r, c in ((2, 1), (3, 96), (5, 255), (5, 256), (5, 257), (7, 1000), (4099, 8)):
        add("row_%dx%d" % (r, c), r, c, r)
    add("row_1x300_is_per_tensor", 1, 300, 1)
    for gi, gr in enumerate(FQB_GRIDS):                       # every grid on each kernel, and the non-finite inputs
        add("scalar_1152_grid%d" % gi, 1, 1152, 1, grid=gr)
        add("vec_65540_grid%d" % gi, 1, 65540, 1, grid=gr)
        add("row_7x1000_grid%d" % gi, 7, 1000, 7, grid=gr)
    add("scalar_1152_nonfinite", 1, 1152, 1, grid=FQB_GRIDS[2], nonfinite=True)
    add("vec_65540_nonfinite", 1, 65540, 1, grid=FQB_GRIDS[2], nonfinite=True)
    add("row_7x1000_nonfinite", 7, 1000, 7, grid=FQB_GRIDS[2], nonfinite=True)
    return tuple(cs)


FQB_CASES = _fqb_cases()
FQB_PLANT_KINDS = ("qmax", "qmin", "above", "below", "tie_hi_out", "tie_hi_in", "tie_lo_out", "tie_lo_in")


@functools.lru_cache(maxsize=2)
def fqb_inputs(case):
    """x, grad_y [rows, cols], scale, offset [n_scale], qmin, qmax, plants {kind: [(row, col)]}, nonfinite positions.  x is built in the
    quotient's domain: 70 % of the elements uniform over the grid, 15 % up to 3.6 steps beyond either end; planted: q exactly on qmax and
    qmin (the mask is inclusive), one step outside, and the four half-integers around the ends (exact ties under a power-of-two scale)."""
    rows, cols, gr = case.rows, case.cols, case.grid
    qmin, qmax = O.qrange(gr.bits, gr.sym)
    rng = _rng("fqb", case.name)
    per_row = fqb_kernel(rows, cols, case.n_scale, case.offs) == "row"
    r_idx = np.arange(rows)
    if per_row:
        s = (F32(gr.scale) * (1 + (r_idx % 3) * F32(0.25))).astype(F32)[:, None]
        o = (F32(gr.offset) + (r_idx % 2)).astype(F32)[:, None]
    else:
        s, o = np.full((1, 1), gr.scale, F32), np.full((1, 1), gr.offset, F32)
    lo_t, hi_t = (qmin - o).astype(F64), (qmax - o).astype(F64)
    kind = rng.choice(3, size=(rows, cols), p=[0.7, 0.15, 0.15])
    u01 = rng.random((rows, cols))
    t = np.where(kind == 0, lo_t + u01 * (hi_t - lo_t), np.where(kind == 1, hi_t + 0.6 + 3 * u01, lo_t - 0.6 - 3 * u01))
    plants = {k: [] for k in FQB_PLANT_KINDS}
    vals = (hi_t, lo_t, hi_t + 1, lo_t - 1, hi_t + 0.5, hi_t - 0.5, lo_t - 0.5, lo_t + 0.5)
    for r in range(rows if rows <= 8 else 8):
        used = set()
        for k in range(min(8, cols)):
            c = (k * 37 + r * 5) % cols
            if c in used:
                continue
            used.add(c)
            kk = (k + r) % 8
            t[r, c] = np.broadcast_to(vals[kk], (rows, 1))[r, 0]
            plants[FQB_PLANT_KINDS[kk]].append((r, c))
    x = (t.astype(F32) * s).astype(F32)
    nonfinite = []
    if case.nonfinite:
        flat = x.reshape(-1)
        nonfinite = [(flat.size // 3, np.nan), (2 * flat.size // 3, np.inf)]
    # the designed gradient: terms of grad_scale all of one sign (inside: sign of r - t; clamped high +, four times as large, clamped low -)
    b = O.fake_quant_backward_terms(x, np.ones_like(x), s, o, qmin, qmax)
    tt = b["t"].astype(F64)
    high = ~b["inside"] & (tt > hi_t)
    sgn = np.where(b["inside"], np.where(b["r"] >= b["t"], 1.0, -1.0), np.where(high, 4.0, -1.0))
    g = ((1 + rng.integers(0, 256, size=(rows, cols)) / 256.0) * sgn).astype(F32)
    geo = fqb_geom(rows, cols, case.n_scale, case.offs)
    group = np.repeat(np.arange(rows), cols) if per_row else np.zeros(rows * cols, np.int64)

    ts1, to1 = b["ts"].astype(F64), b["to"].astype(F64)            # the terms of g = 1: linear in g up to one rounding

    def terms(gv):
        return ts1 * gv, to1 * gv
    g = boost(g, terms, group, rows if per_row else 1, fqb_classes(rows, cols, case.n_scale, case.offs), geo.n)
    for pos, v in nonfinite:
        x.reshape(-1)[pos] = v
    n_s = rows if per_row else 1
    return dict(x=x, g=g, scale=np.ascontiguousarray(s.reshape(-1)[:n_s]), offset=np.ascontiguousarray(o.reshape(-1)[:n_s]), s2d=s, o2d=o,
                qmin=qmin, qmax=qmax, plants=plants, nonfinite=nonfinite, group=group, n_group=n_s)


def fqb_expect(case, mutation=None):
    """gx (fp32, exact), and per sum: float64 value, bar gamma_n * sum|term| (NaN value where a term is NaN: the kernel's sum is NaN too)."""
    d = fqb_inputs(case)
    b = O.fake_quant_backward_terms(d["x"], d["g"], d["s2d"], d["o2d"], d["qmin"], d["qmax"], mutation)
    geo = fqb_geom(case.rows, case.cols, case.n_scale, case.offs)
    out = dict(gx=b["gx"], ts=b["ts"], to=b["to"], n=geo.n)
    for name in ("ts", "to"):
        t = b[name].astype(F64).reshape(-1)
        out["sum_" + name] = np.bincount(d["group"], weights=t, minlength=d["n_group"])
        out["bar_" + name] = gamma(geo.n) * np.bincount(d["group"], weights=np.abs(np.nan_to_num(t, nan=0.0)), minlength=d["n_group"])
    return out


# ---- mq_lwc_fake_quant(_backward) -----------------------------------------------------------------------------------------------------------
LWC_COLS = (4, 64, 1020, 1024, 2048, 2052, 4096, 4100, 6144, 6148, 8192, 8196, 16384)
LWC_ROWS = (1, 5, 33)
LWC_GRIDS = tuple((b, s) for b in (2, 4, 8, 16) for s in (False, True))
LWC_KINDS = {1: ("plant",), 5: ("tie2", "zero", "nan", "plant", "plant"),
             33: ("tie2", "tie3", "const", "zero", "negzero_min", "nan", "pinf") + ("plant",) * 26}


def lwc_vpt(cols):
    return 2 if cols <= 2048 else 4 if cols <= 4096 else 6 if cols <= 6144 else 8 if cols <= 8192 else 16


def lwc_n(cols):
    """Adds on the longest path of the row sum: four per vector and VPT vectors per thread, 6 in the wave, 2 in the workgroup."""
    return 4 * lwc_vpt(cols) + 8


def lwc_classes(rows, cols):
    """Vector j = col / 4 belongs to thread j % 256: slice k = j / 256, wave (j % 256) / 64."""
    j = np.tile(np.arange(cols) // 4, rows)
    return {"k": j // 256, "wave": (j % 256) // 64}


def lwc_positions(cols):
    """Ordered {column: class}: one column in every (wave, k) a row of `cols` columns occupies, the four elements on either side of every
    1024 k boundary (the last vector of slice k - 1 at lane 255 and the first of slice k at lane 0) and the row's last vector."""
    nvec, pos = cols // 4, {}
    for k in range(cdiv(nvec, 256)):
        for w in range(4):
            j = 256 * k + 64 * w + (7 * k + 13 * w) % 64
            if j >= nvec:
                j = 256 * k + 64 * w                       # a partly filled wave: its first lane, if it has one
            if j < nvec:
                pos.setdefault(4 * j + (k + w) % 4, "wave%d_k%d" % (w, k))
    for k in range(1, cdiv(cols, 1024) + 1):
        for c in range(1024 * k - 4, 1024 * k + 4):
            if 0 <= c < cols:
                pos.setdefault(c, "slice%d_%s" % (k, "last" if c < 1024 * k else "first"))
    for c in range(cols - 4, cols):
        pos.setdefault(c, "row_last_vector")
    return pos


def _lwc_plant_index(bits, sym, rows, r):
    """A running count of the planted rows over every (grid, rows) combination of one width, so that their extremes walk through
    lwc_positions(cols) without gaps."""
    n = 0
    for g in LWC_GRIDS:
        for rr in LWC_ROWS:
            kinds = LWC_KINDS[rr]
            if (g, rr) == ((bits, sym), rows):
                return n + sum(1 for q in kinds[:r] if q == "plant")
            n += kinds.count("plant")
    raise KeyError((bits, sym, rows))


def lwc_plants(cols, bits, sym, rows, r):
    """(column of the unique maximum, column of the unique minimum) of planted row r."""
    p = list(lwc_positions(cols))
    i = _lwc_plant_index(bits, sym, rows, r)
    a = i % len(p)
    b = (i + len(p) // 2 + 1) % len(p)
    if b == a:
        b = (b + 1) % len(p)
    return p[a], p[b]


@functools.lru_cache(maxsize=4)
def lwc_inputs(cols, bits, sym, rows):
    """w, grad_y [rows, cols], sig_lo, sig_hi [rows], kinds.  Ordinary elements k / 1024 strictly inside (-1, 1); the sigmoids are small
    enough that a good part of every row clamps."""
    rng = _rng("lwc", cols, bits, sym, rows)
    w = (rng.integers(-1000, 1001, size=(rows, cols)) / 1024.0).astype(F32)
    kinds = LWC_KINDS[rows]
    ext = {}
    for r, kind in enumerate(kinds):
        if kind == "plant":
            a, b = lwc_plants(cols, bits, sym, rows, r)
            w[r, a], w[r, b] = 1.5, -1.25
            ext[r] = ((a,), (b,))
        elif kind == "tie2":
            w[r, cols - 1] = w[r, 1] = 1.5
            w[r, 2] = -1.25
            ext[r] = ((1, cols - 1), (2,))
        elif kind == "tie3":
            w[r, 0] = w[r, cols // 2] = w[r, cols - 1] = -1.25
            w[r, 1] = 1.5
            ext[r] = ((1,), tuple(sorted({0, cols // 2, cols - 1})))
        elif kind == "const":
            w[r] = 0.037
        elif kind == "zero":
            w[r] = 0.0
        elif kind == "negzero_min":
            w[r] = np.abs(w[r]) + F32(1.0 / 1024)
            w[r, 0], w[r, 1], w[r, 2], w[r, cols - 1] = 1.5, -0.0, 0.0, 0.0
        elif kind == "nan":
            w[r, cols - 2] = np.nan
        elif kind == "pinf":
            w[r, cols - 3] = np.inf
    r_idx = np.arange(rows)
    sig_lo = (0.3 + 0.05 * (r_idx % 8)).astype(F32)
    sig_hi = (0.95 - 0.06 * (r_idx % 7)).astype(F32)
    f = O.lwc_fused_forward(w, sig_lo, sig_hi, bits, sym)
    qmin, qmax = O.qrange(bits, sym)
    s, o = f["scale"][:, None], f["offset"][:, None]
    b = O.fake_quant_backward_terms(w, np.ones_like(w), s, o, qmin, qmax)
    with np.errstate(all="ignore"):
        high = ~b["inside"] & (b["t"] > (qmax - o))
    sgn = np.where(b["inside"], np.where(b["r"] >= b["t"], 1.0, -1.0), np.where(high, 1.0, -1.0))
    g = ((1 + rng.integers(0, 256, size=(rows, cols)) / 256.0) * sgn).astype(F32)
    group = np.repeat(r_idx, cols)

    ts1 = b["ts"].astype(F64)

    def terms(gv):
        return (ts1 * gv,)
    g = boost(g, terms, group, rows, lwc_classes(rows, cols), lwc_n(cols))
    return dict(w=w, g=g, sig_lo=sig_lo, sig_hi=sig_hi, kinds=kinds, ext=ext, group=group, fwd=f)


# ---- mq_attention_probs_train(_backward) ----------------------------------------------------------------------------------------------------
AttnFwdGeom = namedtuple("AttnFwdGeom", "vpt grid trips n_l")
AttnBwdGeom = namedtuple("AttnBwdGeom", "vpt tpr grid rpw iters n_l n_grid dead")
AttnCase = namedtuple("AttnCase", "name rows cols mask mask_rows sqrt_d s1 coarse")
SQRT_D = (8.0, float(F32(math.sqrt(128.0))), float(F32(math.sqrt(80.0))))
ATTN_KEYS = (4, 252, 256, 260, 512, 516, 1024, 1028, 2048, 2052, 4096)
ATTN_MASKS = ("none", "full", "wrap", "causal", "nanrow")


def attn_fwd_geom(rows, cols):
    vpt = 1 if cols <= 256 else 2 if cols <= 512 else 4 if cols <= 1024 else 8 if cols <= 2048 else 16
    grid = min(cdiv(rows, 4), 8192)
    return AttnFwdGeom(vpt, grid, cdiv(rows, grid * 4), 4 * vpt + 6)


def attn_bwd_geom(rows, cols):
    """(VPT, TPR): a wave per row up to 512 keys, the workgroup per row beyond; at most 2048 workgroups.  n_l: adds on the longest path of
    a row sum (l, dot); n_grid: of a grid gradient (every trip's 4 VPT terms per thread, 6 + 2, one atomic per workgroup); dead: workgroups
    without a row on the last trip."""
    if cols <= 512:
        vpt, tpr, rpw = (1 if cols <= 256 else 2), 64, 4
        grid = min(cdiv(rows, 4), 2048)
    else:
        vpt, tpr, rpw = (1 if cols <= 1024 else 2 if cols <= 2048 else 4), 256, 1
        grid = min(rows, 2048)
    iters = cdiv(rows, grid * rpw)
    return AttnBwdGeom(vpt, tpr, grid, rpw, iters, 4 * vpt + 6 + (2 if tpr == 256 else 0), iters * 4 * vpt + 8 + grid,
                       grid - cdiv(rows - (iters - 1) * grid * rpw, rpw))


def attn_fast(s1, s2, sqrt_d):
    """The FAST body: both scales within [2^-60, 2^60] and sqrt_d a power of two (a zero mantissa field)."""
    ok = all(2.0 ** -60 <= abs(float(F32(s))) <= 2.0 ** 60 for s in (s1, s2))
    return ok and (int(np.asarray(sqrt_d, F32).view(np.uint32)) & 0x007FFFFF) == 0


def attn_bwd_classes(rows, cols):
    """trip of the row loop, wave (the row's wave when a wave owns a row, the vector's otherwise), slice k of the row."""
    ge = attn_bwd_geom(rows, cols)
    row = np.repeat(np.arange(rows, dtype=np.int64), cols)
    j = np.tile(np.arange(cols) // 4, rows)
    wave = row % 4 if ge.tpr == 64 else (j % 256) // 64
    return {"trip": row // (ge.grid * ge.rpw), "wave": wave, "k": j // ge.tpr}


def attn_fwd_classes(rows, cols):
    ge = attn_fwd_geom(rows, cols)
    row = np.repeat(np.arange(rows, dtype=np.int64), cols)
    j = np.tile(np.arange(cols) // 4, rows)
    return {"trip": row // (ge.grid * 4), "wave": row % 4, "k": j // 64}


def _attn_cases():
    cs = []
    for i, keys in enumerate(ATTN_KEYS):
        for j, sd in enumerate(SQRT_D):
            mk = ATTN_MASKS[(i + 2 * j) % 5]
            rows, mr = (30, 10) if mk == "wrap" else (27, 0 if mk == "none" else 27)    # 27 = 6 * 4 + 3, 30 = 7 * 4 + 2: a partial last group of four
            cs.append(AttnCase("keys%d_sd%d_%s" % (keys, j, mk), rows, keys, mk, mr, sd, None, keys < 64))
    cs.append(AttnCase("fwd_trips", 32768 + 6, 4, "none", 0, SQRT_D[1], None, True))
    cs.append(AttnCase("bwd_wave_trips", 2 * 8192 + 5, 8, "wrap", 9, SQRT_D[0], None, True))
    cs.append(AttnCase("bwd_wg_trips", 2 * 2048 + 3, 516, "none", 0, SQRT_D[2], None, False))
    cs.append(AttnCase("s1_2p61", 9, 64, "none", 0, SQRT_D[0], 2.0 ** 61, False))
    return tuple(cs)


ATTN_CASES = _attn_cases()
ATTN_GRID1 = (float(F32(256.0 / 65535)), 32768.0, 0.0, 65535.0)           # 16-bit, |raw| beyond 128 clamps on either side
ATTN_GRID2 = (float(F32(0.5 / 65535)), 0.0, 0.0, 65535.0)                 # 16-bit, p above 1/2 clamps
ATTN_GRID2_COARSE = (float(F32(0.5 / 255)), 0.0, 0.0, 255.0)              # few keys: large probabilities would sit on 16-bit ties too often


def attn_grids(case):
    g1 = ATTN_GRID1 if case.s1 is None else (case.s1, 32768.0, 0.0, 65535.0)
    if case.s1 is not None:           # every probability is fl(1 / 64): a step that puts t2 at 1000.7, clear of ties, r2 - t2 well above t2's error
        return g1, (float(F32(1.0 / 64 / 1000.7)), 0.0, 0.0, 65535.0)
    return g1, (ATTN_GRID2_COARSE if case.coarse else ATTN_GRID2)


def attn_peak_cols(rows, cols):
    """Columns for the peaks of the peaked rows, in turn: vectors chosen so that the peaks reach every slice k and every wave of the
    backward kernel's row layout, partly filled ones included (a greedy cover of the two marginals), highest column first; the vector's first element."""
    ge, nvec = attn_bwd_geom(rows, cols), cols // 4
    j = np.arange(nvec)
    k, w = j // ge.tpr, ((j % 256) // 64 if ge.tpr == 256 else np.zeros(nvec, np.int64))
    todo_k, todo_w, picks = set(k.tolist()), set(w.tolist()), []
    while todo_k or todo_w:
        gain = np.array([(int(a) in todo_k) + (int(b) in todo_w) for a, b in zip(k, w)])
        best = np.flatnonzero(gain == gain.max())
        jj = int(best[len(best) // 2])
        picks.append(4 * jj)
        todo_k.discard(int(k[jj]))
        todo_w.discard(int(w[jj]))
    return sorted(picks, reverse=True)


def _attn_raw(case, seed):
    """Ordinary rows: N(0, 60) -- Q1 clamps beyond +-128 on both sides -- with one key at 200 walking through attn_peak_cols, so that Q1
    clamps in every slice and wave.  Every third row is PEAKED: N(-80, 15) and one key at 300, far enough above the rest that its
    probability passes 1/2 and Q2 clamps; the peaks walk through attn_peak_cols from the last row back (under the causal mask the last
    rows are the ones that see the last vector).  No mask hides a vector that holds a pick."""
    rng = _rng("attn", case.name, seed)
    rows, cols = case.rows, case.cols
    raw = (rng.standard_normal((rows, cols)) * 60).astype(F32)
    peaked = np.arange(rows) % 3 == 1
    raw[peaked] = (rng.standard_normal((int(peaked.sum()), cols)) * 15 - 80).astype(F32)
    picks = attn_peak_cols(rows, cols)
    g0 = ((1 + rng.integers(0, 256, size=(rows, cols))) / 128.0).astype(F32)         # (0, 2]
    mask = None
    if case.mask != "none":
        mr = case.mask_rows
        mask = (rng.integers(-64, 65, size=(mr, cols)) / 32.0).astype(F32)
        if case.mask == "causal":
            lim = cols - mr + 1 + np.arange(mr)                           # the last mr of cols positions: row r sees the first lim[r] keys
            mask = np.where(np.arange(cols)[None, :] < np.maximum(lim, 1)[:, None], F32(0), F32(-np.inf)).astype(F32)
        elif case.mask == "nanrow":
            mask[2] = -np.inf
        else:
            hide = rng.random((mr, cols)) < 0.05
            for c in picks:
                hide[:, c:c + 4] = False
            mask[hide] = -np.inf

    def seen(r, c):
        return mask is None or np.isfinite(mask[r % mask.shape[0], c]) or case.mask == "nanrow"
    for rws, val in ((np.flatnonzero(peaked)[::-1], 300.0), (np.flatnonzero(~peaked)[::-1], 200.0)):
        i = 0
        for n, r in enumerate(rws):                                       # the next pick this row's mask lets it see
            for _ in range(len(picks)):
                c = picks[i % len(picks)] + ((n // len(picks)) % 4 if val == 200.0 else 0)
                i += 1
                if seen(r, c):
                    raw[r, c] = val
                    break
    return raw, g0, mask, peaked


def attn_design_gy(g0, f):
    """The designed gradient.  A row in which Q2 clamps: + on the clamped elements (d s2 and d o2 terms of one sign), - elsewhere; any
    other row: +4 on the elements Q1 clamps at the top (they are the row's maxima), (0, 2] elsewhere.  Either way the gradient that reaches
    the Q1-clamped maxima, p (gp - dot), is positive in every row, and with it the terms that dominate d s1 and d o1."""
    c2 = ~f["in2"] & np.isfinite(f["p"])
    row_c2 = c2.any(axis=1, keepdims=True)
    high1 = ~f["in1"] & (f["t1"] > 0)
    return np.where(row_c2, np.where(c2, g0 + 1, -g0), np.where(high1, F32(4), g0)).astype(F32)


@functools.lru_cache(maxsize=2)
def attn_inputs(case):
    """raw, gy, mask, grids, the two oracles' results (forward with the forward kernel's summation length, backward with the backward
    kernel's).  Re-seeded until no undecided element straddles the Q2 clamp edge in either.  The rows of a short last trip of the
    backward's row loop carry a gradient 2^k times larger (a row's terms are linear in its gradient), so that losing that trip shows."""
    g1, g2 = attn_grids(case)
    fg, bg = attn_fwd_geom(case.rows, case.cols), attn_bwd_geom(case.rows, case.cols)
    for seed in range(8):
        raw, g0, mask, peaked = _attn_raw(case, seed)
        f = O.train_attn_probs(raw, mask, g1, g2, case.sqrt_d, fg.n_l)
        gy = attn_design_gy(g0, f)
        b = O.train_attn_probs_backward(raw, gy, mask, g1, g2, case.sqrt_d, bg.n_l)
        if f["edge"].any() or b["fwd"]["edge"].any():
            continue
        if bg.iters > 1:
            trip = np.arange(case.rows) // (bg.grid * bg.rpw)
            last = trip == bg.iters - 1
            k = 0
            for t, e in zip(b["terms"], b["errs"]):
                bar = gamma(bg.n_grid) * np.abs(t).sum() + e.sum()
                have = abs(t[last].sum())
                if bar > 0 and have > 0:
                    k = max(k, int(np.ceil(np.log2(_TARGET * bar / have))) + 1)
            if k > 0:
                gy = (gy * np.where(last, F32(2.0 ** min(k, 16)), F32(1))[:, None]).astype(F32)
                b = O.train_attn_probs_backward(raw, gy, mask, g1, g2, case.sqrt_d, bg.n_l)
        return dict(raw=raw, gy=gy, mask=mask, grid1=g1, grid2=g2, fwd=f, bwd=b, seed=seed, peaked=peaked)
    raise AssertionError("no seed of %s keeps the Q2 clamp decided" % case.name)


def attn_bwd_sums(case, d=None):
    """The four grid gradients: float64 value and bar = gamma_n_grid * sum|term| + the propagated envelope."""
    d = attn_inputs(case) if d is None else d
    bg = attn_bwd_geom(case.rows, case.cols)
    b = d["bwd"]
    vals, bars = [], []
    for t, e in zip(b["terms"], b["errs"]):
        vals.append(t.sum())
        bars.append(gamma(bg.n_grid) * np.nansum(np.abs(t)) + np.nansum(e))
    return np.array(vals), np.array(bars)
