"""Inputs, case lists and launch-geometry predicates of the calibration / min-max pin (csrc/mq_reduce.hip), built once for the CPU checks
(test_calib_oracle.py) and the GPU comparison (test_gpu_calib.py): both files take every tensor, position list and case from here, so what
runs on the GPU is what the CPU file has checked.

The geometry predicates (tensor_geom, rows_vec_ok, cols_geom, probs_geom, causal_geom, norm_geom, gated_geom, rope_geom) restate the host
launch code of mq_reduce.hip; test_calib_oracle.py holds every case list to the branches it has to reach, so a list that stops reaching
one fails without a GPU.

Min/max inputs are PLANTED: every ordinary element lies in [-1, 1] (k / 1024: exact in fp16) and the unique extremes sit where a kernel
that drops a head scalar, a tail vector, a lane, a row chunk or a grid-stride trip would lose them."""
import functools
import zlib
from collections import namedtuple

import numpy as np

from oracle import mq_oracle as O

F32, F16 = np.float32, np.float16
NP = {"f32": F32, "f16": F16}
VEC = {"f32": 4, "f16": 8}                   # Ld16<T>::N: elements of a 16-byte load
SIZE = {"f32": 4, "f16": 2}
PINF, NINF = F32(np.inf), F32(-np.inf)


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def base_values(n, dtype, *key):
    """n ordinary values k / 1024, |k| <= 1000: strictly inside (-1, 1), exact in fp16 and fp32."""
    return (_rng("base", n, dtype, *key).integers(-1000, 1001, size=n) / 1024.0).astype(NP[dtype])


# ---- per-tensor: launch_tensor / launch_tensor_fresh ------------------------------------------------------------------------------------
TensorGeom = namedtuple("TensorGeom", "head nvec tail g stride")


def tensor_geom(numel, off, dtype):
    """off: elements past a 16-byte boundary.  head scalars up to the next boundary, nvec 16-byte vectors, tail scalars; g workgroups of
    256 lanes ((nvec + 1023) / 1024 clamped to [1, 512]), stride = g * 256 vectors per grid-stride trip."""
    n, sz = VEC[dtype], SIZE[dtype]
    a = off * sz
    head = min((16 - a % 16) // sz if a % 16 else 0, numel)
    nvec = (numel - head) // n
    g = min(max((nvec + 1023) // 1024, 1), 512)
    return TensorGeom(head, nvec, numel - head - nvec * n, g, g * 256)


def tensor_trips(geom):
    """(full 4-way iterations of lane 0, single trips of lane 0 behind them): stream_minmax's two loops."""
    i = four = 0
    while i + 3 * geom.stride < geom.nvec:
        i, four = i + 4 * geom.stride, four + 1
    one = 0
    while i < geom.nvec:
        i, one = i + geom.stride, one + 1
    return four, one


def tensor_sizes(dtype):
    """1 .. 4 * 1024 + 9 (g = 1 throughout), one 1 < g < 512, and one g = 512 that wraps: two full 4-way iterations, then two or three single
    trips (the vectors past 10 strides belong to the first 1000 lanes only), three tail scalars."""
    n = VEC[dtype]
    return (1, 3, 4, 5, 63, 64, 65, 1023, 1024 * 4 - 1, 1024 * 4 + 9, 3 * 1024 * 8 + 5, (10 * 512 * 256 + 1000) * n + 3)


def tensor_offsets(dtype):
    return tuple(range(16 // SIZE[dtype]))


def tensor_positions(numel, off, dtype):
    """dict position -> class for the planted extremes: every head scalar, the first and last element of the first and last vector, every
    tail scalar, the element on either side of the k * stride vector boundary for k = 1, 2, 3."""
    ge, n = tensor_geom(numel, off, dtype), VEC[dtype]
    pos = {}
    for i in range(ge.head):
        pos[i] = "head"
    if ge.nvec:
        for i, c in ((ge.head, "vec0_first"), (ge.head + n - 1, "vec0_last"), (ge.head + (ge.nvec - 1) * n, "vecN_first"),
                     (ge.head + ge.nvec * n - 1, "vecN_last")):
            pos.setdefault(i, c)
    for i in range(ge.head + ge.nvec * n, numel):
        pos[i] = "tail"
    for k in (1, 2, 3):
        if k * ge.stride < ge.nvec:
            pos.setdefault(ge.head + k * ge.stride * n - 1, "stride%d_before" % k)
            pos.setdefault(ge.head + k * ge.stride * n, "stride%d_at" % k)
    return dict(sorted(pos.items()))


def tensor_plants(numel, off, dtype):
    """[(position of the maximum +2, position of the minimum -2)]: every position holds each extreme once."""
    p = list(tensor_positions(numel, off, dtype))
    return [(p[i], p[(i + 1) % len(p)]) for i in range(len(p))]


# ---- per-row: mq_minmax_rows ------------------------------------------------------------------------------------------------------
RowsCase = namedtuple("RowsCase", "id dtype rows cols off")


def rows_vec_ok(cols, off, dtype):
    return off * SIZE[dtype] % 16 == 0 and cols % VEC[dtype] == 0


def _rows_cases():
    out = []
    for dt in ("f32", "f16"):
        n = VEC[dt]
        for rows, cols, off in ((1, 1, 0), (5, 7, 0), (4, 64 * n, 0), (7, 64 * n + n, 0), (9, 4100, 0), (6, 8 * 64 * n + 3, 0), (4, 64 * n, 1)):
            out.append(RowsCase("rows_%s_%dx%d%s" % (dt, rows, cols, "_off%d" % off if off else ""), dt, rows, cols, off))
    return out


ROWS_CASES = _rows_cases()


def rows_launches(c):
    """Per launch a list over the rows of (column of the row's maximum, column of its minimum).  The (launch, row) pairs are numbered
    t = launch * rows + r; pair t plants in unit t (a 16-byte vector on the vector path, a column on the scalar one) at element t % N of it,
    the minimum half a row further; the last launch plants row 0's extremes in the last column and at the head of the last vector (scalar path: the column before)."""
    n = VEC[c.dtype]
    vec = rows_vec_ok(c.cols, c.off, c.dtype)
    step = n if vec else 1
    units = c.cols // step
    launches = -(-min(64, units) // c.rows) + 1
    out = []
    for j in range(launches):
        row = []
        for r in range(c.rows):
            t = j * c.rows + r
            mx = ((t % units) * step + (t % step)) % c.cols
            row.append((mx, (((t + units // 2) % units) * step + ((t + 1) % step)) % c.cols))
        out.append(row)
    out[-1][0] = (c.cols - 1, (units - 1) * step if vec else max(c.cols - 2, 0))
    return out


def rows_lane(col, c):
    """The lane of minmax_rows_kernel that reads column col."""
    return (col // VEC[c.dtype]) % 64 if rows_vec_ok(c.cols, c.off, c.dtype) else col % 64


def rows_input(c, launch):
    x = base_values(c.rows * c.cols, c.dtype, c.id, launch).reshape(c.rows, c.cols)
    for r, (mx, mn) in enumerate(rows_launches(c)[launch]):
        if c.cols > 1:
            x[r, mn] = -2 - r / 8
        x[r, mx] = 2 + r / 8
    return x


# ---- per-column: launch_cols ------------------------------------------------------------------------------------------------------
ColsCase = namedtuple("ColsCase", "id dtype rows cols off")
ColsGeom = namedtuple("ColsGeom", "vec ctiles chunks rpb")


def cols_geom(rows, cols, off, dtype):
    n = VEC[dtype]
    vec = off * SIZE[dtype] % 16 == 0 and cols % n == 0
    ctiles = -(-cols // (64 * n)) if vec else -(-cols // 256)
    chunks = -(-2048 // ctiles)
    rpb = max(-(-rows // chunks), 64)
    return ColsGeom(vec, ctiles, -(-rows // rpb), rpb)


def _cols_cases():
    out = []
    for dt in ("f32", "f16"):
        n = VEC[dt]
        shapes = [(c, 0) for c in (n, 64 * n, 64 * n + n, 5 * 64 * n, 1, 7, 255, 257, 1001)] + [(64 * n, 1)]
        for cols, off in shapes:
            for rows in (1, 3, 63, 64, 65, 4 * 64 + 1):
                out.append(ColsCase("cols_%s_%dx%d%s" % (dt, rows, cols, "_off%d" % off if off else ""), dt, rows, cols, off))
    return out


COLS_CASES = _cols_cases()


def cols_plants(c, launch):
    """(rows of the columns' maxima [cols], rows of their minima [cols]) for launch 0 | 1: slot 4 c + 2 launch + kind lands in row slot % rows, so
    with 4 cols >= rows every row holds some column's extreme over the two launches."""
    col = np.arange(c.cols)
    return (4 * col + 2 * launch) % c.rows, (4 * col + 2 * launch + 1) % c.rows


def cols_input(c, launch):
    x = base_values(c.rows * c.cols, c.dtype, c.id, launch).reshape(c.rows, c.cols)
    col = np.arange(c.cols)
    mx, mn = cols_plants(c, launch)
    v = 2 + (col % 8) / 8
    if c.rows > 1:
        x[mn, col] = -v
    x[mx, col] = v
    return x


# ---- non-finite values and zeros ------------------------------------------------------------------------------------------------------
def later_updates(dtype, n):
    """Tensors that follow a NaN on the running paths: finite, +inf, -inf, +-huge -- the statistic stays NaN."""
    big = 1e30 if dtype == "f32" else 6e4
    return [np.full(n, v, NP[dtype]) for v in (0.5, np.inf, -np.inf, big, -big)]


def zeros_input(n, dtype):
    x = np.zeros(n, NP[dtype])
    x[::2] = -0.0
    return x


# ---- score chain: mq_calib_attention_probs(_causal) ---------------------------------------------------------------------------------------
SQRT_D = 8.0                                  # head_dim 64: inv = 0.125 exactly
INV_SQRT_D = F32(1.0) / F32(SQRT_D)


def probs_vpt(cols):
    return 1 if cols <= 256 else 2 if cols <= 512 else 4 if cols <= 1024 else 8 if cols <= 2048 else 16


def probs_geom(rows, cols):
    """(VPT, workgroups, rows per trip, trips) of the explicit-mask / no-mask launch: a wave per row, the grid capped at 2048 workgroups."""
    grid = min(-(-rows // 4), 2048)
    return probs_vpt(cols), grid, grid * 4, -(-rows // (grid * 4))


def causal_geom(rows, seq):
    """(VPT, workgroups, blocks per trip, [blocks of each trip]) of the causal launch: whole [seq, seq] blocks per trip, 8192 / seq of them
    (at least one, at most all)."""
    blocks = rows // seq
    per_trip = min(max(8192 // seq, 1), blocks)
    trips = [min(per_trip, blocks - b) for b in range(0, blocks, per_trip)]
    return probs_vpt(seq), per_trip * seq // 4, per_trip, trips


ProbsCase = namedtuple("ProbsCase", "id rows cols mask_rows")          # mask_rows 0: no mask
PROBS_CASES = [ProbsCase("probs_%d_%s" % (k, "mask" if m else "nomask"), 6, k, m) for k in (4, 256, 260, 512, 516, 1024, 1028, 2048, 2052, 4096)
               for m in (3, 0)] + [ProbsCase("probs_multitrip_70x130x260_mask", 70 * 130, 260, 130)]


def _scores(rows, cols, *key):
    """Raw scores ~ N(0, 16^2) -- x = raw / 8 ~ N(0, 2^2): probabilities well above the denormals -- clipped to +-60."""
    return np.clip(_rng("scores", rows, cols, *key).standard_normal((rows, cols), dtype=F32) * F32(16), -60, 60).astype(F32)


def _mask(mask_rows, cols, *key):
    """Additive mask: finite N(0, 2^2) with a tenth of the entries -inf; column 0 stays finite (no row without a live entry)."""
    g = _rng("mask", mask_rows, cols, *key)
    m = (g.standard_normal((mask_rows, cols), dtype=F32) * F32(2)).astype(F32)
    m[g.random((mask_rows, cols)) < 0.1] = NINF
    m[:, 0] = 0
    return m


def plant_rows(rows, per_trip_rows, seq=None):
    """Rows that take the planted extremes in turn: in the first trip, the last row of the first block of trip 1 (causal: the row the kernel
    visits FIRST on that trip -- odd trips run bottom-up; otherwise the last row of trip 1) and the very last row (the partial trip)."""
    first = 2 if rows > 2 else rows - 1
    if rows <= per_trip_rows:
        return [first, rows - 1]
    odd = per_trip_rows + seq - 1 if seq else min(2 * per_trip_rows, rows) - 1
    return list(dict.fromkeys([first, odd, rows - 1]))


@functools.lru_cache(maxsize=4)
def probs_input(c, variant=0):
    """(raw [rows, cols], mask | None).  variant v plants the unique raw maximum +80 (x = 10: the row's probability there is the tensor's
    largest) at column 0 of plant row v and the unique raw minimum -80 at its column 1."""
    raw = _scores(c.rows, c.cols, c.id)
    mask = _mask(c.mask_rows, c.cols, c.id) if c.mask_rows else None
    if mask is not None:
        mask[:, 1] = 0
    r = plant_rows(c.rows, probs_geom(c.rows, c.cols)[2])[variant]
    raw[r, 0], raw[r, 1] = 80, -80
    raw.setflags(write=False)
    return raw, mask


def probs_variants(c):
    return range(len(plant_rows(c.rows, probs_geom(c.rows, c.cols)[2])))


CausalCase = namedtuple("CausalCase", "id seq blocks")
CAUSAL_CASES = [CausalCase("causal_S%d_x%d" % (s, b), s, b) for s, b in
                ((4, 3), (64, 3), (100, 2), (256, 2), (260, 1), (64, 260), (100, 200), (260, 70), (1028, 16), (2052, 7))]


@functools.lru_cache(maxsize=2)
def causal_base(c):
    raw = _scores(c.seq * c.blocks, c.seq, c.id)
    raw.setflags(write=False)
    return raw


def causal_plants(c):
    """[(row, {(row, col): value})]: the raw extremes at the live columns 0 and 1 of each plant row (every plant row has row % seq >= 2)."""
    rows = c.seq * c.blocks
    return [(r, {(r, 0): F32(80), (r, 1): F32(-80)}) for r in plant_rows(rows, causal_geom(rows, c.seq)[2] * c.seq, c.seq)]


# odd rows: the score value, where it sits relative to the diagonal of row r (live: col <= r % seq), and whether the row turns NaN
ODD_ROWS = (("ninf_live", -np.inf, "live", False), ("ninf_masked", -np.inf, "masked", False), ("pinf_masked", np.inf, "masked", True),
            ("pinf_live", np.inf, "live", True), ("nan_live", np.nan, "live", True), ("nan_masked", np.nan, "masked", True),
            ("all_ninf_live", -np.inf, "all_live", True))
ODD_SEQ = (260, 516)                          # VPT 2 (klive 1 | 2) and VPT 4: odd rows below and above the first 256-column block


def odd_input(seq):
    """raw [3 seq, seq] with one odd row per ODD_ROWS entry in each of the three blocks, at rows whose diagonal lies in different 256-column
    blocks; the other rows are ordinary.  Returns (raw, [(row, name, nan_expected)])."""
    raw = _scores(3 * seq, seq, "odd").copy()
    marks = []
    picks = sorted({5, 40, 130, 250, 255, 256, 257, seq // 2 + 1, seq - 3, seq - 2, seq - 1})
    k = 0
    for blk in range(3):
        for name, val, where, nan in ODD_ROWS:
            d = picks[k % len(picks)]
            k += 1
            r = blk * seq + d
            if where == "live":
                raw[r, d // 2] = val
            elif where == "masked":
                if d + 1 >= seq:                                      # the last row masks nothing
                    d = seq - 6
                    r = blk * seq + d
                raw[r, min(d + 1 + (k % 7), seq - 1)] = val
            else:
                raw[r, :d + 1] = val
            marks.append((r, name, nan))
    assert len({m[0] for m in marks}) == len(marks), sorted(m[0] for m in marks)
    return raw, marks


def odd_mask(seq):
    """The causal mask of a [seq, seq] block as an additive tensor (0 on and below the diagonal, -inf above)."""
    return np.where(np.arange(seq)[None, :] > np.arange(seq)[:, None], NINF, F32(0)).astype(F32)


ALLONES_COLS = 260
ALLONES_PLACES = ((0, 1), (3, 259), (255, 256), (258, 257))


def allones_input():
    """(raw [16, 260], mask [16, 260], [(row, k, col of the 0, col of -k 2^-23 sqrt_d)]): every row's only unmasked entries are 0 and
    -k 2^-20 (x = -k 2^-23 exactly, sqrt_d = 8).  expf(-2^-23) correctly rounded is 1 - 2^-23 and l = 2 - 2^-23 = 0x3fffffff."""
    rows = 4 * len(ALLONES_PLACES)
    raw = _scores(rows, ALLONES_COLS, "allones").copy()
    mask = np.full((rows, ALLONES_COLS), NINF, F32)
    info = []
    for i, (c0, c1) in enumerate(ALLONES_PLACES):
        for k in range(1, 5):
            r = 4 * i + k - 1
            raw[r, c0], raw[r, c1] = 0, -k * 2.0 ** -20
            mask[r, c0] = mask[r, c1] = 0
            info.append((r, k, c0, c1))
    return raw, mask, info


def allones_table(jmax=24):
    """For ex = 1 - j 2^-24 (j = 0 .. jmax: every fp32 a device expf could return for these arguments), l = fl(1 + ex) and the IEEE
    quotients (RN(1 / l), RN(ex / l)) as bit patterns: {(p_max bits, p_other bits): [(j, l bits)]}.  A pair names its l except where l has
    an all-ones significand: there an expf one ulp low (odd j: 1 + ex ties to the even neighbour) gives the same pair (test_calib_oracle.py)."""
    out = {}
    for j in range(jmax + 1):
        ex = F32(1.0 - j * 2.0 ** -24)
        l = F32(F32(1) + ex)
        key = (int((F32(1) / l).view(np.uint32)), int((ex / l).view(np.uint32)))
        out.setdefault(key, []).append((j, int(l.view(np.uint32))))
    return out


# ---- mq_calib_norm --------------------------------------------------------------------------------------------------------------------
def norm_geom(rows, cols):
    return (1 if cols <= 1024 else 2 if cols <= 2048 else 4 if cols <= 4096 else 8), min(rows, 8192)


NormCase = namedtuple("NormCase", "id rows cols ln delta slots bias")
NORM_EPS = 1e-5


def _norm_cases():
    out = []
    for i, cols in enumerate((4, 1000, 1024, 1028, 2048, 2052, 4096, 4100, 8192)):
        for ln, bias in ((0, 0), (1, 0), (1, 1)):
            for delta, slots in ((0, 0), (1, 0), (1, 1)):
                out.append(NormCase("norm_%s%s_%d%s" % ("ln" if ln else "rms", "_bias" if bias else "", cols, ("_delta_slots" if slots else "_delta") if delta else ""),
                                    3 + i % 3, cols, ln, delta, slots, bias))
    for ln in (0, 1):
        for v in range(3):
            out.append(NormCase("norm_%s_wrap_v%d" % ("ln" if ln else "rms", v), 8192 + 37, 12, ln, 1, 1, ln))
    return out


NORM_CASES = _norm_cases()
NORM_WRAP_ROWS = (0, 8191, 8192 + 36)


@functools.lru_cache(maxsize=8)
def norm_input(c):
    """(x, delta | None, weight, bias | None).  LayerNorm rows have mean ~ 1.5 (the candidate list of the fp32 mean stays short).  The wrap
    shape plants delta = h = +50 at column 0 of one of NORM_WRAP_ROWS and -50 at column 1 of the next (x = 0 there): the extremes of delta
    and h, and -- a row that one entry dominates normalises to +-sqrt(cols) there -- of y; variant v rotates the rows."""
    g = _rng("norm", c.id)
    x = (g.standard_normal((c.rows, c.cols), dtype=F32) + F32(1.0 if c.ln else 0.0)).astype(F32)
    d = (g.standard_normal((c.rows, c.cols), dtype=F32) * F32(0.5) + F32(0.5 if c.ln else 0.0)).astype(F32) if c.delta else None
    w = (0.5 + g.random(c.cols)).astype(F32)
    b = (g.standard_normal(c.cols) * 0.1).astype(F32) if c.bias else None
    if c.rows > 8192:
        v = int(c.id[-1])
        hi, lo = NORM_WRAP_ROWS[v % 3], NORM_WRAP_ROWS[(v + 1) % 3]
        w[0] = w[1] = 1.5
        x[hi, 0] = x[lo, 1] = 0
        d[hi, 0], d[lo, 1] = 50, -50
    return x, d, w, b


# ---- mq_calib_gated -------------------------------------------------------------------------------------------------------------------
GATED_WRAP = 4096 * 256 * 4                    # elements of one trip of the capped grid
GATED_SIZES = (4, 1028, 4 * 256 * 3 + 4, GATED_WRAP + 4 * 777)
GATED_ARGMIN = {0: -1.2784645, 1: -0.7517916}  # where SiLU / GELU are lowest


def gated_geom(numel):
    grid = min(-(-(numel // 4) // 256), 4096)
    return grid, -(-(numel // 4) // (grid * 256))


def gated_quads(numel):
    """Quads that take the planted extremes in turn: the first, the last one of the first trip (wrapping sizes) and the last."""
    nq = numel // 4
    return sorted({0, min(GATED_WRAP // 4, nq) - 1, nq - 1})


@functools.lru_cache(maxsize=4)
def gated_base(numel):
    """a, b ~ N(0, 2^2) clipped to +-8; the wrapping size tiles a block of 65536 values (the float64 erf runs over its distinct values)."""
    g = _rng("gated", numel)
    n = min(numel, 65536)
    a = np.clip(g.standard_normal(n, dtype=F32) * F32(2), -8, 8).astype(F32)
    b = np.clip(g.standard_normal(n, dtype=F32) * F32(2), -8, 8).astype(F32)
    reps = -(-numel // n)
    a, b = np.tile(a, reps)[:numel].copy(), np.tile(b, reps)[:numel].copy()
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def gated_plant(act, quad):
    """{index: (a, b)} for one quad: a's extremes +-9, b's +-9, the product's act(9) * 8.5 and 8.5 * -9, act(a)'s 9 and its global minimum."""
    q = 4 * quad
    return {q: (9.0, 8.5), q + 1: (8.5, -9.0), q + 2: (-9.0, 2.0), q + 3: (GATED_ARGMIN[act], 9.0)}


# ---- mq_calib_rope / mq_calib_rope_qkv --------------------------------------------------------------------------------------------------
RopeCase = namedtuple("RopeCase", "id B S H KV D rot qkv")
RopeGeom = namedtuple("RopeGeom", "dq hstep dq_shift grid trips")


def rope_geom(c):
    dq = c.D // 4
    shift = dq.bit_length() - 1 if dq & (dq - 1) == 0 else -1
    grid = min(c.B * c.S, 8192)
    return RopeGeom(dq, 256 // dq, shift, grid, -(-c.B * c.S // grid))


def _rope_cases():
    two = [(2, 37, 32, 4, 64, 64), (1, 50, 8, 1, 256, 256), (1, 29, 32, 32, 64, 16), (2, 21, 6, 2, 80, 32)]
    three = [(2, 37, 32, 4, 64, 64), (1, 29, 8, 8, 64, 16), (1, 19, 6, 2, 80, 32)]
    new = [(3, 2800, 2, 1, 8, 8), (1, 2, 2, 1, 1024, 1024), (2, 5, 6, 3, 12, 8)]
    return [RopeCase("rope%s_B%dS%dH%dKV%dD%drot%d" % ((("_qkv" if qkv else ""),) + g), *g, qkv)
            for qkv, gs in ((0, two + new), (1, three + new)) for g in gs]


ROPE_CASES = _rope_cases()


@functools.lru_cache(maxsize=4)
def rope_input(c):
    """(q_lin [B, S, H D], k_lin, v_lin [B, S, KV D], cos, sin [S, rot]).  The last (b, s) row of the first trip of the grid holds the
    maximum +50 of each input, the last row of the last trip its minimum -50 (one trip: the same row)."""
    g = _rng("rope", c.id)
    q, k, v = (g.standard_normal((c.B, c.S, n * c.D), dtype=F32) for n in (c.H, c.KV, c.KV))
    inv = 1.0 / (10000.0 ** (np.arange(0, c.rot, 2, dtype=np.float64) / c.rot))
    ang = np.outer(np.arange(c.S, dtype=np.float64), inv)
    ang = np.concatenate((ang, ang), -1)
    cos, sin = np.cos(ang).astype(F32), np.sin(ang).astype(F32)
    ends = rope_plant_rows(c)
    for t in (q, k, v):
        flat = t.reshape(c.B * c.S, -1)
        flat[ends[0], 3 % flat.shape[1]] = 50
        flat[ends[-1], flat.shape[1] - 1] = -50
    return q, k, v, cos, sin


def rope_plant_rows(c):
    ge = rope_geom(c)
    return sorted({min((t + 1) * ge.grid, c.B * c.S) - 1 for t in range(ge.trips)})
