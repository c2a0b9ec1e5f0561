"""Inputs and case lists of the quantize-to-integer pin, built once for the CPU checks (test_quantize_oracle.py) and the GPU comparison
(test_gpu_quantize.py): both files take every tensor, grid and case from here, so what runs on the GPU is what the CPU file has checked.

The dispatch predicates (quantize_branch, tiled_branch, fake_quant_branch) restate launch_quantize, mq_quantize_tiled and
launch_fake_quant of csrc/mq_quantize.hip / csrc/mq_fake_quant.hip: test_quantize_oracle.py holds every case list to the branches it
has to reach, so a list that stops reaching one fails without a GPU."""
import functools
import zlib
from collections import namedtuple

import numpy as np

from oracle import mq_oracle as O

F32 = np.float32
F16 = np.float16
FLT_MAX = np.finfo(np.float32).max

# ---- grids ----------------------------------------------------------------------------------------------------------------------
# name -> (scale, offset, qmin, qmax).  No scale is a power of two; all lie inside the reciprocal form's range (mq_common.h).
# "clamp" is the lower clamp of set_scale_offset_from_minmax (qmodule.py:58); "sym" is small enough (<= 2^-8) for +-FLT_MAX.
GRIDS = {
    "u8": (0.031, 121.0, 0, 255),
    "h8": (0.0390625, 121.0, 0, 255),        # 5 * 2^-7: (k + 1/2 - o) s is exact in fp16 for |k - o| <= 200, so fp16 inputs hold exact ties
    "clamp": (1e-5, 97.0, 0, 255),
    "coarse": (3.7, 130.0, 0, 255),
    "sym": (0.0031, -0.0, -127, 127),
    "w4": (0.21, 7.0, 0, 15),
    "hsym": (0.0029296875, -0.0, -127, 127),  # 3 * 2^-10 and 7 * 2^-5: the symmetric and the 4-bit grid for fp16 inputs
    "hw4": (0.21875, 7.0, 0, 15),
    "u16": (0.00021, 32771.0, 0, 65535),
    "i16": (0.00033, -0.0, -32768, 32767),
}
F16_GRID = {"u8": "h8", "sym": "hsym", "w4": "hw4"}
ROW_VARIANTS = 4            # per-row grids: row r takes variant r % 4 of its base grid
SPECIAL_COLS = (0, 3, 4, 15, 16, 255, 256, -1)


def grid_rows(name, rows, per_row):
    """(scale fp32 [n], offset fp32 [n], qmin, qmax), n = rows for a per-row grid (variant r % 4: the scale grows by a quarter a step -- still
    no power of two, and few enough bits for fp16 ties on "h8" --, an asymmetric offset moves by one), else 1."""
    s, o, qmin, qmax = GRIDS[name]
    if not per_row:
        return np.array([s], F32), np.array([o], F32), qmin, qmax
    v = np.arange(rows) % ROW_VARIANTS
    sym = qmin < 0
    return (F32(s) * (F32(1) + F32(0.25) * v.astype(F32))).astype(F32), (F32(o) + (0 if sym else 1) * v.astype(F32)).astype(F32), qmin, qmax


def _ulp_neighbours(v):
    """v and its neighbours at +-1 and +-2 ulp of its own format (integer steps on the bit pattern; +-0 are left alone)."""
    it = np.int32 if v.dtype == np.float32 else np.int16
    b = v.view(it).astype(np.int64)
    out = []
    for d in (0, 1, -1, 2, -2):
        out.append((b + d).astype(it).view(v.dtype))
    out = np.concatenate(out)
    return out[np.isfinite(out)]


def _pool(s, o, qmin, qmax, dtype, rng):
    """Every index within 2 of either clamp and ~60 interior ones: the centre (k - o) s and the half step (k + 1/2 - o) s -- round-half-
    even ties of both parities -- each with its neighbours at +-1 / +-2 ulp; +-0 and a few denormals."""
    edge = np.concatenate([np.arange(qmin - 2, qmin + 3), np.arange(qmax - 2, qmax + 3)])
    inner = rng.choice(np.arange(qmin + 3, qmax - 2), size=min(60, qmax - qmin - 5), replace=False)
    inner[: len(inner) // 2 * 2: 2] |= 1                      # both parities for certain
    k = np.concatenate([edge, inner]).astype(np.float64)
    s64, o64 = float(F32(s)), float(F32(o))
    pts = np.concatenate([(k - o64) * s64, (k + 0.5 - o64) * s64]).astype(dtype)
    tiny = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45], F32) if dtype == np.float32 else np.array([0.0, -0.0, 6e-8, -6e-8, 3e-6], F16)
    return np.concatenate([_ulp_neighbours(pts), tiny.astype(dtype)])


def _nonfinite_values(s, dtype):
    vals = [np.nan, np.inf, -np.inf]
    if dtype == np.float32 and float(F32(s)) <= 2.0 ** -8:     # both division forms overflow
        vals += [FLT_MAX, -FLT_MAX]
    return np.array(vals, dtype)


def _fill(n_rows, cols, s, o, qmin, qmax, dtype, nonfinite, rng):
    lo, hi = (qmin - float(o)) * float(s), (qmax - float(o)) * float(s)
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    x = (mid + rng.standard_normal(n_rows * cols) * (1.3 * half / 2.5)).astype(dtype)          # ~1 % beyond 1.3 x either clamp
    pool = _pool(s, o, qmin, qmax, dtype, rng)
    if nonfinite:
        pool = np.concatenate([pool, np.repeat(_nonfinite_values(s, dtype), 3)])
    rng.shuffle(pool)
    n = min(len(pool), x.size)
    x[rng.permutation(x.size)[:n]] = pool[:n]
    return x.reshape(n_rows, cols)


@functools.lru_cache(maxsize=None)
def make_input(rows, cols, grid, dtype="f32", per_row=False, nonfinite=False):
    """(x [rows, cols] read-only, scale [n], offset [n], qmin, qmax).  Every row is built for its own grid; the first and the last row
    hold half-step ties (or, in a non-finite case, NaN / +-inf / +-FLT_MAX) at columns 0, 3, 4, 15, 16, 255, 256 and the last."""
    dt = np.float32 if dtype == "f32" else np.float16
    sc, of, qmin, qmax = grid_rows(grid, rows, per_row)
    rng = np.random.default_rng(zlib.crc32(repr((rows, cols, grid, dtype, per_row, nonfinite)).encode()))
    x = np.empty((rows, cols), dt)
    nv = ROW_VARIANTS if per_row else 1
    for v in range(min(nv, rows)):
        sel = np.arange(v, rows, nv)
        x[sel] = _fill(len(sel), cols, sc[v % sc.size], of[v % of.size], qmin, qmax, dt, nonfinite, rng)
    for r in sorted({0, rows - 1}):
        s, o = float(sc[r % sc.size]), float(of[r % of.size])
        nf = _nonfinite_values(s, dt)
        for i, c in enumerate(SPECIAL_COLS):
            c = cols - 1 if c < 0 else c
            if c >= cols:
                continue
            k = min(max(qmin + 1 + 2 * i + (i & 1) + r % 2, qmin), qmax - 1)                    # ties of both parities
            x[r, c] = nf[(i + r) % len(nf)] if nonfinite else dt((k + 0.5 - o) * s)
    assert nonfinite or np.all(np.isfinite(x))
    for a in (x, sc, of):
        a.setflags(write=False)
    return x, sc, of, qmin, qmax


@functools.lru_cache(maxsize=None)
def chan_scale(cols):
    """[cols] in [0.25, 4], no power of two."""
    cs = np.exp2(np.random.default_rng(4242 + cols).uniform(-2, 2, cols)).astype(F32)
    pow2 = (cs.view(np.uint32) & 0x007FFFFF) == 0
    cs[pow2] = F32(1.37)
    cs = np.clip(cs, F32(0.2500001), F32(3.999))
    cs.setflags(write=False)
    return cs


@functools.lru_cache(maxsize=None)
def chan_input(rows, cols, grid, nonfinite=False):
    """make_input with every value multiplied by its channel's scale (one rounding), so that the quotient x / chan_scale the kernel forms
    lands on the centres, the ties and their neighbours again (wherever fl(fl(v c) / c) = v: most elements)."""
    x, sc, of, qmin, qmax = make_input(rows, cols, grid, "f32", False, nonfinite)
    with np.errstate(over="ignore"):
        xc = (x.astype(np.float64) * chan_scale(cols).astype(np.float64)[None, :]).astype(F32)
    xc.setflags(write=False)
    return xc, sc, of, qmin, qmax


def exact_ties(x, scale, chan=None):
    """The fp32 quotients the reference rounds that are exact half steps (x [rows, cols], scale [1 | rows])."""
    with np.errstate(all="ignore"):
        xf = np.asarray(x).astype(F32)
        if chan is not None:
            xf = (xf / chan[None, :]).astype(F32)
        t = (xf / np.asarray(scale, F32).reshape(-1, 1)).astype(F32).astype(np.float64)
    t = t[np.isfinite(t)]
    return t[t - np.floor(t) == 0.5]


# ---- mq_quantize ----------------------------------------------------------------------------------------------------------------
Q_BYTES = {"i8": 1, "u8": 1, "i16": 2, "u16": 2, "i32": 4}
Q_NUMPY = {"i8": np.int8, "u8": np.uint8, "i16": np.int16, "u16": np.uint16, "i32": np.int32}

QCase = namedtuple("QCase", "id rows cols dtype grid shift q_dtype per_row row_sum chan x_off q_off cs_off nonfinite",
                   defaults=(False, True, False, 0, 0, 0, False))
# x_off: elements, q_off / cs_off: bytes the pointer is moved off its 64-byte aligned buffer
QUANTIZE_CASES = [
    # b16 wave-per-row kernel: fp32, 1-byte storage, cols % 16 == 0, cols >= 256
    QCase("b16-256-u8", 5, 256, "f32", "u8", 128, "i8"),
    QCase("b16-256-sym-rows", 5, 256, "f32", "sym", 0, "i8", per_row=True, row_sum=False),
    QCase("b16-272-U8", 5, 272, "f32", "u8", 0, "u8"),
    QCase("b16-272-w4-rows", 5, 272, "f32", "w4", 0, "u8", per_row=True),
    QCase("b16-1040-clamp", 9, 1040, "f32", "clamp", 128, "i8", row_sum=False),
    QCase("b16-1040-coarse-rows", 9, 1040, "f32", "coarse", 128, "i8", per_row=True),
    QCase("b16-5632-u8", 2, 5632, "f32", "u8", 128, "i8"),
    QCase("b16-5632-sym-rows", 2, 5632, "f32", "sym", 0, "i8", per_row=True),
    QCase("b16-sweep2-u8", 16400, 256, "f32", "u8", 128, "i8"),
    QCase("b16-sweep2-u8-rows", 16400, 256, "f32", "u8", 128, "i8", per_row=True, row_sum=False),
    QCase("b16-onerow", 1, 512, "f32", "u8", 128, "i8"),
    # generic kernel, vector form
    QCase("vec-1000-u8", 4, 1000, "f32", "u8", 128, "i8"),
    QCase("vec-1000-sym-rows", 4, 1000, "f32", "sym", 0, "i8", per_row=True, row_sum=False),
    QCase("vec-1000-f16", 6, 1000, "f16", "h8", 128, "i8"),
    QCase("vec-1000-f16-U8-rows", 6, 1000, "f16", "h8", 0, "u8", per_row=True),
    QCase("vec-1000-f16-U16", 6, 1000, "f16", "u16", 0, "u16"),
    QCase("vec-512-U16", 5, 512, "f32", "u16", 0, "u16"),
    QCase("vec-512-I16-rows", 5, 512, "f32", "i16", 0, "i16", per_row=True),
    QCase("vec-512-I16-shift", 5, 512, "f32", "u16", 32768, "i16", row_sum=False),
    QCase("vec-512-I32", 5, 512, "f32", "u16", 0, "i32"),
    QCase("vec-512-I32-u8", 5, 512, "f32", "u8", 0, "i32", per_row=True),
    # generic kernel, scalar form
    QCase("scalar-1x1", 1, 1, "f32", "u8", 128, "i8"),
    QCase("scalar-3x5-rows", 3, 5, "f32", "u8", 128, "i8", per_row=True),
    QCase("scalar-255-sym", 7, 255, "f32", "sym", 0, "i8"),
    QCase("scalar-1027-w4-rows", 3, 1027, "f32", "w4", 0, "u8", per_row=True),
    QCase("scalar-1027-f16", 3, 1027, "f16", "h8", 128, "i8"),
    QCase("scalar-1027-U16", 3, 1027, "f32", "u16", 0, "u16", row_sum=False),
    QCase("scalar-x-off", 5, 256, "f32", "u8", 128, "i8", x_off=1),
    QCase("scalar-q-off", 5, 256, "f32", "u8", 128, "i8", q_off=1),
    QCase("scalar-1000-x-off-rows", 4, 1000, "f32", "sym", 0, "i8", per_row=True, x_off=1),
    QCase("scalar-512-U16-q-off", 5, 512, "f32", "u16", 0, "u16", q_off=2),
    QCase("scalar-1000-f16-x-off", 6, 1000, "f16", "h8", 128, "i8", x_off=1),
    # chan_scale
    QCase("cs-b16", 64, 256, "f32", "u8", 128, "i8", chan=True),
    QCase("cs-b16-sym", 64, 256, "f32", "sym", 0, "i8", chan=True, row_sum=False),
    QCase("cs-vec-100", 5, 100, "f32", "u8", 128, "i8", chan=True),
    QCase("cs-vec-100-w4", 5, 100, "f32", "w4", 0, "u8", chan=True),
    QCase("cs-scalar-101", 5, 101, "f32", "u8", 128, "i8", chan=True),
    QCase("cs-ptr-off", 8, 512, "f32", "u8", 128, "i8", chan=True, cs_off=4),
    # non-finite inputs, one shape per kernel
    QCase("nonfinite-b16", 5, 272, "f32", "clamp", 128, "i8", nonfinite=True),
    QCase("nonfinite-b16-sym-rows", 5, 272, "f32", "sym", 0, "i8", per_row=True, nonfinite=True),
    QCase("nonfinite-generic", 4, 1000, "f32", "clamp", 128, "i8", nonfinite=True),
    QCase("nonfinite-generic-f16", 3, 1027, "f16", "h8", 128, "i8", nonfinite=True),
]


def quantize_branch(c):
    """The kernel launch_quantize picks for a case (csrc/mq_quantize.hip) and the facts the suite wants covered."""
    f32 = c.dtype == "f32"
    esz = 4 if f32 else 2
    vn = 4 if f32 else 8
    qb = Q_BYTES[c.q_dtype]
    x_al = (c.x_off * esz) % 16 == 0
    vec_ok = x_al and c.q_off % (qb * vn) == 0 and c.cols % vn == 0
    b16 = f32 and qb == 1 and x_al and c.q_off % 16 == 0 and c.cols % 16 == 0 and c.cols >= 256
    if c.chan:
        assert f32 and not c.per_row
        kernel = "b16-cs" if (b16 and c.cs_off % 16 == 0) else ("generic-cs-vec" if vec_ok else "generic-cs-scalar")
    elif b16:
        kernel = "b16"
    else:
        kernel = "generic-vec" if vec_ok else "generic-scalar"
    per_row = c.per_row and c.rows > 1 and not c.chan
    return dict(kernel=kernel, per_row=per_row, dtype=c.dtype, q_dtype=c.q_dtype, row_sum=c.row_sum,
                sweep2=kernel.startswith("b16") and (c.rows + 3) // 4 > 256 * 16,
                forced_scalar=kernel.endswith("scalar") and c.cols % vn == 0, nonfinite=c.nonfinite)


def quantize_inputs(c):
    """(x, scale, offset, qmin, qmax, chan_scale | None) of a case."""
    if c.chan:
        return chan_input(c.rows, c.cols, c.grid, c.nonfinite) + (chan_scale(c.cols),)
    return make_input(c.rows, c.cols, c.grid, c.dtype, c.per_row, c.nonfinite) + (None,)


def quantize_expect(c):
    x, sc, of, qmin, qmax, cs = quantize_inputs(c)
    return O.quantize_storage(x, sc, of, qmin, qmax, c.shift, cs)


# ---- mq_quantize_tiled ----------------------------------------------------------------------------------------------------------
TILED_GRIDS = [("u8", 128), ("sym", 0), ("w4", 0)]
TCase = namedtuple("TCase", "id rows cols dtype chan knob_rows staged nonfinite", defaults=("f32", False, 0, 1, False))
TILED_CASES = [
    # lane-per-fragment kernel, generic k-block loop
    TCase("lane-1x128", 1, 128), TCase("lane-7x128", 7, 128), TCase("lane-16x640", 16, 640), TCase("lane-33x1152", 33, 1152),
    TCase("lane-40x5632", 40, 5632), TCase("lane-100x5120", 100, 5120),
    # lane-per-fragment kernel, everything in flight (16 / 32 k blocks), rows < 64
    TCase("flight-5x1024", 5, 1024), TCase("flight-63x1024", 63, 1024), TCase("flight-9x2048", 9, 2048), TCase("flight-63x2048", 63, 2048),
    TCase("flight-3x2048", 3, 2048),
    # staged kernel, rows per workgroup chosen by shape
    TCase("staged-64x1024", 64, 1024), TCase("staged-77x2048", 77, 2048), TCase("staged-70x3072", 70, 3072), TCase("staged-65x4096", 65, 4096),
    # staged kernel, rows forced; the staged kernel switched off
    TCase("staged-77x2048-rows4", 77, 2048, knob_rows=4), TCase("staged-77x2048-rows8", 77, 2048, knob_rows=8),
    TCase("staged-70x4096-rows4", 70, 4096, knob_rows=4), TCase("staged-70x4096-rows8", 70, 4096, knob_rows=8),
    TCase("unstaged-77x2048", 77, 2048, staged=0),
    # fp16, chan_scale
    TCase("f16-33x1152", 33, 1152, dtype="f16"), TCase("f16-70x2048", 70, 2048, dtype="f16"),
    TCase("cs-33x1152", 33, 1152, chan=True), TCase("cs-70x2048", 70, 2048, chan=True),
    # non-finite inputs: lane-per-fragment and staged
    TCase("nonfinite-lane", 33, 1152, nonfinite=True), TCase("nonfinite-staged", 77, 2048, nonfinite=True),
]


def tiled_branch(c):
    """The kernel mq_quantize_tiled picks (csrc/mq_quantize.hip) and the shape facts the issue names."""
    assert c.cols % 128 == 0 and c.rows > 0
    kblocks = c.cols >> 6
    kpairs = kblocks >> 1
    if c.chan:
        assert c.dtype == "f32"
        kernel = "lane-generic-cs"
    elif c.dtype == "f32" and 1024 <= c.cols <= 4096 and c.cols % 1024 == 0 and c.rows >= 64 and c.staged:
        four = c.knob_rows == 4 or (c.knob_rows == 0 and c.cols <= 2048)
        kernel = "staged-V%d-rows%d" % (c.cols // 1024, 4 if four else 8)
    elif c.dtype == "f32":
        kernel = "lane-steps2" if kblocks == 32 else ("lane-steps1" if kblocks == 16 else "lane-generic")
    else:
        kernel = "lane-generic-f16"
    generic = kernel.startswith("lane-generic")
    return dict(kernel=kernel, knob=c.knob_rows, staged_off=not c.staged, nonfinite=c.nonfinite,
                padding_workgroup=kernel.startswith("lane") and 1 <= c.rows % 16 <= 8,          # an 8-row workgroup wholly past `rows`
                idle_waves=generic and kpairs < 8, second_trip=generic and kpairs > 8, unequal_waves=generic and kpairs % 8 != 0,
                rows_lt_64=c.rows < 64)


def tiled_inputs(c, grid):
    if c.chan:
        return chan_input(c.rows, c.cols, grid, c.nonfinite) + (chan_scale(c.cols),)
    return make_input(c.rows, c.cols, F16_GRID[grid] if c.dtype == "f16" else grid, c.dtype, False, c.nonfinite) + (None,)


# ---- mq_fake_quant --------------------------------------------------------------------------------------------------------------
FCase = namedtuple("FCase", "id rows cols dtype grid per_row x_off alias", defaults=(False, 0, False))
FQ_GRID_CAP = 2048 * 256          # grid_for: 2048 workgroups of 256 threads, grid-stride beyond
FAKE_QUANT_CASES = [
    FCase("f32-tensor-vec", 6, 1000, "f32", "u8"),
    FCase("f32-tensor-scalar-numel", 3, 1027, "f32", "clamp"),
    FCase("f32-tensor-scalar-ptr", 6, 1000, "f32", "u8", x_off=1),
    FCase("f32-row-vec", 6, 1000, "f32", "sym", per_row=True),
    FCase("f32-row-scalar", 3, 1027, "f32", "u16", per_row=True),
    FCase("f16-tensor-vec", 6, 1000, "f16", "h8"),
    FCase("f16-tensor-scalar", 3, 1027, "f16", "hw4"),
    FCase("f16-row-vec", 6, 1000, "f16", "h8", per_row=True),
    FCase("f16-row-scalar", 3, 1027, "f16", "h8", per_row=True),
    FCase("f32-alias", 6, 1000, "f32", "u8", alias=True),
    FCase("f16-alias", 3, 1027, "f16", "h8", alias=True),
    FCase("f32-vec-second-trip", 1, 4 * FQ_GRID_CAP + 1024, "f32", "u8"),
    FCase("f32-scalar-second-trip", 1, FQ_GRID_CAP + 259, "f32", "i16"),
]


def fake_quant_branch(c):
    vn = 4 if c.dtype == "f32" else 8
    per_row = c.per_row and c.rows > 1
    numel = c.rows * c.cols
    vec = (c.x_off * (4 if c.dtype == "f32" else 2)) % 16 == 0 and ((c.cols if per_row else numel) % vn == 0)
    work = numel // vn if vec else numel
    return dict(kernel="%s-%s-%s" % (c.dtype, "row" if per_row else "tensor", "vec" if vec else "scalar"), alias=c.alias,
                second_trip=work > FQ_GRID_CAP, misaligned=c.x_off != 0)


def fake_quant_inputs(c):
    return make_input(c.rows, c.cols, c.grid, c.dtype, c.per_row, True)       # NaN is kept: every case carries the non-finite values


def fake_quant_expect(c):
    x, sc, of, qmin, qmax = fake_quant_inputs(c)
    with np.errstate(over="ignore", invalid="ignore"):
        if c.dtype == "f32":
            return O.fake_quant(x, sc.reshape(-1, 1), of.reshape(-1, 1), qmin, qmax)
        if c.per_row and c.rows > 1:
            return O.fake_quant_f16_per_row(x, sc, of, qmin, qmax)
        return O.fake_quant_f16_per_tensor(x, sc[0], of[0], qmin, qmax)[0]


# ---- mq_linear_epilogue_prepare ---------------------------------------------------------------------------------------------------
EPILOGUE_N = [1, 255, 256, 257, 5632]
# (a_offset, a_shift, w_shift, K): za = -7 / 255 / 121, both signs of the K za zw product far past 2^31
EPILOGUE_CONFIGS = [(121.0, 128, 128, (1 << 24) - 1), (255.0, 0, 0, (1 << 24) - 1), (121.0, 0, 128, 5632), (121.0, 128, 0, 4096)]


def epilogue_case(N, per_row, a_offset, a_shift, w_shift, K):
    """dict(a_scale, a_offset, a_shift, w_scale [1 | N], w_offset, w_shift, w_colsum int32 [N], K)."""
    rng = np.random.default_rng(991 * N + 7 * int(per_row) + a_shift + 3 * w_shift + K % 1000)
    n = N if per_row else 1
    w_scale = (F32(0.0123) * (1 + rng.uniform(0, 1, n))).astype(F32)
    w_offset = rng.integers(0, 256, n).astype(F32)                         # zw in [-128, 255] behind the shift
    lim = min(K * 128, 2 ** 31 - 1)
    colsum = rng.integers(-lim, lim, N, dtype=np.int64).astype(np.int32)
    colsum[0] = np.int32(lim)
    colsum[-1] = np.int32(-lim)
    return dict(a_scale=np.array([0.031], F32), a_offset=np.array([a_offset], F32), a_shift=a_shift, w_scale=w_scale, w_offset=w_offset,
                w_shift=w_shift, w_colsum=colsum, K=K)


def all_epilogue_cases():
    for N in EPILOGUE_N:
        for per_row in (False, True):
            for cfg in EPILOGUE_CONFIGS:
                yield (N, per_row) + cfg, epilogue_case(N, per_row, *cfg)


# ---- mq_pack_w4 -----------------------------------------------------------------------------------------------------------------
PACK_SHAPES = [(1, 64), (3, 128), (257, 192)]


def pack_input(N, K):
    return np.random.default_rng(31 * N + K).integers(0, 16, (N, K), dtype=np.uint8)
