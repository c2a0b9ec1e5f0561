"""Inputs, grids and case list of the mq_qmatmul pin, built once for the CPU checks (test_qmatmul_oracle.py) and the GPU comparison
(test_gpu_qmatmul.py): both files take every tensor, grid and case from here, so what runs on the GPU is what the CPU file has checked.

The dispatch predicates restate the host code of csrc/mq_qmatmul.hip: choose() its choice of kernel and launch dimensions (checked
against the library's own mq_qmatmul_geometry, case by case and over a sweep of shapes), epilogue_route() make_epi's choice of the
epilogue body.  test_qmatmul_oracle.py holds the list to the 28 instantiations and the (kernel family, epilogue cause) pairs it has to
reach, so a list that stops reaching one fails without a GPU.

Operand content is a random body (fewer than 5 % of the elements clamp) plus quantize_cases._pool: centres and exact half steps of both
parities with their +-1 / +-2 ulp neighbours, both clamps and the steps around them, +-0 and denormals, then NaN, +-inf and (where the
scale lets the quotient overflow) +-FLT_MAX.  Ties and non-finite values are also planted in the last real k, the last row and the last
column.  The M N >= 2^29 fall-back from buffer stores (a 2-GB output) is not part of the list."""
import functools
import zlib
from collections import namedtuple

import numpy as np

import quantize_cases as QC
from oracle import mq_oracle as O

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max

# ---- grids: name -> (scale, offset, qmin, qmax).  No operand scale is a power of two. ------------------------------------------------
GRIDS = {
    "u4": (0.21, 7.0, 0, 15),
    "u6": (0.057, 30.0, 0, 63),
    "u8": (0.031, 121.0, 0, 255),
    "u8b": (0.0123, 128.0, 0, 255),          # offset 128: ca = cb = 0, the bracket bound is K 255 255 (fits 32 bits up to K = 33025)
    "i8": (0.0173, 3.0, -128, 127),
    "u12": (0.0021, 2040.0, 0, 4095),
    "i12": (0.0017, -0.0, -2048, 2047),
    "u16": (0.00021, 32771.0, 0, 65535),
    "i16": (0.00033, -0.0, -32768, 32767),
    # the special grids of the epilogue's slow route
    "u8+off": (0.031, 100003.0, 0, 255),     # zero points near +-1e5: the bracket leaves 32 bits at K = 1
    "u8-off": (0.031, -99991.0, 0, 255),
    "u8edge": (0.031, 1048575.0, 0, 255),    # |zero point| = 2^20 - 1: the last one served
    "u8insane": (0.031, 1048576.0, 0, 255),  # 2^20: every output NaN
    "u8lo30": (32767.5, 121.0, 0, 255),      # s^2 just below 2^30
    "u8hi30": (32768.5, 121.0, 0, 255),      # s^2 just above 2^30
    "u8huge": (1.0e18, 121.0, 0, 255),       # alpha = 1e36: t alpha overflows from |t| ~ 340 up
    # output ties: alpha = 15 2^-15 exact, the output scale is 2 alpha -- every odd bracket is an exact tie of the output quantizer
    "t6a": (3 * 2.0 ** -7, 31.0, 0, 63),
    "t6b": (5 * 2.0 ** -8, 30.0, 0, 63),
}
# output grids given outright; "auto8" / "auto16" / "auto16s" are derived from the oracle's own unquantized product (0.5 % beyond either clamp)
OUT_GRIDS = {
    "tie16": (15 * 2.0 ** -14, 32768.0, 0, 65535),
    "fixed16": (0.0137, 30011.0, 0, 65535),
    "coarse8": (1.1e18, 128.0, 0, 255),                      # the largest scales of the reciprocal form: finite products of alpha = 1e36 clamp
    "so-70": (2.0 ** -70, 0.0, -2.0 ** 100, 2.0 ** 100),      # IEEE divide; levels wide enough that nothing saturates
    "so+70": (2.0 ** 70, 128.0, 0, 255),                     # every quotient is below 2^-9: all outputs sit on index 128 (value 0)
    "oo61": (0.0137, 1.5 * 2.0 ** 61, 0, 2.0 ** 62),         # r + o = o: all outputs 0 (idx = o)
}
AUTO = {"auto8": (8, False), "auto16": (16, False), "auto16s": (16, True)}

QCase = namedtuple("QCase", "id batch M N K kcontig g1 g2 gout a_off b_off o_off content degenerate",
                   defaults=("auto16", 0, 0, 0, "random", None))
# a_off / b_off / o_off: bytes the base is moved past a 64-byte boundary.  content: "random" | "centres" (exact grid points: integer
# brackets of both parities for the output ties) | "limit" (saturated rows / columns at K = 131071).  degenerate: why the output grid of a
# case saturates by construction (the case is then outside the no-saturation conditions).
CASES = [
    # ---- row-panel kernel: x1 <= 8 bits, K <= 256, M > 64, N > 64 -------------------------------------------------------------------
    QCase("panel-kT-kc1-vec", 2, 129, 132, 64, True, "u8", "u8"),                    # two row panels: rotated tile order
    QCase("panel-kT-kc2-vec-ranges", 1, 130, 260, 128, True, "u8", "i8"),            # N >= 260: two column ranges per row panel
    QCase("panel-kT-kc4-vec-nblk8", 4, 200, 128, 256, True, "u6", "u8", "auto8"),    # nblk % 8 == 0: the XCD order
    QCase("panel-kT-kc1-x1off", 1, 129, 132, 36, True, "u8", "u8", "auto16", 4),
    QCase("panel-kT-kc2-oddN", 2, 65, 67, 100, True, "i8", "u8", "auto16s"),
    QCase("panel-kT-kc4-oddK", 1, 130, 100, 250, True, "u4", "u8", "auto8"),
    QCase("panel-kT-kc1-x2off", 1, 70, 68, 64, True, "u8", "u6", None, 0, 4),
    QCase("panel-kn-kc1-vec", 2, 130, 132, 64, False, "u8", "u8"),
    QCase("panel-kn-kc2-vec", 1, 129, 68, 100, False, "u8", "i8", None),
    QCase("panel-kn-kc4-vec-nblk16", 8, 70, 260, 256, False, "i8", "u8", "auto8"),
    QCase("panel-kn-kc1-x1off", 1, 129, 132, 36, False, "u8", "u8", "auto16", 4),
    QCase("panel-kn-kc2-outoff", 1, 130, 68, 128, False, "u8", "u4", "auto16", 0, 0, 4),
    QCase("panel-kn-kc4-oddK", 2, 66, 72, 250, False, "u6", "u8", "auto8"),
    # ---- tile kernel, 64 rows per workgroup -------------------------------------------------------------------------------------
    QCase("tile-kT-M1", 2, 1, 512, 64, True, "u8", "u8"),
    QCase("tile-kT-nothing-divides", 3, 5, 7, 13, True, "u8", "i8", None),
    QCase("tile-kn-K4", 3, 16, 8, 4, False, "u8", "u8", None),
    QCase("tile-kn-K9", 2, 40, 12, 9, False, "i8", "u8", "auto8"),
    QCase("tile-kT-K260", 1, 130, 130, 260, True, "u8", "u8"),                       # K > 256 keeps an 8-bit x1 off the panel kernel
    QCase("tile-kT-a16", 2, 64, 100, 256, True, "u16", "u8", "auto8"),
    QCase("tile-kT-a16-oddK", 1, 77, 50, 203, True, "i12", "u6", "auto8"),
    QCase("tile-kn-a16-rot", 1, 130, 128, 200, False, "u16", "u8", "auto8"),         # 4 chunks, the partial one mid-loop under rotation
    QCase("tile-kn-a16-K9", 8, 1, 64, 9, False, "i16", "u8", "auto8"),
    QCase("tile-kn-a12-x1off", 1, 50, 64, 200, False, "u12", "i8", None, 4),
    # ---- tile kernel, 128 rows per workgroup: M >= 256 and batch ceil(M / 128) ceil(N / 64) >= 512 ------------------------------------
    QCase("rf2-kT-vec", 171, 257, 64, 8, True, "u8", "u8"),                          # the last 128-row tile holds one real row
    QCase("rf2-kT-oddK", 171, 257, 64, 9, True, "i8", "u8", "auto8"),
    QCase("rf2-kn-vec", 171, 257, 64, 12, False, "u8", "i8", None),
    QCase("rf2-kn-oddK", 171, 257, 64, 10, False, "u6", "u8", "auto8"),
    QCase("rf2-kT-a16-vec", 86, 257, 128, 16, True, "u16", "u8", "auto8"),
    QCase("rf2-kT-a16-oddK", 86, 257, 128, 18, True, "i16", "u8", "auto16s"),
    QCase("rf2-kn-a16-vec", 86, 320, 128, 20, False, "u12", "u8", None),             # 320: the last tile holds exactly 64 real rows
    QCase("rf2-kn-a16-x1off", 86, 257, 128, 8, False, "u16", "i8", "auto8", 4),
    # ---- the epilogue's slow route, cause by cause, on the panel kernel and on the tile kernel ---------------------------------------
    QCase("panel-fits32-offsets", 1, 129, 68, 36, True, "u8+off", "u8-off"),
    QCase("tile-fits32-offsets", 2, 33, 20, 70, True, "u8-off", "u8+off"),
    QCase("panel-fits32-offsets-plain", 1, 66, 68, 36, False, "u8+off", "u8-off", None),
    QCase("panel-sane-edge", 1, 129, 68, 36, True, "u8edge", "u8"),
    QCase("tile-sane-edge", 2, 33, 20, 70, True, "u8", "u8edge", None),
    QCase("panel-insane", 1, 129, 68, 36, True, "u8insane", "u8", "fixed16", degenerate="every output is NaN"),
    QCase("tile-insane", 2, 33, 20, 70, True, "u8", "u8insane", None, degenerate="every output is NaN"),
    QCase("panel-so-small", 1, 129, 68, 36, True, "u8", "u8", "so-70"),
    QCase("tile-so-small", 2, 33, 20, 70, True, "u8", "u8", "so-70"),
    QCase("panel-so-big", 1, 129, 68, 36, True, "u8", "u8", "so+70", degenerate="every quotient rounds to 0"),
    QCase("tile-so-big", 2, 33, 20, 70, True, "u8", "u8", "so+70", degenerate="every quotient rounds to 0"),
    QCase("panel-alpha-below", 1, 129, 68, 36, True, "u8lo30", "u8lo30"),            # the fast route, at its bound
    QCase("tile-alpha-below", 2, 33, 20, 70, True, "u8lo30", "u8lo30"),
    QCase("panel-alpha-above", 1, 129, 68, 36, True, "u8hi30", "u8hi30"),
    QCase("tile-alpha-above", 2, 33, 20, 70, True, "u8hi30", "u8hi30", None),
    QCase("panel-oo-big", 1, 129, 68, 36, True, "u8", "u8", "oo61", degenerate="r + offset is the offset"),
    QCase("tile-oo-big", 2, 33, 20, 70, True, "u8", "u8", "oo61", degenerate="r + offset is the offset"),
    QCase("panel-overflow", 1, 129, 68, 36, True, "u8huge", "u8huge", "coarse8", degenerate="most products overflow to inf: NaN out, the rest on a clamp"),
    QCase("tile-overflow", 2, 33, 20, 70, True, "u8huge", "u8huge", "coarse8", degenerate="most products overflow to inf: NaN out, the rest on a clamp"),
    QCase("tile-overflow-plain", 2, 33, 20, 70, True, "u8huge", "u8huge", None),     # no quantizer: +-inf is stored
    QCase("tile-K33025-fits", 1, 20, 16, 33025, True, "u8b", "u8b", "auto8"),                   # K 255 255 < 2^31: the last K on the fast route
    QCase("tile-K33026", 1, 20, 16, 33026, True, "u8b", "u8b", "auto8"),
    # ---- output ties ----------------------------------------------------------------------------------------------------------------
    QCase("panel-out-ties", 1, 130, 132, 64, True, "t6a", "t6b", "tie16", content="centres"),
    QCase("tile-out-ties", 2, 50, 70, 40, True, "t6a", "t6b", "tie16", content="centres"),
    # ---- the limit: K = 131071, a' = b' = -128 in whole rows and columns (the accumulators reach 2^31 - 2^14), and the mixed-sign twin
    QCase("limit-8bit", 1, 3, 4, 131071, True, "u8", "u8", content="limit"),
    QCase("limit-16bit", 1, 3, 4, 131071, False, "u16", "u8", "auto8", content="limit"),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)

ALL_KERNELS = sorted(["panel<bkm=%d,kc=%d,vec=%d>" % (b, k, v) for b in (0, 1) for k in (1, 2, 4) for v in (0, 1)] +
                     ["tile<a16=%d,bkm=%d,rf=%d,vec=%d>" % (a, b, r, v) for a in (0, 1) for b in (0, 1) for r in (1, 2) for v in (0, 1)])
# (kernel family, epilogue cause) pairs the list has to reach; a 16-bit x1 and K > 256 exist on the tile kernel only
CAUSES = ("plain1", "plain2", "zero-points", "insane", "scale-small", "scale-big", "alpha", "offset-out")
REQUIRED_ROUTES = sorted([(f, c) for f in ("panel", "tile") for c in CAUSES] + [("tile", "a16"), ("tile", "large-K")])


# ---- dispatch predicates --------------------------------------------------------------------------------------------------------
def choose(batch, M, N, K, kcontig, al1, al2, alo, span1):
    """mq_qmatmul's choice of kernel and launch dimensions (choose_kernel in csrc/mq_qmatmul.hip), restated."""
    a16 = span1 > 255
    rf = 2 if (M >= 256 and batch * ((M + 127) // 128) * ((N + 63) // 64) >= 512) else 1
    tiles_m, tiles_n = (M + 64 * rf - 1) // (64 * rf), (N + 63) // 64
    a_vec = K % 4 == 0 and al1
    b_vec = (K % 4 == 0 and al2) if kcontig else True
    o_vec = N % 4 == 0 and alo
    vec = a_vec and b_vec
    panel, kc, nsplit, per = False, 0, 1, tiles_n
    if not a16 and K <= 256 and M > 64 and N > 64:
        panel, rf = True, 2
        kc = 1 if K <= 64 else (2 if K <= 128 else 4)
        tiles_m = (M + 127) // 128
        base = batch * tiles_m
        nsplit = min(tiles_n, max(1, (2048 + base - 1) // base))
        per = max((tiles_n + nsplit - 1) // nsplit, min(4, tiles_n))
        nsplit = (tiles_n + per - 1) // per
        vec = vec and o_vec and M * N < 2 ** 29
    nblk = batch * tiles_m * (nsplit if panel else tiles_n)
    return dict(panel=int(panel), a16=int(a16), bkm=int(bool(kcontig)), rf=rf, kc=kc, vec=int(vec), a_vec=int(a_vec), b_vec=int(b_vec),
                o_vec=int(o_vec), tiles_m=tiles_m, tiles_n=tiles_n, nsplit=nsplit, tiles_per_split=per, nblk=nblk)


def kernel_name(g):
    if g["panel"]:
        return "panel<bkm=%d,kc=%d,vec=%d>" % (g["bkm"], g["kc"], g["vec"])
    return "tile<a16=%d,bkm=%d,rf=%d,vec=%d>" % (g["a16"], g["bkm"], g["rf"], g["vec"])


def grids_of(c):
    """(g1, g2, g_out | None) as (scale, offset, qmin, qmax) tuples of python floats (fp32 values for scale and offset)."""
    def f(g):
        return (float(F32(g[0])), float(F32(g[1])), float(g[2]), float(g[3]))
    g1, g2 = f(GRIDS[c.g1]), f(GRIDS[c.g2])
    if c.gout is None:
        return g1, g2, None
    if c.gout in OUT_GRIDS:
        return g1, g2, f(OUT_GRIDS[c.gout])
    return g1, g2, _auto_grid(c.id)


def kernel_of(c):
    """The geometry dict of a case, its instantiation under "name"."""
    g1 = GRIDS[c.g1]
    g = choose(c.batch, c.M, c.N, c.K, c.kcontig, c.a_off % 16 == 0, c.b_off % 16 == 0, c.o_off % 16 == 0, g1[3] - g1[2])
    g["name"] = kernel_name(g)
    return g


def epilogue_route(c):
    """(PLAIN, causes): the epilogue body make_epi picks -- 1 / 2 = ordinary grids without / with an output quantizer, 0 = every special
    case -- and the set of reasons for 0 (restated from csrc/mq_qmatmul.hip)."""
    g1, g2, go = grids_of(c)
    a16 = g1[3] - g1[2] > 255
    z1, z2 = np.rint(F32(g1[1])), np.rint(F32(g2[1]))
    sane = abs(z1) < 2.0 ** 20 and abs(z2) < 2.0 ** 20
    a_shift = int(g1[2]) + (32896 if a16 else 128)
    b_shift = int(g2[2]) + 128
    ca, cb = a_shift - int(z1), b_shift - int(z2)
    alpha = float(F32(F32(g1[0]) * F32(g2[0])))
    causes = set()
    if a16:
        causes.add("a16")
    elif not float(c.K) * (255.0 + abs(ca)) * (255.0 + abs(cb)) < 2147483648.0:
        if not sane:
            pass
        elif max(abs(ca), abs(cb)) > 1000:
            causes.add("zero-points")
        else:
            causes.add("large-K")
    if not sane:
        causes.add("insane")
    if abs(alpha) > 2.0 ** 30:
        causes.add("alpha")
    if go is not None:
        so, oo, qmin, qmax = go
        if not 2.0 ** -60 <= abs(so) <= 2.0 ** 60:
            causes.add("scale-small" if abs(so) < 1 else "scale-big")
        if abs(oo) > 2.0 ** 60:
            causes.add("offset-out")
        if not (qmin <= qmax and abs(qmin) <= 2.0 ** 60 and abs(qmax) <= 2.0 ** 60):
            causes.add("levels")
    if causes:
        return 0, causes
    return (1, {"plain1"}) if go is None else (2, {"plain2"})


def route_pairs(c):
    """The (kernel family, cause) pairs a case stands for: a case with one cause only ("levels" rides along with so-70's wide levels)."""
    plain, causes = epilogue_route(c)
    fam = "panel" if kernel_of(c)["panel"] else "tile"
    causes = causes - {"levels"}
    return {(fam, next(iter(causes)))} if len(causes) == 1 else set()


# ---- operands -------------------------------------------------------------------------------------------------------------------
def _body(n_rows, cols, grid, rng, nonfinite=True):
    """[n_rows, cols] fp32 for one grid: a Gaussian body inside the grid (sigma = half range / 2.6: under 1 % beyond a clamp), then at most
    an eighth of the elements replaced by quantize_cases._pool and the non-finite values."""
    s, o, qmin, qmax = grid
    lo, hi = (qmin - o) * s, (qmax - o) * s
    x = ((lo + hi) / 2 + rng.standard_normal(n_rows * cols) * ((hi - lo) / 2 / 2.6)).astype(F32)
    pool = QC._pool(s, o, int(qmin), int(qmax), F32, rng)
    if nonfinite:
        pool = np.concatenate([pool, np.repeat(QC._nonfinite_values(s, F32), 3)])
    rng.shuffle(pool)
    n = min(len(pool), x.size // 8)
    x[rng.permutation(x.size)[:n]] = pool[:n]
    return x.reshape(n_rows, cols)


def _specials(grid):
    """Half-step ties of both parities, NaN, +-inf (and +-FLT_MAX where the quotient overflows) for planting."""
    s, o, qmin, qmax = grid
    mid = int((qmin + qmax) // 2)
    ties = [F32((k + 0.5 - o) * s) for k in (mid, mid + 1, int(qmin), int(qmax) - 1)]
    return ties + list(QC._nonfinite_values(s, F32))


def _plant(x, grid):
    """x [batch, rows, K]: specials into the last k, the last row and row 0 of every batch element."""
    sp = _specials(grid)
    B, R, K = x.shape
    spots = [(R - 1, K - 1), (0, K - 1), (R - 1, 0), (R // 2, K - 1), (R - 1, K // 2), (0, 0), (R // 2, K // 2)]
    spots = spots[:R * K // 64]                                  # a tiny operand takes fewer: the 5 % bound on clamped elements holds
    for b in range(B):
        for i, (r, k) in enumerate(spots):
            x[b, r, k] = sp[(i + b) % len(sp)]


@functools.lru_cache(maxsize=None)
def operands(cid):
    """(x1 [batch, M, K], x2m: x2 AS IT LIES IN MEMORY -- [batch, N, K] for a K-contiguous x2, [batch, K, N] otherwise), read-only."""
    c = BY_ID[cid]
    g1, g2, _ = (grids_of(c._replace(gout=None)))
    rng = np.random.default_rng(zlib.crc32(repr((c.id, c.batch, c.M, c.N, c.K)).encode()))
    B, M, N, K = c.batch, c.M, c.N, c.K
    if c.content == "random":
        x1 = _body(B * M, K, g1, rng).reshape(B, M, K)
        x2 = _body(B * N, K, g2, rng).reshape(B, N, K)
        _plant(x1, g1)
        _plant(x2, g2)
    elif c.content == "centres":
        def centres(rows, g):
            k = rng.integers(int(g[2]), int(g[3]) + 1, (B, rows, K))
            return ((k - g[1]) * g[0]).astype(F32)
        x1, x2 = centres(M, g1), centres(N, g2)
    else:
        assert c.content == "limit"
        x1 = _body(B * M, K, g1, rng, nonfinite=False).reshape(B, M, K)
        x2 = _body(B * N, K, g2, rng, nonfinite=False).reshape(B, N, K)
        big = F32(1e25)
        x1[:, 0, :] = -big                 # index qmin: the stored byte (both planes of a 16-bit x1) is -128
        x1[:, M - 1, :] = big              # index qmax: +127
        x2[:, 0, :] = -big
        x2[:, 1, :] = big
    x2m = x2 if c.kcontig else np.ascontiguousarray(np.swapaxes(x2, 1, 2))
    for a in (x1, x2m):
        a.setflags(write=False)
    return x1, x2m


def logical_x2(c):
    x2m = operands(c.id)[1]
    return np.swapaxes(x2m, 1, 2) if c.kcontig else x2m


@functools.lru_cache(maxsize=None)
def _auto_grid(cid):
    """An ordinary calibrated output grid from the oracle's own unquantized product: 0.5 % of the finite values beyond either clamp."""
    c = BY_ID[cid]
    bits, sym = AUTO[c.gout]
    v = expect(cid, None, False)["v"]
    v = v[np.isfinite(v)].astype(np.float64)
    lo, hi = np.percentile(v, 0.5), np.percentile(v, 99.5)
    qmin, qmax = O.qrange(bits, sym)
    if sym:
        s, o = max(abs(lo), abs(hi)) / qmax, 0.0
    else:
        s = (hi - lo) / (qmax - qmin)
        o = float(np.rint(-lo / s))
    s = F32(s)
    if (s.view(np.uint32) & 0x007FFFFF) == 0:
        s = F32(s * F32(1.03))
    return (float(s), float(F32(o)), float(qmin), float(qmax))


@functools.lru_cache(maxsize=None)
def expect(cid, mutation=None, with_out=True):
    """oracle.qmatmul_launch on a case (with_out False: without its output grid, for the grid's own derivation)."""
    c = BY_ID[cid]
    x1, _ = operands(cid)
    g1, g2, go = grids_of(c) if with_out else grids_of(c._replace(gout=None))
    return O.qmatmul_launch(x1, logical_x2(c), g1, g2, go, mutation)


def stored_operands(c, e):
    """(a', b'): the bytes the kernel parks in the LDS (index - shift; a 16-bit x1 as 256 hi' + lo'), from the oracle's indices."""
    g1, g2, _ = grids_of(c._replace(gout=None))
    a16 = g1[3] - g1[2] > 255
    return e["ia"] - (int(g1[2]) + (32896 if a16 else 128)), e["ib"] - (int(g2[2]) + 128)


def clamped(x, grid):
    """Elements of an operand whose index leaves the grid: rint(x / s) + o outside [qmin, qmax], or NaN."""
    s, o, qmin, qmax = grid
    with np.errstate(all="ignore"):
        t = (np.asarray(x, F32) / F32(s)).astype(F32)
        q = (((np.rint(t) - t).astype(F32) + t).astype(F32) + F32(o)).astype(F32)
    return ~((q >= qmin) & (q <= qmax))
