"""Operands, grids and case lists of the prefill GEMM epilogue pin, built once for the CPU checks (test_gemm_oracle.py) and the GPU
comparison (test_gpu_gemm_epilogue.py): both files take every tensor, grid and case from here, so what runs on the GPU is what the CPU
file has checked.

The dispatch predicates (pick_variant, run_gemm_kernel, kernels_of) restate run_gemm, pick_variant,
linear_tiled_residual, mq_w8a8_linear_tiled_segmented, linear_tiled_gated and mq_w4a8_linear_tiled of csrc/mq_gemm.hip and name the
kernel that serves a case; test_gemm_oracle.py holds the case lists to the kernels and the grid classes they have to reach, so a list
that stops reaching one fails without a GPU.  tile_of_block restates the kernels' block -> tile map.

Operands are built from column and row classes, not uniform noise.  Columns, by n % 32 (COL_CLASS):
  tie (0..5)     few non-zero effective weights in -8..7, A' = alpha' an exact dyadic c / 2^k with c odd, B' an integer: on the low rows
                 q = t A' + B' is exact and a half-integer whenever t c = 2^(k-1) mod 2^k
  near (6..9)    the tie column n - 6 again (same weights, same A') with B' moved by -2, -1, +1, +2 ulp
  generic (10..19)  full-range weights, zero points in -255..255 (both extremes), non-dyadic alpha, random bias
  sat (20..25)   generic operands under an alpha four grid widths wide: both clamps hit; the zero row lands one step outside, on and
                 one step inside either clamp
  big (26..31)   col_term of +-(2^25 .. 2^30.8): |t| > 2^24, the int32 -> fp32 conversion rounds; alpha small, so the fma cancels
                 t A' against a bias of the same size and the result still lands inside the grid
Rows, by m % 16: 0..9 low magnitude (activations in -2..1), 10..15 the full int8 range (both extremes in every row); row 5 is all
zero, so its accumulators are col_term itself."""
import functools
import zlib
from collections import namedtuple

import numpy as np

from oracle import mq_oracle as O

F32 = np.float32

# ---- output grids ---------------------------------------------------------------------------------------------------------------
# name -> (qmin, qmax, storage, offset, scale, power-of-two scale).  None: no output quantizer.
Grid = namedtuple("Grid", "qmin qmax storage offset scale scale_p2")
GRIDS = {
    "u8": Grid(0, 255, "u8", 117.0, 0.0371, 2.0 ** -5),            # the cvt_pk_u8 fast path
    "i8u": Grid(0, 255, "i8", 117.0, 0.0371, 2.0 ** -5),           # i8 storage = index - 128 on the same path
    "s8": Grid(-128, 127, "i8", 0.0, 0.0371, 2.0 ** -5),
    "u4": Grid(0, 15, "u8", 7.0, 0.21, 2.0 ** -2),                 # the non-fast 8-bit path
    "u16": Grid(0, 65535, "u16", 32771.0, 0.00021, 2.0 ** -12),
    "i16": Grid(-32768, 32767, "i16", 5.0, 0.00021, 2.0 ** -12),
    "f32_8": Grid(0, 255, "f32", 117.0, 0.0371, 2.0 ** -5),
    "f16_8": Grid(0, 255, "f16", 117.0, 0.0371, 2.0 ** -5),
    "f32_16": Grid(0, 65535, "f32", 32771.0, 0.00021, 2.0 ** -12),
    "f16_16": Grid(0, 65535, "f16", 32771.0, 0.00021, 2.0 ** -12),
    "f32_i16": Grid(-32768, 32767, "f32", 5.0, 0.00021, 2.0 ** -12),
    "none32": None,
    "none16": None,
}
NONE_STORAGE = {"none32": "f32", "none16": "f16"}
U8_FAST = ("u8", "i8u")                                            # what the generated index kernels accept
GRID16_F32 = ("f32_16", "f32_i16")                                 # what the generated residual kernels accept


COL_PERIOD = 32
COL_CLASS = np.array(["tie"] * 6 + ["near"] * 4 + ["generic"] * 10 + ["sat"] * 6 + ["big"] * 6)
NEAR_ULPS = (-2, -1, 1, 2)
TIE_CK = ((1, 1), (1, 2), (3, 2), (3, 3), (5, 3), (1, 1))        # A' = c / 2^k of the six tie columns
BIG_CT = (2, -4, 9, -30, 70, -110)                                 # col_term of the six big columns, in units of 2^24 (+ an odd rest)
ZERO_ROW = 5
SAT_STEPS = ("lo-1", "lo", "lo+1", "hi-1", "hi", "hi+1")           # where the zero row lands in the six sat columns

# name, entry point, shape, packed 4-bit weights, output grid, column segment ends (None: one grid), bias / row sums present, forced
# variant (-1: by shape), hook = (setter, value) or None, power-of-two scales
Case = namedtuple("Case", "id entry M N K w4 grid segs bias rowsum variant hook p2")


def _case(entry, shape, grid="u8", w4=False, segs=None, bias=True, rowsum=True, variant=-1, hook=None, p2=False):
    M, N, K = shape
    w4 = w4 or entry == "tiled_w4"                                 # (mq_w4a8_linear_tiled has no int8 form)
    cid = "%s-%s%dx%dx%d-%s" % (entry, "w4-" if w4 else "", M, N, K, grid)
    if segs:
        cid += "-seg" + "_".join(str(s) for s in segs)
    if not bias:
        cid += "-nobias"
    if not rowsum:
        cid += "-nors"
    if variant >= 0:
        cid += "-v%d" % variant
    if hook:
        cid += "-%s%d" % (hook[0].replace("mq_gemm_set_", ""), hook[1])
    if p2:
        cid += "-p2"
    return Case(cid, entry, M, N, K, w4, grid, segs, bias, rowsum, variant, hook, p2)


# ---- dispatch, restated -----------------------------------------------------------------------------------------------------------
VARIANTS = ((256, 176), (256, 176), (256, 256), (128, 128), (128, 256), (256, 128), (64, 64), (256, 176), (64, 32), (256, 176), (128, 128),
            (256, 176))                                            # kVariants: (bm, bn)
N_VARIANTS = len(VARIANTS)


def _ceil(a, b):
    return -(-a // b)


def tiled_supported(M, N, K):
    return M > 0 and N % 176 == 0 and K % 256 == 0 and _ceil(M, 256) * (N // 176) >= 192


def fr128_shape(M, N, K):
    return M > 0 and N % 128 == 0 and K % 256 == 0 and K >= 768


def frw4_shape(M, N, K):
    return M > 0 and (N % 176 == 0 or N % 128 == 0) and K % 256 == 0 and K >= 768


def _u8_grid(c):
    return c.grid in U8_FAST


def fr_supported(c):
    return _u8_grid(c) and c.K % 256 == 0 and c.K >= 768 and c.N % 176 == 0


def pick_variant(M, N, w4, forced=-1):
    if forced >= 0:
        return forced
    blocks = lambda v: _ceil(M, VARIANTS[v][0]) * _ceil(N, VARIANTS[v][1])
    if w4:
        if blocks(2) >= 224:
            return 2
        if blocks(10) >= 96:
            return 10
        return 6 if blocks(6) >= 256 else 8
    if N % 176 == 0 and blocks(1) >= 192:
        return 7
    if blocks(2) >= 224:
        return 2
    if blocks(5) >= 160:
        return 5
    if blocks(10) >= 96:
        return 10
    return 6 if blocks(6) >= 256 else 8


def run_gemm_kernel(c, a_tiled, resid=False):
    """run_gemm: the kernel name and its tile.  gemm_i8_kernel instances are "cpp_v<variant>" (7 with packed weights is variant 1's
    classic loop; 9 is the generated pp_asm loop with the C++ epilogue), None where the entry point answers MQ_EUNSUPPORTED."""
    M, N, K = c.M, c.N, c.K
    if a_tiled and not c.w4 and not tiled_supported(M, N, K) and fr128_shape(M, N, K) and not resid and _u8_grid(c):
        return "fr128", (256, 128)
    v = pick_variant(M, N, c.w4, c.variant)
    if a_tiled:
        if c.w4 or not tiled_supported(M, N, K):
            return None, None
        v = 11 if (fr_supported(c) and c.variant != 9) else 9
    elif v in (9, 11):
        v = 7
    if v == 11:
        return "fr", (256, 176)
    if v == 7 and c.w4:
        return "cpp_v1", VARIANTS[1]
    return "cpp_v%d" % v, VARIANTS[v]


def _hook(c, name, default=0):
    return c.hook[1] if c.hook and c.hook[0] == name else default


def kernels_of(c):
    """[(kernel name, (tile rows, tile columns))] of the launches that serve case c, in launch order."""
    M, N, K = c.M, c.N, c.K
    if c.entry in ("linear", "segmented"):
        return [run_gemm_kernel(c, False)]
    if c.entry == "linear_residual":
        return [run_gemm_kernel(c, False, True)]
    if c.entry == "tiled":
        return [run_gemm_kernel(c, True)]
    if c.entry == "tiled_w4":
        if not frw4_shape(M, N, K) or (c.segs and len(c.segs) > 1 and N % 128 != 0):
            return [(None, None)]
        return [("frw4x176", (256, 176))] if (not c.segs or len(c.segs) == 1) and N % 176 == 0 else [("frw4x128", (256, 128))]
    if c.entry == "tiled_segmented":
        if not fr128_shape(M, N, K):
            return [(None, None)]
        if N % 160 == 0 and _ceil(M, 128) * (N // 160) <= 256 and _hook(c, "mq_gemm_set_segmented_tile") != 128:
            return [("fr160", (128, 160))]
        return [("fr128", (256, 128))]
    if c.entry == "tiled_residual":
        if not fr128_shape(M, N, K) or c.grid not in GRID16_F32:
            return [(None, None)]
        if c.w4:
            return [("frw4r", (128, 128))]
        forced = _hook(c, "mq_gemm_set_residual_tile")
        tall = forced == 256 if forced in (128, 256) else _ceil(M, 128) * (N // 128) > 512
        return [("fr128r8", (256, 128))] if tall else [("fr128r", (128, 128))]
    if c.entry == "pair":
        if not tiled_supported(M, N, K) or not fr_supported(c):
            return [(None, None)]
        return [("fr_pair_persistent" if _hook(c, "mq_gemm_set_pair_mode") == 1 else "fr_pair", (256, 176))]
    if c.entry == "gated":
        wide = tiled_supported(M, N, K) and N % 64 == 0 and ((N % 176 == 0 and K % 256 == 0 and K >= 768) if c.w4 else fr_supported(c))
        narrow = not wide and fr128_shape(M, N, K) and _ceil(M, 256) * (N // 128) >= 192
        if not (wide or narrow) or M > 256 * 512:
            return [(None, None)]
        bn = 176 if wide else 128
        first = ("frw4x%d" % bn) if c.w4 else ("fr" if wide else "fr128")
        return [(first, (256, bn)), (("frgw4x%d" if c.w4 else "frg%d") % bn, (256, bn))]
    raise ValueError(c.entry)


def tile_of_block(bid, nblk, grid_m, grid_n, group_m=0):
    """csrc/mq_gemm.hip tile_of_block: the XCD-aware remap of the linear block id, then the grouped (GROUP_M tall) tile order."""
    q, r = nblk >> 3, nblk & 7
    xcd, idx = bid & 7, bid >> 3
    L = (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + idx
    G = group_m if group_m > 0 else 4
    per_group = G * grid_n
    g = L // per_group
    first_m = g * G
    gm = min(grid_m - first_m, G)
    in_g = L - g * per_group
    return first_m + in_g % gm, in_g // gm


# ---- operands ---------------------------------------------------------------------------------------------------------------------
def _seed(*parts):
    return zlib.crc32(repr(parts).encode())


def col_classes(N):
    return COL_CLASS[np.arange(N) % COL_PERIOD]


def _span(c):
    g = GRIDS[c.grid]
    return 255 if g is None else g.qmax - g.qmin


@functools.lru_cache(maxsize=4)
def activations(M, K):
    """(a int8 [M, K], row sums int32 [M]): rows by m % 16 as the module docstring says."""
    rng = np.random.default_rng(_seed("a", M, K))
    a = rng.integers(-128, 128, size=(M, K)).astype(np.int8)
    low = (np.arange(M) % 16) < 10
    a[low] = rng.integers(-2, 2, size=(int(low.sum()), K)).astype(np.int8)
    a[~low, 0], a[~low, K - 1] = -128, 127
    if M > ZERO_ROW:
        a[ZERO_ROW] = 0
    return a, a.astype(np.int64).sum(axis=1).astype(np.int32)


def _tie_nnz(span, K, c, k):
    """Non-zero effective weights of a tie column: enough for a spread of a fifth of the grid on the low rows (activations of
    standard deviation 1.1, weights 4.6), at least 4, at most K."""
    target = span / 5.0 / (c / 2.0 ** k)
    return int(min(K, max(4, round((target / (1.1 * 4.6)) ** 2))))


@functools.lru_cache(maxsize=6)
def weights(N, K, w4, rowsum, span, which):
    """(w stored integers [N, K] (int8, or the unsigned nibbles), w_zp int32 [N], col_term int32 [N]).  `which` numbers the linears
    that share an activation (pair, gated)."""
    rng = np.random.default_rng(_seed("w", N, K, w4, rowsum, span, which))
    cls = col_classes(N)
    j = np.arange(N) % COL_PERIOD
    lo, hi = (0, 16) if w4 else (-128, 128)
    w = rng.integers(lo, hi, size=(N, K)).astype(np.int64)
    zp = rng.integers(-255, 256, size=N).astype(np.int64)
    gen = np.flatnonzero(cls == "generic")
    zp[gen[0::10]], zp[gen[1::10]] = 255, -255
    ct = rng.integers(-4000, 4000, size=N).astype(np.int64)
    for n in np.flatnonzero(cls == "tie"):
        c_, k_ = TIE_CK[j[n]]
        eff = np.zeros(K, np.int64)
        nnz = _tie_nnz(span, K, c_, k_)
        eff[rng.permutation(K)[:nnz]] = rng.integers(-8, 8, size=nnz)
        zp[n] = 8 if w4 else int(rng.integers(-1, 2))
        if not rowsum:
            zp[n] = 0
            eff = np.abs(eff) if w4 else eff
        w[n] = eff + zp[n]
        ct[n] = int(rng.integers(-3, 4)) + int(round(0.5 * eff.sum()))      # the low rows' activations average -1/2: t centred at 0
    for n in np.flatnonzero(cls == "near"):
        w[n], zp[n], ct[n] = w[n - 6], zp[n - 6], ct[n - 6]
    ct[cls == "sat"] = 0
    for n in np.flatnonzero(cls == "big"):
        ct[n] = BIG_CT[j[n] - 26] * (1 << 24) + int(rng.integers(-(1 << 20), 1 << 20)) * 2 + 1
    if not rowsum:
        zp[:] = 0
    assert w.min() >= lo and w.max() < hi
    return w, zp.astype(np.int32), ct.astype(np.int32)


def _solve_mul(target, inv):
    """An fp32 x with fl(x * inv) == target (both fp32), or None: the quotient and its neighbours within 4 ulp."""
    target, inv = F32(target), F32(inv)
    x0 = F32(target / inv)
    for d in (0, 1, -1, 2, -2, 3, -3, 4, -4):
        x = (np.array([x0], F32).view(np.int32) + d).view(F32)[0]
        if F32(x * inv) == target:
            return x
    return None


def _ulps(v, d):
    return (np.array([v], F32).view(np.int32) + (d if v >= 0 else -d)).view(F32)[0]


Problem = namedtuple("Problem", "a a_rowsum w w_zp col_term alpha bias grids seg_end resid t")


@functools.lru_cache(maxsize=3)
def problem(c, which=0):
    """Every operand of linear `which` of case c, and its exact accumulators t (oracle.prefill_gemm_acc)."""
    g = GRIDS[c.grid]
    M, N, K = c.M, c.N, c.K
    span = _span(c)
    a, rs = activations(M, K)
    w, zp, ct = weights(N, K, c.w4, c.rowsum, span, which)
    t = O.prefill_gemm_acc(a, w, rs if c.rowsum else None, zp, ct)
    rng = np.random.default_rng(_seed("e", c.id, which))
    cls = col_classes(N)
    j = np.arange(N) % COL_PERIOD
    # grids: one per column segment; the middle one of three (the second of two) takes the power-of-two scale, or all with p2
    if g is None:
        grids, ends, qmin, qmax, fold = None, None, 0.0, 255.0, False
        sc, oo = np.full(N, F32(0.0371)), np.full(N, F32(128.0))    # (only shape alpha and bias: outputs of a few units)
    else:
        n_seg = len(c.segs) if c.segs else 1
        grids = []
        for i in range(n_seg):
            p2 = c.p2 or (n_seg > 1 and i == 1)
            grids.append((F32(g.scale_p2 if p2 else g.scale * (1 + 0.37 * i)), F32(g.offset + (3 * i if g.qmin == 0 else 0))))
        ends = list(c.segs) if c.segs else None
        qmin, qmax, fold = float(g.qmin), float(g.qmax), span <= 255
        sc, oo = O.prefill_gemm_columns(N, grids, ends)
    inv = (F32(1.0) / sc).astype(F32)
    centre = (qmin + qmax) / 2
    tl = t.astype(np.float64)
    full = (np.arange(M) % 16) >= 10
    mean, std = tl.mean(axis=0), tl.std(axis=0) + 1.0
    std_full = tl[full].std(axis=0) + 1.0 if full.sum() > 1 else std
    if not c.bias and g is not None:                               # no bias to centre a generic column with: col_term does it
        shift = np.where(cls == "generic", -np.rint(mean), 0.0).astype(np.int64)
        ct = (ct.astype(np.int64) + shift).astype(np.int32)
        t = (t.astype(np.int64) + shift[None, :]).astype(np.int32)
        mean = mean + shift
    alpha, bias = np.empty(N, F32), np.empty(N, F32)
    for n in range(N):
        k = cls[n]
        off = float(oo[n])
        if k in ("tie", "near"):
            c_, k_ = TIE_CK[j[n] if k == "tie" else j[n] - 6]
            al = None
            while al is None:                                      # an alpha whose product with inv IS the dyadic: next odd c otherwise
                al = _solve_mul(c_ / 2.0 ** k_, inv[n])
                c_ += 0 if al is not None else 2
            b_int = round(centre - off) + int(j[n] % 3) - 1        # B' = b_int + offset (folded) or b_int: an integer
            if span >= 255 and abs(b_int + (off if fold else 0)) < 48:
                b_int += 64                                        # (an ulp of a B' near 0 is lost in every q beyond twice its size)
            bs = None
            while bs is None:
                b_int += b_int == 0                                # (never 0: its ulp neighbours would be denormals)
                want = F32(b_int + off) if fold else F32(b_int)
                if k == "near":
                    want = _ulps(want, NEAR_ULPS[j[n] - 6])
                x = F32(want - F32(off)) if fold else want         # fl(bias * inv), exact difference
                bs = _solve_mul(x, inv[n]) if F32(x + F32(off) if fold else x) == want else None
                b_int += 0 if bs is not None else 1
            alpha[n], bias[n] = al, bs
            continue
        if k == "generic":
            a1 = span / 4.0 / std[n] * (1.0 + 0.3 * rng.random())
            b1 = centre - mean[n] * a1 + rng.standard_normal() * span / 10.0
        elif k == "sat":
            a1 = 4.0 * span / std_full[n]
            step = SAT_STEPS[j[n] - 20]
            b1 = (qmin if step[:2] == "lo" else qmax) + {"-1": -1, "": 0, "+1": 1}[step[2:]] + 0.3
            if not c.bias and g is not None:                       # no bias to place the zero row with: col_term (0 so far) does it
                ct_n = int(round((b1 - off) / a1)) or 1
                a1 = (b1 - off) / ct_n
                ct[n] += ct_n                                      # (ct and t are this call's own arrays since the shift above)
                t[:, n] += np.int32(ct_n)
        else:
            a1 = span / 4.0 / std[n]
            b1 = centre - mean[n] * a1
        alpha[n] = F32(a1 * float(sc[n]))
        bias[n] = F32((b1 - off) * float(sc[n]))
    if not c.bias:
        bias = None
    resid = None
    if c.entry in ("linear_residual", "tiled_residual"):
        resid = (rng.standard_normal((M, N)) * 3.0).astype(F32)
    return Problem(a, rs if c.rowsum else None, w, zp, ct, alpha, bias, grids, ends, resid, t)


Expect = namedtuple("Expect", "stored q tie a1 b1")


def storage_of(c):
    g = GRIDS[c.grid]
    return NONE_STORAGE[c.grid] if g is None else g.storage


@functools.lru_cache(maxsize=3)
def expect(c, which=0):
    """The oracle's storage array of linear `which` of case c with q, its tie distance, and the per-column A', B' of the report."""
    p = problem(c, which)
    g = GRIDS[c.grid]
    qmin, qmax = (0, 255) if g is None else (g.qmin, g.qmax)
    stored, q, tie = O.prefill_gemm_epilogue(p.t, p.alpha, p.bias, p.grids, p.seg_end, qmin, qmax, storage_of(c), p.resid)
    bs = np.zeros(c.N, F32) if p.bias is None else p.bias
    if g is None:
        return Expect(stored, q, tie, p.alpha, bs)
    sc, oo = O.prefill_gemm_columns(c.N, p.grids, p.seg_end)
    inv = (F32(1.0) / sc).astype(F32)
    b1 = (bs * inv).astype(F32)
    return Expect(stored, q, tie, (p.alpha * inv).astype(F32), (b1 + oo).astype(F32) if qmax - qmin <= 255 else b1)


def conditions(c, which=0):
    """The counts test_gemm_oracle.py holds every case to, from the oracle alone: exact ties by the parity of their floor (inside the
    clamps), clamped outputs per sat column and end, outputs one step outside / on / inside either clamp, |t| > 2^24 with a conversion
    that rounds, and the largest |t| (no int32 wrap: the exact sum equals the wrapped one)."""
    p, e = problem(c, which), expect(c, which)
    g = GRIDS[c.grid]
    cls = col_classes(c.N)
    t64 = p.t.astype(np.int64)
    big = np.abs(t64) > (1 << 24)
    rounds = big & (p.t.astype(F32).astype(np.int64) != t64)
    out = {"big": int(big.sum()), "big_rounds": int(rounds.sum()), "tmax": int(np.abs(t64).max())}
    exact = np.rint(p.a.astype(np.float64) @ p.w.astype(np.float64).T).astype(np.int64)        # exact below 2^53, never wrapped
    if p.a_rowsum is not None:
        exact -= p.w_zp.astype(np.int64)[None, :] * p.a_rowsum.astype(np.int64)[:, None]
    out["wraps"] = int((exact + p.col_term.astype(np.int64)[None, :] != t64).sum())
    if g is None:
        return out
    fold = g.qmax - g.qmin <= 255
    _, oo = O.prefill_gemm_columns(c.N, p.grids, p.seg_end)
    r = np.rint(e.q) + (0.0 if fold else oo.astype(np.float64)[None, :])          # the index in front of the clamp
    fl = np.floor(e.q) + (0.0 if fold else oo.astype(np.float64)[None, :])
    is_tie = (e.tie == 0.0) & (fl >= g.qmin) & (fl + 1 <= g.qmax)
    out["tie_even"] = int((is_tie & (np.floor(e.q) % 2 == 0)).sum())
    out["tie_odd"] = int((is_tie & (np.floor(e.q) % 2 == 1)).sum())
    near = cls == "near"
    out["near_tie"] = int(((e.tie[:, near] > 0) & (e.tie[:, near] < 1e-3)).sum())
    sat = cls == "sat"
    out["sat_lo_min"] = int((r[:, sat] < g.qmin).sum(axis=0).min())
    out["sat_hi_min"] = int((r[:, sat] > g.qmax).sum(axis=0).min())
    out["sat_rows"] = c.M
    for name, v in (("lo-1", g.qmin - 1), ("lo", g.qmin), ("lo+1", g.qmin + 1), ("hi-1", g.qmax - 1), ("hi", g.qmax), ("hi+1", g.qmax + 1)):
        out[name] = int((r == v).sum())
    return out


# ---- gated pair -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def gate_table():
    """An arbitrary int8 map of the 65 536 index pairs (the kernels only look it up): every value, both extremes."""
    rng = np.random.default_rng(_seed("table"))
    tb = rng.integers(-128, 128, size=65536).astype(np.int8)
    tb[0], tb[65535], tb[255], tb[255 * 256] = -128, 127, 127, -128
    return tb


# ---- case lists -------------------------------------------------------------------------------------------------------------------
S1, S2, S3 = (37, 180, 256), (300, 260, 384), (257, 352, 128)      # ragged M, N % 16 != 0 (element-wise stores), one / two / three stages
ROWMAJOR_SHAPES = (S1, S2, S3)
CPP_VARIANTS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 10)                     # gemm_i8_kernel instances row-major operands reach
ALL_TYPES = ("i8u", "s8", "u4", "u16", "i16", "f32_8", "f16_8", "f32_16", "f16_16", "none32", "none16")

ROWMAJOR_CASES = []
for _i, _v in enumerate(CPP_VARIANTS):                             # the u8 fast path on every variant, int8 and packed weights
    ROWMAJOR_CASES.append(_case("linear", ROWMAJOR_SHAPES[_i % 3], "u8", variant=_v))
    ROWMAJOR_CASES.append(_case("linear", ROWMAJOR_SHAPES[(_i + 1) % 3], "u8", w4=True, variant=_v, p2=bool(_i & 1)))
for _g in ALL_TYPES:                                               # every output type on two variants
    ROWMAJOR_CASES.append(_case("linear", S2, _g, variant=3))
    ROWMAJOR_CASES.append(_case("linear", S1, _g, w4=True, variant=8, p2=True))
ROWMAJOR_CASES += [
    _case("linear", S3, "u8", variant=10, bias=False, rowsum=False),
    _case("linear", S1, "u16", w4=True, variant=6, bias=False, rowsum=False),
    _case("linear", S2, "f32_8", variant=7, bias=False),
    _case("linear", S2, "u4", bias=True, rowsum=False),
    _case("linear_residual", S2, "f32_16"),
    _case("linear_residual", S1, "f32_8", variant=5),
    _case("linear_residual", S3, "none32", variant=0, bias=False),
    _case("segmented", S2, "u8", segs=(260,)),
    _case("segmented", S2, "u8", segs=(132, 260), variant=3),
    _case("segmented", (300, 384, 384), "u8", segs=(132, 260, 384), variant=5),
    _case("segmented", (300, 384, 384), "u8", segs=(128, 256, 384), variant=7),
    _case("segmented", S2, "u8", w4=True, segs=(132, 260)),
    _case("segmented", (37, 384, 256), "u8", w4=True, segs=(132, 260, 384), variant=4),
]

SEG_TILE, RES_TILE, PAIR_MODE = "mq_gemm_set_segmented_tile", "mq_gemm_set_residual_tile", "mq_gemm_set_pair_mode"
TILED128_CASES = [
    _case("tiled_segmented", (37, 384, 768), "u8", segs=(132, 260, 384)),                          # fr128
    _case("tiled_segmented", (300, 384, 1024), "u8", segs=(128, 256, 384), p2=True),               # fr128, tile-aligned ends
    _case("tiled_segmented", (300, 128, 1280), "u8", segs=(128,), bias=False, rowsum=False),       # fr128, one grid
    _case("tiled_segmented", (300, 640, 768), "u8", segs=(132, 260, 640)),                         # fr160
    _case("tiled_segmented", (37, 640, 1024), "u8", segs=(164, 640), bias=False),                  # fr160
    _case("tiled_segmented", (300, 640, 768), "u8", segs=(132, 260, 640), hook=(SEG_TILE, 128)),   # fr128 on fr160's shape
    _case("tiled", (37, 384, 768), "i8u"),                                                         # fr128 through run_gemm
    _case("tiled", (300, 640, 1280), "u8", p2=True),
    _case("tiled_residual", (300, 384, 768), "f32_16", hook=(RES_TILE, 128)),                      # fr128r: 3 x 3 tiles of 128 rows
    _case("tiled_residual", (300, 384, 768), "f32_16", hook=(RES_TILE, 256)),                      # fr128r8
    _case("tiled_residual", (37, 128, 1280), "f32_i16", bias=False, rowsum=False),                 # fr128r by shape
    _case("tiled_residual", (300, 640, 1024), "f32_i16", hook=(RES_TILE, 256), p2=True),
    _case("tiled_residual", (300, 384, 1024), "f32_16", hook=(RES_TILE, 512)),                     # split-K: experiment builds only
    _case("tiled_w4", (300, 384, 1024), "u8"),                                                     # frw4x128, one grid
    _case("tiled_w4", (300, 384, 768), "i8u", segs=(132, 260, 384)),
    _case("tiled_w4", (37, 640, 768), "u8", segs=(164, 640), bias=False, rowsum=False),
    _case("tiled_w4", (300, 352, 768), "u8"),                                                      # frw4x176
    _case("tiled_w4", (37, 352, 1280), "i8u", segs=(352,), p2=True),
    _case("tiled_residual", (300, 384, 768), "f32_16", w4=True),                                   # frw4r
    _case("tiled_residual", (37, 128, 1280), "f32_i16", w4=True, bias=False, rowsum=False),
]

W1, W2, WN = (1793, 4224, 768), (2049, 3872, 1024), (1793, 3072, 768)      # 8 x 24 tiles with a one-row tail; 9 x 22 = 198; narrow gate
WIDE_CASES = [
    _case("tiled", W1, "u8"),                                                                      # fr
    _case("tiled", W2, "i8u", bias=False, rowsum=False, p2=True),
    _case("tiled", W1, "u8", variant=9),                                                           # pp_asm + the C++ fast path
] + [_case("tiled", W2 if _i & 1 else W1, _g) for _i, _g in enumerate(("s8", "u4", "u16", "i16", "f32_8", "f16_8", "f32_16", "f16_16"))] + [
    _case("pair", W1, "u8", hook=(PAIR_MODE, 0)),
    _case("pair", W2, "i8u", hook=(PAIR_MODE, 1)),
    _case("gated", W1, "u8"),                                                                      # fr + frg176
    _case("gated", WN, "u8", bias=False),                                                          # fr128 + frg128
    _case("gated", W1, "u8", w4=True, p2=True),                                                    # frw4x176 + frgw4x176
    _case("gated", WN, "u8", w4=True),                                                             # frw4x128 + frgw4x128
]
ALL_CASES = ROWMAJOR_CASES + TILED128_CASES + WIDE_CASES
SPLITK_ONLY = [c for c in ALL_CASES if c.hook == (RES_TILE, 512)]

# what the case lists have to reach: kernel -> the grid classes it accepts (every one of them has to arrive there)
INDEX_GRIDS = {"u8", "i8u"}
REACH = dict([("cpp_v%d" % v, {"u8"}) for v in CPP_VARIANTS] + [
    ("cpp_v3", set(ALL_TYPES) | {"u8"}), ("cpp_v8", set(ALL_TYPES) | {"u8"}),
    ("cpp_v9", {"u8", "s8", "u4", "u16", "i16", "f32_8", "f16_8", "f32_16", "f16_16"}),
    ("fr", INDEX_GRIDS), ("fr_pair", {"u8"}), ("fr_pair_persistent", {"i8u"}), ("fr128", INDEX_GRIDS), ("fr160", {"u8"}),
    ("fr128r", set(GRID16_F32)), ("fr128r8", set(GRID16_F32)), ("frg176", {"u8"}), ("frg128", {"u8"}),
    ("frw4x176", INDEX_GRIDS), ("frw4x128", INDEX_GRIDS), ("frw4r", set(GRID16_F32)), ("frgw4x176", {"u8"}), ("frgw4x128", {"u8"}),
])
