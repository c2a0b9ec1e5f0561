"""Inputs of the prefill element-wise pin, built once for the CPU cap checks (test_prefill_elementwise_oracle.py) and the GPU comparison
(test_gpu_prefill_elementwise.py): both files take every tensor and grid from here, so a seed or shape change moves both."""
import functools

import numpy as np

from oracle import mq_oracle as O

F32 = np.float32
EPS = 1e-5

# ---- norm -----------------------------------------------------------------------------------------------------------------------
# row-major kernel: every dispatch branch of launch_norm at its first and last width (mq_norm.hip), rows = 5: a ragged last workgroup
# of the wave-per-row form (4 rows per workgroup)
NORM_COLS = [(4, "V4/TPR64"), (60, "V4/TPR64"), (1020, "V4/TPR64"), (1024, "V1"), (1028, "V2"), (2048, "V2"), (2052, "V4"), (4096, "V4"),
             (4100, "V8"), (8192, "V8"), (8196, "re-read"), (12288, "re-read")]
NORM_ROWS = 5
# (bias, 16-bit input grid, output grid bits or None)
NORM_CONFIGS = [(b, i, o) for b in (False, True) for i in (False, True) for o in (8, 16, None)]
# norm_tiled8_kernel: V = 1 / 2 / 4, widths that are and are not a multiple of the 1024-column trip; rows ragged against the 4 / 8 rows
# of a workgroup and the 16-row tile
TILED_COLS = [1024, 1088, 2048, 2112, 4096]
TILED_ROWS = [64, 70, 77]
TILED_KNOBS = [0, 4, 8]
GENERIC_TILED = (5, 1088)                    # rows < 64: the generic kernel's tiled stores


def grid(bits, lo, hi):
    g = O.QuantizerOracle(bitwidth=bits)
    g.set_from_minmax(F32(lo), F32(hi))
    return g


@functools.lru_cache(maxsize=None)
def _norm_base(rows, cols, layernorm, nonfinite):
    rng = np.random.default_rng(1000003 * cols + 101 * rows + int(layernorm))
    x = (rng.standard_normal((rows, cols)) * 2.5 + (0.7 if layernorm else 0.0)).astype(F32)
    x[0, :4] = np.array([0.0, -0.0, 1e-9, -0.5], F32)
    if nonfinite:                            # rows 1 / 2 / 3; rows 0 and 4 stay clean
        x[1, 3 % cols], x[2, cols // 2], x[3, cols - 1] = np.nan, np.inf, -np.inf
    w_raw = (rng.standard_normal(cols) * 0.3 + 1.0).astype(F32)
    w = O.QuantizerOracle(16).forward(w_raw).astype(F32)          # the caller fake-quantises the weight once (16-bit, own range)
    b = (rng.standard_normal(cols) * 0.1).astype(F32)
    fin = x[np.isfinite(x)]
    in_q = grid(16, float(fin.min()) * 0.9, float(fin.max()) * 0.9)         # clips a little on purpose
    for a in (x, w, b):
        a.setflags(write=False)
    return x, w, b, in_q


def norm_case(rows, cols, layernorm, bias, in_on, out_bits, nonfinite=False):
    """One norm launch's inputs: dict(x, w, b, eps, layernorm, in_q, out_q, shift, n_red)."""
    x, w, b, in_q = _norm_base(rows, cols, bool(layernorm), bool(nonfinite))
    out_q = grid(out_bits, -4.0, 4.5) if out_bits else None                 # normalised rows * (1 +- 0.3) + 0.1: clips the tails
    return dict(x=x, w=w, b=b if bias else None, eps=EPS, layernorm=bool(layernorm), in_q=in_q if in_on else None, out_q=out_q,
                shift=128 if out_bits == 8 else 0, n_red=O.prefill_norm_n_red(cols))


def norm_oracle(c):
    return O.prefill_norm_rows(c["x"], c["w"], c["b"], c["eps"], c["layernorm"], c["in_q"], c["out_q"], c["shift"], c["n_red"])


def all_norm_cases():
    """(tag, case) of every norm input the GPU file launches."""
    for cols, _ in NORM_COLS:
        for ln in (False, True):
            for bias, in_on, out_bits in NORM_CONFIGS:
                yield ("rowmajor", cols, NORM_ROWS, ln, bias, in_on, out_bits), norm_case(NORM_ROWS, cols, ln, bias, in_on, out_bits)
    for cols in TILED_COLS:
        for rows in TILED_ROWS:
            for ln in (False, True):
                for bias in (False, True):
                    yield ("tiled", cols, rows, ln, bias, True, 8), norm_case(rows, cols, ln, bias, True, 8)
    for ln in (False, True):
        yield ("generic-tiled",) + GENERIC_TILED + (ln,), norm_case(GENERIC_TILED[0], GENERIC_TILED[1], ln, True, True, 8)
        for in_on in (False, True):
            yield ("nonfinite", 1028, NORM_ROWS, ln, in_on), norm_case(NORM_ROWS, 1028, ln, True, in_on, 8, nonfinite=True)


NORM_CASES = dict(all_norm_cases())          # the GPU file takes every norm case from here BY TAG: what it launches is what the CPU file caps


# ---- activation ---------------------------------------------------------------------------------------------------------------
ACT_NUMEL = [3, 4, 7, 1027, 2097152 + 7]      # scalar tail alone; vector + tail; one full grid-stride pass (2048 x 256 x 4) + second trip + tail
ACT_BASE_N = 1027
G_A = (8, -3.0, 2.5)                           # w1's output grid: the sweep holds its 256 dequantised values
ACT_IN = (16, -8.0, 8.0)
# A calibrated sigmoid range: on [0, 1] sigmoid(+-0) = 0.5 sits ON the boundary 127.5.  The three ranges below are chosen so that, per
# quantizer, at most one of the 1027 base inputs lies within 2^-17 relative of a rounding boundary (the window is ~0.4 % of a step at
# the top of an 8-bit grid, so an arbitrary choice flags 2 - 6 of them); test_prefill_elementwise_oracle.py holds the choice to the cap.
ACT_MID = (8, 0.0, 0.995)
ACT_OUT = {0: (8, -0.3, 7.0), 1: (8, -0.2, 7.0)}
# (act, mid grid, input grid): GELU has no mid quantizer
ACT_CONFIGS = [(0, False, False), (0, False, True), (0, True, False), (0, True, True), (1, False, False), (1, False, True)]


@functools.lru_cache(maxsize=None)
def act_base():
    """1027 inputs: non-finite values, +-0, values beyond +-20 (exp(-x) overflows at -100; erf saturates), every dequantised value of the
    8-bit grid G_A, and a spread over [-9, 9] -- shuffled behind the first eight, which every numel >= 7 sees."""
    ga = grid(*G_A)
    head = np.array([0.5, -0.0, np.nan, 25.0, -100.0, np.inf, -np.inf, 1e-9], F32)
    vals = O.dequantize_index(np.arange(256, dtype=F32), ga.scale, ga.offset)
    more = np.array([0.0, -25.0, 100.0, 21.0, -21.0, -1e-9], F32)
    rest = np.linspace(-9.0, 9.0, ACT_BASE_N - len(head) - 256 - len(more)).astype(F32)
    body = np.concatenate([vals, more, rest])
    np.random.default_rng(77).shuffle(body)
    base = np.concatenate([head, body]).astype(F32)
    assert base.shape == (ACT_BASE_N,)
    base.setflags(write=False)
    return base


def act_grids(act, mid_on, in_on):
    return (grid(*ACT_IN) if in_on else None, grid(*ACT_MID) if mid_on else None, grid(*ACT_OUT[act]))


def act_input(numel):
    """The first `numel` elements of the periodic continuation of act_base()."""
    return np.resize(act_base(), numel)


# ---- gated --------------------------------------------------------------------------------------------------------------------
# The gated routes rest on mq_act_quant's value at the 256 values of a's grid (gated_observation): with 256 inputs the 0.1 % cap means
# that NONE of them may be flagged, so the sigmoid and activation grids are chosen for that ([0, 0.995] flags index 228).
GATED_GRIDS = dict(a=G_A, b=(8, -2.0, 3.0), mid=(8, 0.0, 0.996), act=(8, -0.3, 2.5), out=(8, -4.0, 5.0))
GATED_SHAPES = [(r, c) for c in (16, 1008, 1024, 1040, 2064) for r in (1, 5)]
GATED_WAVE_LOOP = (16389, 16)                 # past the wave kernel's 4096-block cap (4 rows per block): its row loop runs twice
LOOKUP_LOOP = (2053, 64)                      # past the lookup's 512-block cap
LOOKUP_SLOW = {False: (5, 8200), True: (5, 8256)}      # tiled?: beyond 8192 columns


def gated_grids():
    return {k: grid(*v) for k, v in GATED_GRIDS.items()}


def gated_observation(act):
    """The launch that observes the activation value per index of a's grid: (va256, (in, mid, out) grids of mq_act_quant, all grids).
    act 0 SiLU, 1 GELU (no sigmoid grid)."""
    G = gated_grids()
    if act == 1:
        G["mid"] = None
    va256 = O.dequantize_index(np.arange(256, dtype=F32), G["a"].scale, G["a"].offset)
    return va256, (None, G["mid"], G["act"]), G


def gated_indices(rows, cols):
    rng = np.random.default_rng(20240607 + 7919 * rows + cols)
    a = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
    b = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
    n = min(256, cols)
    a[0, :n] = np.arange(n, dtype=np.uint8)
    b[0, :n] = np.arange(n, dtype=np.uint8)[::-1]
    return a, b
