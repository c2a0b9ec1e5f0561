"""GPU: the element-wise kernels that feed every prefill GEMM its int8 image -- mq_rmsnorm_quant / mq_layernorm_quant (mq_norm.hip) and
mq_act_quant / mq_gated_act_quant / mq_gated_table / mq_gated_lookup[_tiled] (mq_activation.hip) -- against oracle.prefill_*, at every
dispatch branch.  What the oracle cannot replay is observed from the kernel or bounded by a derived fp32 error; everything behind it is
held bit for bit; every excluded share is capped, and test_prefill_elementwise_oracle.py checks the caps on these inputs on the CPU.

RMSNorm: the fp32 row scalar r depends on the kernel's summation order, so it is SEARCHED among the fp32 neighbours of the float64 r
within the derived bound (at most 51 candidates on these inputs); with it prefill_norm_replay gives every y, q_out, q_tiled and row_sum
of the row bit for bit.  No excluded share, 8- and 16-bit output grids and none.
LayerNorm: every element whose `tie` is clear equals the float64 oracle's index, a flagged one is within one step (flagged share of
the oracle with an 8-bit grid: at most 0.078 % in any case, 0.014 % over all of them); without an output grid every value lies within
the derived fp32 bound.  (A row-scalar replay would need the pair (r, shift) of a row; it is not searched here.)
Both: y is dequant of the written index, q_tiled is tiled_image(q_out), row_sum is the sum of the image, canaries stay.
mq_act_quant: bit for bit wherever _gate_chain's `tie` (2^-17 relative, exp / erf) is clear, within one step of the output grid where
set: per quantizer at most 1 of the 1027 base inputs (0.097 %) is flagged.
Gated routes: the activation value is observed (mq_act_quant on the 256 values of a's grid: 0 of 256 flagged on the gated grids, so the
observation is the oracle's bit for bit); given it, every table entry, q, row_sum and y of every route equals prefill_gate with no
exception.
Every norm case comes from prefill_elementwise_cases.NORM_CASES by tag, the activation and gated inputs from the same module: what is
launched here is what the CPU file caps."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import prefill_elementwise_cases as C  # noqa: E402
from oracle import mq_oracle as O  # noqa: E402
from test_gpu_round2 import tiled_image  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
CF, CQ, CI = -7777.0, 85, 7           # canaries: fp32, int8, int32
PAD = 64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    import mobilequant_amd._lib as L
    assert L.device_info()["arch"].startswith("gfx950")
    return torch.device("cuda:0")


def _call(name, *args):
    from mobilequant_amd import ops
    ops._lib.call(name, *args)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)                     # a copy: the shared inputs are read-only


def _g(g, dev, keep):
    """(scale ptr, offset ptr, qmin, qmax) of a QuantizerOracle on the device; None: an absent grid."""
    if g is None:
        return [None, None, 0.0, 0.0]
    s, o = torch.tensor([float(g.scale)], device=dev), torch.tensor([float(g.offset)], device=dev)
    keep += [s, o]
    return [s.data_ptr(), o.data_ptr(), float(g.qmin), float(g.qmax)]


def _buf(n, fill, dtype, dev):
    return torch.full((n + PAD,), fill, dtype=dtype, device=dev)


def _take(t, n, fill, what):
    h = t.cpu().numpy()
    assert np.all(h[n:] == fill), "canary behind %s changed" % what
    return h[:n]


def same(a, b):
    """Bit for bit, NaN exactly where the other has NaN."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


def untile(img, cols):
    """Inverse of tiled_image: the fragment-blocked bytes -> [ceil16(rows), cols] row-major."""
    mp = img.size // cols
    out = img.reshape(mp // 16, cols // 64, 4, 16, 16).transpose(0, 3, 1, 2, 4).reshape(mp, cols)
    assert np.array_equal(tiled_image(out).reshape(-1), img.reshape(-1))
    return out


# ---- norm -----------------------------------------------------------------------------------------------------------------------
def run_norm(dev, c, want_y, emit_q, emit_tiled):
    """One launch of the C entry on buffers with canaries behind them.  Returns dict(y [rows, cols], q, rs, qt [ceil16(rows), cols]
    un-tiled with the canary left in the padding rows) -- None for what was not asked."""
    keep = []
    x = _t(c["x"], dev)
    rows, cols = c["x"].shape
    w = _t(c["w"], dev)
    b = _t(c["b"], dev) if c["b"] is not None else None
    mp = (rows + 15) // 16 * 16
    y = _buf(rows * cols, CF, torch.float32, dev) if want_y else None
    q = _buf(rows * cols, CQ, torch.int8, dev) if emit_q else None
    qt = _buf(mp * cols, CQ, torch.int8, dev) if emit_tiled else None
    rs = _buf(rows, CI, torch.int32, dev) if (emit_q or emit_tiled) else None
    p = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
    gi, go = _g(c["in_q"], dev, keep), _g(c["out_q"], dev, keep)
    _call("mq_layernorm_quant" if c["layernorm"] else "mq_rmsnorm_quant", x.data_ptr(), rows, cols, w.data_ptr(), p(b), float(c["eps"]),
          *gi, *go, p(y), p(q), p(qt), int(c["shift"]), p(rs), _stream())
    torch.cuda.synchronize()
    out = dict(y=None, q=None, rs=None, qt=None)
    if want_y:
        out["y"] = _take(y, rows * cols, CF, "y").reshape(rows, cols)
    if emit_q:
        out["q"] = _take(q, rows * cols, CQ, "q_out").reshape(rows, cols)
    if rs is not None:
        out["rs"] = _take(rs, rows, CI, "row_sum").astype(np.int64)
    if emit_tiled:
        out["qt"] = untile(_take(qt, mp * cols, CQ, "q_tiled"), cols)
        assert np.all(out["qt"][rows:] == CQ), "the padded tail of the tiled image was written"
    return out


def find_r(c, r, i, got):
    """An fp32 row scalar within the derived bound of the float64 one for which the replay gives row i of every output the launch
    wrote, bit for bit; None when there is none."""
    cand = O.f32_between(r["r64"][i] - r["r_err"][i], r["r64"][i] + r["r_err"][i])
    assert 1 <= len(cand) <= 256
    cand = cand[np.argsort(np.abs(cand.astype(np.float64) - r["r64"][i]), kind="stable")]
    img = got["q"] if got["q"] is not None else (got["qt"] if got["qt"] is not None else None)
    n = min(64, c["x"].shape[1])
    bias = None if c["b"] is None else c["b"][:n]
    pre = O.prefill_norm_replay(r["xi"][i, :n][None, :], cand[:, None], 0.0, c["w"][:n], bias, False, c["out_q"], c["shift"])
    if got["y"] is not None:
        ok = np.array([same(pre["y"][k], got["y"][i, :n]) for k in range(len(cand))])
    else:
        ok = np.all(pre["q8"] == img[i, :n][None, :], axis=1)
    for rc in cand[ok]:
        rp = O.prefill_norm_replay(r["xi"][i], rc, 0.0, c["w"], c["b"], False, c["out_q"], c["shift"])
        if got["y"] is not None and not same(rp["y"], got["y"][i]):
            continue
        if img is not None and not (np.array_equal(rp["q8"], img[i]) and int(rp["rs"]) == int(got["rs"][i])):
            continue
        return rc
    return None


def check_norm(c, got, rows_to_judge=None, tag=None):
    """Checks 1 - 3 of the module docstring on one launch's outputs (rows_to_judge: only these rows against the oracle)."""
    r = C.norm_oracle(c)
    rows, cols = c["x"].shape
    judge = range(rows) if rows_to_judge is None else rows_to_judge
    out_q, shift = c["out_q"], c["shift"]
    img = got["q"] if got["q"] is not None else (got["qt"][:rows] if got["qt"] is not None else None)
    # 3. both norms: y is dequant of the written index, q_tiled is tiled_image(q_out), row_sum is the sum of the image
    if got["q"] is not None and got["y"] is not None:
        deq = O.dequantize_index(got["q"].astype(F32) + F32(shift), out_q.scale, out_q.offset)
        nan = np.isnan(got["y"])
        assert np.array_equal(deq[~nan].view(np.uint32), got["y"][~nan].view(np.uint32)), tag
        assert np.all(got["q"][nan] == out_q.qmin - shift), tag
    if got["q"] is not None and got["qt"] is not None:
        padded = np.full(got["qt"].shape, CQ, np.int8)
        padded[:rows] = got["q"]
        assert np.array_equal(tiled_image(padded), tiled_image(got["qt"])), tag
    if img is not None:
        assert np.array_equal(got["rs"], img.astype(np.int64).sum(axis=1)), tag
    if not c["layernorm"]:
        # 1. RMSNorm: a row scalar inside the bound replays the whole row
        for i in judge:
            assert find_r(c, r, i, got) is not None, (tag, "row", i, "no fp32 r within the bound replays the row")
        return
    # 2. LayerNorm
    sel = np.zeros((rows, 1), bool)
    sel[list(judge)] = True
    if out_q is None:
        assert np.all((np.abs(got["y"].astype(np.float64) - r["v64"]) <= r["err"] * (1 + 1e-6) + 1e-300) | ~sel), tag
        return
    clear = ~r["tie"] & sel
    flagged = r["tie"] & sel
    if img is not None:
        assert np.array_equal(img[clear], r["q8"][clear]), (tag, int((img != r["q8"])[clear].sum()))
        assert np.all(np.abs(img.astype(np.int64) - r["q8"].astype(np.int64))[flagged] <= 1), tag
    if got["y"] is not None:
        want = O.dequantize_index(r["idx"], out_q.scale, out_q.offset)
        assert np.array_equal(got["y"][clear].view(np.uint32), want[clear].view(np.uint32)), (tag, int((got["y"] != want)[clear].sum()))
        # one step at most: the value of the index below, of the index itself or of the one above (clamped), bit for bit -- a difference
        # in float steps would not do on a 16-bit grid, where fl((q - o) s) itself moves by 2e-3 of a step
        near = [O.dequantize_index(np.clip(r["idx"] + k, out_q.qmin, out_q.qmax), out_q.scale, out_q.offset) for k in (-1, 0, 1)]
        hit = (got["y"] == near[0]) | (got["y"] == near[1]) | (got["y"] == near[2])
        assert np.all(hit[flagged]), (tag, int((~hit)[flagged].sum()))


@pytest.mark.parametrize("layernorm", [False, True], ids=["rms", "layernorm"])
@pytest.mark.parametrize("cols,branch", C.NORM_COLS)
def test_norm_rowmajor(dev, cols, branch, layernorm):
    """rmsnorm_quant_kernel at each dispatch branch's first and last width, rows = 5, with bias on / off, the 16-bit input grid on / off
    and an 8-bit grid (y + q_out + row_sum, + q_tiled where cols % 64 == 0), a 16-bit grid (y) or none (y) behind it."""
    for bias, in_on, out_bits in C.NORM_CONFIGS:
        c = C.NORM_CASES[("rowmajor", cols, C.NORM_ROWS, layernorm, bias, in_on, out_bits)]
        got = run_norm(dev, c, True, out_bits == 8, out_bits == 8 and cols % 64 == 0)
        check_norm(c, got, tag=(cols, branch, layernorm, bias, in_on, out_bits))


@pytest.mark.parametrize("layernorm", [False, True], ids=["rms", "layernorm"])
def test_norm_generic_kernel_tiled_stores(dev, layernorm):
    """rows = 5 < 64 with the fragment-blocked output: the generic kernel's 4-byte tiled stores; with and without the row-major copy."""
    c = C.NORM_CASES[("generic-tiled",) + C.GENERIC_TILED + (layernorm,)]
    check_norm(c, run_norm(dev, c, True, True, True), tag="y + q + tiled")
    check_norm(c, run_norm(dev, c, False, False, True), tag="tiled only")


@pytest.mark.parametrize("layernorm", [False, True], ids=["rms", "layernorm"])
@pytest.mark.parametrize("rows", C.TILED_ROWS)
@pytest.mark.parametrize("cols", C.TILED_COLS)
def test_norm_tiled_image(dev, cols, rows, layernorm):
    """norm_tiled8_kernel (image only, rows >= 64, 1024 <= cols <= 4096): V = 1 / 2 / 4, its four-row and eight-row forms forced through
    mq_norm_tiled_set_rows and the default choice, rows ragged against the workgroup's rows and the 16-row tile."""
    try:
        for knob in C.TILED_KNOBS:
            _call("mq_norm_tiled_set_rows", knob)
            for bias in (False, True):
                c = C.NORM_CASES[("tiled", cols, rows, layernorm, bias, True, 8)]
                check_norm(c, run_norm(dev, c, False, False, True), tag=(cols, rows, layernorm, knob, bias))
    finally:
        _call("mq_norm_tiled_set_rows", 0)


@pytest.mark.parametrize("in_on", [False, True], ids=["in-off", "in16"])
@pytest.mark.parametrize("layernorm", [False, True], ids=["rms", "layernorm"])
def test_norm_nonfinite_rows(dev, layernorm, in_on):
    """NaN, +inf and -inf in rows 1, 2, 3 of [5, 1028]: y is NaN exactly where the oracle's is (RMSNorm without an input grid: an
    infinite element alone -- r = 0 zeroes the rest of its row, as the reference does; with the grid, or LayerNorm: the whole row), the
    integer image holds qmin - shift there, and rows 0 and 4 are judged as in every other case."""
    c = C.NORM_CASES[("nonfinite", 1028, C.NORM_ROWS, layernorm, in_on)]
    got = run_norm(dev, c, True, True, False)
    r = C.norm_oracle(c)
    nan = np.isnan(r["v64"])
    assert nan[1:4].any(axis=1).all() and not nan[[0, 4]].any()
    assert np.array_equal(np.isnan(got["y"]), nan)
    assert np.all(got["q"][nan] == c["out_q"].qmin - c["shift"])
    check_norm(c, got, rows_to_judge=[0, 4])
    if not layernorm:
        for i in (1, 2, 3):             # the row scalar of a poisoned row is exact: NaN, or 0 behind an infinite sum of squares
            rp = O.prefill_norm_replay(r["xi"][i], F32(r["r64"][i]), 0.0, c["w"], c["b"], False, c["out_q"], c["shift"])
            assert same(rp["y"], got["y"][i]) and np.array_equal(rp["q8"], got["q"][i]) and int(rp["rs"]) == int(got["rs"][i]), i
    else:
        assert nan[1:4].all()


# ---- mq_act_quant -------------------------------------------------------------------------------------------------------------
def run_act(dev, x, act, grids):
    keep = []
    xt = _t(x, dev)
    y = _buf(x.size, CF, torch.float32, dev)
    args = []
    for g in grids:
        args += _g(g, dev, keep)
    _call("mq_act_quant", xt.data_ptr(), x.size, int(act), *args, y.data_ptr(), _stream())
    torch.cuda.synchronize()
    return _take(y, x.size, CF, "y")


_ACT_REF = {}


def act_ref(act, mid_on, in_on):
    """The oracle on the 1027 base inputs, once per configuration (every numel is a prefix of their periodic continuation)."""
    key = (act, mid_on, in_on)
    if key not in _ACT_REF:
        r = O.prefill_act(C.act_base(), act, *C.act_grids(act, mid_on, in_on))
        r["y"].setflags(write=False)
        _ACT_REF[key] = r
    return _ACT_REF[key]


def check_act(got, want, tie, out_q):
    """Bit for bit where `tie` is clear; a flagged element within one step of the OUTPUT grid, whichever quantizer flagged it (a flag of
    the sigmoid grid moves the product by |x| s_mid, which may exceed that: the check errs strict there and would fail, not hide)."""
    clear = ~tie
    assert same(got[clear], want[clear]), int(clear.sum())
    with np.errstate(invalid="ignore"):
        assert np.all(np.abs(got[tie] - want[tie]) <= F32(out_q.scale) * F32(1.001))


@pytest.mark.parametrize("numel", C.ACT_NUMEL)
@pytest.mark.parametrize("act,mid_on,in_on", C.ACT_CONFIGS)
def test_act_quant(dev, act, mid_on, in_on, numel):
    """QSiLU / QGELU at the scalar tail alone (3), vector + tail (4, 7, 1027) and past one pass of the grid-stride loop (2 097 159: second
    trip and tail): bit for bit where `tie` is clear, one output-grid step where set.  Flagged per quantizer: at most 1 of 1027 base inputs."""
    grids = C.act_grids(act, mid_on, in_on)
    r = act_ref(act, mid_on, in_on)
    got = run_act(dev, C.act_input(numel), act, grids)
    check_act(got, np.resize(r["y"], numel), np.resize(r["tie"], numel), grids[2])


# ---- gated routes -------------------------------------------------------------------------------------------------------------
class Gated:
    """The grids on the device, the observed activation value per index of a's grid, and prefill_gate's 256 x 256 expectation."""

    def __init__(self, dev, act):
        self.dev, self.act, self.keep = dev, act, []
        self.va256, obs_grids, self.G = C.gated_observation(act)
        self.vb256 = O.dequantize_index(np.arange(256, dtype=F32), self.G["b"].scale, self.G["b"].offset)
        self.y1 = run_act(dev, self.va256, act, obs_grids)                                       # OBSERVED
        # ... and itself held to the oracle: none of the 256 inputs is flagged on these grids (checked on the CPU), so all 256 observed
        # values are the oracle's bit for bit and nothing behind them is excluded
        ref = O.prefill_act(self.va256, act, *obs_grids)
        assert not ref["tie"].any()
        assert same(self.y1, ref["y"])
        e = O.prefill_gate(self.y1[:, None], self.vb256[None, :], self.G["out"], 128)
        self.table, self.prod = e["q8"], e["prod"]
        self.ptrs = []
        for k, limits in (("a", False), ("b", False), ("mid", True), ("act", True), ("out", True)):
            g = _g(self.G[k], dev, self.keep)
            self.ptrs.append(g if limits else g[:2])

    def grid_args(self, index):
        a, b, mid, act, out = self.ptrs
        return (a if index else [None, None]) + (b if index else [None, None]) + mid + act + out

    def launch(self, a, b, want_y):
        """mq_gated_act_quant on uint8 indices or fp32 values [rows, cols] -> (q, rs, y | None)."""
        from mobilequant_amd import ops
        rows, cols = a.shape
        index = a.dtype == np.uint8
        at, bt = _t(a, self.dev), _t(b, self.dev)
        q, rs = _buf(rows * cols, CQ, torch.int8, self.dev), _buf(rows, CI, torch.int32, self.dev)
        y = _buf(rows * cols, CF, torch.float32, self.dev) if want_y else None
        _call("mq_gated_act_quant", at.data_ptr(), bt.data_ptr(), ops.MQ_U8 if index else ops.MQ_F32, rows, cols, self.act,
              *self.grid_args(index), 128, q.data_ptr(), rs.data_ptr(), y.data_ptr() if want_y else None, _stream())
        torch.cuda.synchronize()
        return (_take(q, rows * cols, CQ, "q").reshape(rows, cols), _take(rs, rows, CI, "row_sum").astype(np.int64),
                _take(y, rows * cols, CF, "y").reshape(rows, cols) if want_y else None)

    def kernel_table(self):
        t = _buf(65536, CQ, torch.int8, self.dev)
        _call("mq_gated_table", self.act, *self.grid_args(True), 128, t.data_ptr(), _stream())
        torch.cuda.synchronize()
        assert np.array_equal(_take(t, 65536, CQ, "table").reshape(256, 256), self.table)
        return t

    def lookup(self, a, b, table, tiled):
        rows, cols = a.shape
        mp = (rows + 15) // 16 * 16 if tiled else rows
        at, bt = _t(a, self.dev), _t(b, self.dev)
        q, rs = _buf(mp * cols, CQ, torch.int8, self.dev), _buf(rows, CI, torch.int32, self.dev)
        _call("mq_gated_lookup_tiled" if tiled else "mq_gated_lookup", at.data_ptr(), bt.data_ptr(), rows, cols, table.data_ptr(),
              q.data_ptr(), rs.data_ptr(), _stream())
        torch.cuda.synchronize()
        return _take(q, mp * cols, CQ, "q").reshape(mp, cols), _take(rs, rows, CI, "row_sum").astype(np.int64)

    def expect(self, a_idx, b_idx):
        q = self.table[a_idx, b_idx]
        return q, q.astype(np.int64).sum(axis=1), self.prod[a_idx, b_idx]

    def check_routes(self, rows, cols, routes):
        a_idx, b_idx = C.gated_indices(rows, cols)
        q, rs, prod = self.expect(a_idx, b_idx)
        va, vb = self.va256[a_idx], self.vb256[b_idx]
        for name in routes:
            if name == "index rows":
                gq, grs, gy = self.launch(a_idx, b_idx, False)
            elif name == "index wave + y":
                gq, grs, gy = self.launch(a_idx, b_idx, True)
            elif name == "values":
                gq, grs, gy = self.launch(va, vb, False)
            elif name == "values + y":
                gq, grs, gy = self.launch(va, vb, True)
            else:
                tiled = name == "lookup tiled"
                gq, grs = self.lookup(a_idx, b_idx, self.kernel_table(), tiled)
                gy = None
                if tiled:
                    padded = np.full(gq.shape, CQ, np.int8)
                    padded[:rows] = q
                    assert np.array_equal(gq, tiled_image(padded)), (name, rows, cols)
                    gq = q
            assert np.array_equal(gq, q), (name, rows, cols)
            assert np.array_equal(grs, rs), (name, rows, cols)
            if gy is not None:
                assert same(gy, prod), (name, rows, cols)


@pytest.fixture(scope="module", params=[0, 1], ids=["silu", "gelu"])
def gated(dev, request):
    return Gated(dev, request.param)


def test_gated_table_is_prefill_gate(gated):
    """Every entry of the 256 x 256 table behind the observed activation values; canary behind it."""
    gated.kernel_table()


@pytest.mark.parametrize("rows,cols", C.GATED_SHAPES)
def test_gated_routes(gated, rows, cols):
    """Every route at [1 | 5, 16 .. 2064]: a ragged last wave, widths around the wave kernel's 1024-element trip and past the row
    kernel's 2048-element one.  The tiled lookup needs cols % 64 == 0."""
    routes = ["index rows", "index wave + y", "values", "values + y", "lookup"] + (["lookup tiled"] if cols % 64 == 0 else [])
    gated.check_routes(rows, cols, routes)


def test_gated_wave_kernel_row_loop(gated):
    """[16389, 16]: 4098 workgroups' worth of rows against the wave kernel's cap of 4096, so its row loop runs a second trip."""
    gated.check_routes(*C.GATED_WAVE_LOOP, ["index wave + y", "values", "values + y", "index rows"])


def test_gated_lookup_row_loop(gated):
    """[2053, 64]: past the lookup's 512-workgroup cap (four rows each), row-major and tiled."""
    gated.check_routes(*C.LOOKUP_LOOP, ["lookup", "lookup tiled"])


@pytest.mark.parametrize("tiled", [False, True], ids=["rowmajor", "tiled"])
def test_gated_lookup_slow_path(gated, tiled):
    """Rows beyond 8192 columns: the lookup's looping path (8200 row-major: a ragged last trip; 8256 tiled)."""
    gated.check_routes(*C.LOOKUP_SLOW[tiled], ["lookup tiled" if tiled else "lookup"])


def test_gated_values_with_nan(gated):
    """NaN in either value input: the image holds qmin - shift, y is NaN; every other element as prefill_gate has it behind the
    activation value observed element by element."""
    rows, cols = 5, 1040
    a_idx, b_idx = C.gated_indices(rows, cols)
    va, vb = gated.va256[a_idx].copy(), gated.vb256[b_idx].copy()
    va[0, 3], va[4, 1039], vb[1, 16], vb[4, 1024] = np.nan, np.nan, np.nan, np.nan
    y1 = run_act(gated.dev, va.reshape(-1), gated.act, (None, gated.G["mid"], gated.G["act"])).reshape(rows, cols)
    e = O.prefill_gate(y1, vb, gated.G["out"], 128)
    for want_y in (False, True):
        gq, grs, gy = gated.launch(va, vb, want_y)
        assert np.array_equal(gq, e["q8"]) and np.array_equal(grs, e["q8"].astype(np.int64).sum(axis=1))
        for pos in ((0, 3), (4, 1039), (1, 16), (4, 1024)):
            assert gq[pos] == gated.G["out"].qmin - 128
            assert gy is None or np.isnan(gy[pos])
        assert gy is None or (same(gy, e["prod"]) and np.isnan(gy).sum() == 4)
