"""CPU: the prefill element-wise oracle (oracle.prefill_norm_rows / prefill_norm_replay / prefill_act / prefill_gate) against the frozen
reference outputs, and the cap conditions of test_gpu_prefill_elementwise.py on the very inputs that file launches: the share of elements
the oracle itself flags as possible near-ties stays within 0.1 % per case and quantizer, and every RMSNorm row has between 1 and 256 fp32
candidates for its row scalar.  Realised figures (this file prints them with -s): LayerNorm, 8-bit output grid: at most 0.078 % in any
case (4 elements of [5, 1024]), 0.014 % over all cases (743 of 5 262 896); RMSNorm: 1 to 51 candidates per row; mq_act_quant: at most 1
of the 1027 base inputs (0.097 %) per quantizer; the gated routes' observation launch (256 values of w1's grid): 0 of 256."""
import numpy as np
import pytest

import prefill_elementwise_cases as C
from conftest import load_meta, load_npz
from oracle import mq_oracle as O

F32 = np.float32
CAP = 1e-3


def eq_nan(a, b):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


def _q(bits, rng):
    return C.grid(bits, *rng) if bits else None


# ---- against the frozen reference ---------------------------------------------------------------------------------------------
def test_norm_oracle_matches_frozen_reference():
    """qrmsnorm_cases.npz (QRMSNorm and QLayerNorm of the reference, torch CPU).  With an output grid: dequant of the float64 oracle's
    index IS the reference's output wherever `tie` is clear, and within one step where it is set; without one the reference's value lies
    within the derived fp32 bound of the float64 value.  RMSNorm: one of the enumerated fp32 row scalars replays every element of the
    row bit for bit (torch's rsqrt is 1 / sqrt, both correctly rounded, of a mean summed in another order)."""
    z = load_npz("qrmsnorm_cases.npz")
    seen = 0
    for m in load_meta(z):
        k = m["id"]
        ln = bool(m.get("layernorm"))
        x = z[k + "_x"].reshape(m["rows"], m["cols"])
        want = z[k + "_y"].reshape(m["rows"], m["cols"])
        in_q, out_q = _q(m["in_bits"], m["act"]["input"]), _q(m["out_bits"], m["act"]["output"])
        w = O.QuantizerOracle(16).forward(z[k + "_w"]).astype(F32)
        b = z[k + "_b"] if ln else None
        r = O.prefill_norm_rows(x, w, b, m["eps"], ln, in_q, out_q, 128, O.prefill_norm_n_red(m["cols"]))
        if out_q is None:
            assert np.all(np.abs(want.astype(np.float64) - r["v64"]) <= r["err"] + O.U32 * np.abs(r["v64"])), k
        else:
            got = O.dequantize_index(r["idx"], out_q.scale, out_q.offset)
            clear = ~r["tie"]
            assert np.array_equal(got[clear], want[clear]), k
            assert np.all(np.abs(got - want) <= F32(out_q.scale) * F32(1.001)), k
            assert clear.mean() > (0.999 if m["out_bits"] == 8 else 0.9), (k, clear.mean())
        if not ln:
            for i in range(m["rows"]):
                cand = O.f32_between(r["r64"][i] - r["r_err"][i], r["r64"][i] + r["r_err"][i])
                assert 1 <= len(cand) <= 256
                hit = [c for c in cand if np.array_equal(O.prefill_norm_replay(r["xi"][i], c, 0.0, w, None, False, out_q, 128)["y"], want[i])]
                assert hit, (k, i)
        seen += 1
    assert seen == 10


def test_act_oracle_matches_frozen_reference():
    """qact_cases.npz (QSiLU / QGELU of the reference): with an output grid the oracle's value is the reference's bit for bit wherever
    _gate_chain's `tie` is clear and one step away at most where it is set; without one, to the 3e-6 the math libraries differ by."""
    z = load_npz("qact_cases.npz")
    x = z["x"].reshape(-1)
    seen = 0
    for m in load_meta(z):
        act = 0 if m["kind"] == "silu" else 1
        in_q, out_q = _q(m["in_bits"], m["act"]["input"]), _q(m["out_bits"], m["act"]["output"])
        mid_q = C.grid(8, *m["act"].get("input2", [0.0, 1.0])) if act == 0 else None
        r = O.prefill_act(x, act, in_q, mid_q, out_q)
        want = z[m["id"] + "_y"].reshape(-1)
        if out_q is None:
            assert np.allclose(r["y"], want, rtol=3e-6, atol=2e-6), m
        else:
            clear = ~r["tie"]
            assert np.array_equal(r["y"][clear], want[clear]), m
            assert np.all(np.abs(r["y"] - want) <= F32(out_q.scale) * F32(1.001)), m
            assert clear.mean() > (0.995 if m["out_bits"] == 8 else 0.8), (m, clear.mean())
        seen += 1
    assert seen == 8


def test_nonfinite_conventions_match_frozen_reference():
    """nonfinite_cases.npz: NaN stays NaN and +-inf turns NaN in the value (round_ste), exactly where the reference's quantizer has it;
    the integer image holds qmin - shift there.  prefill_norm_replay with r = 1, w = 1 and prefill_gate with b = 1 are that quantizer."""
    z = load_npz("nonfinite_cases.npz")
    x = z["x"]
    one = np.ones(x.shape[1], F32)
    for m in load_meta(z):
        if m["is_per_channel"]:
            continue
        g = O.QuantizerOracle(m["bitwidth"], -1, m["is_symmetric"])
        g.set_from_minmax(*m["rng"])
        want = z[m["id"] + "_y"]
        shift = 128 if (m["bitwidth"] == 8 and not m["is_symmetric"]) else 0
        rp = O.prefill_norm_replay(x, F32(1.0), 0.0, one, None, False, g, shift)
        assert eq_nan(rp["y"], want), m
        assert np.array_equal(np.isnan(rp["y"]), ~np.isfinite(x))
        if m["bitwidth"] == 8:
            gt = O.prefill_gate(x, F32(1.0), g, shift)
            bad = np.isnan(want)
            assert np.all(rp["q8"][bad] == g.qmin - shift) and np.all(gt["q8"][bad] == g.qmin - shift)
            assert np.array_equal(gt["q8"], rp["q8"]) and eq_nan(gt["prod"], x)
            assert np.array_equal(O.dequantize_index(gt["q8"][~bad].astype(F32) + F32(shift), g.scale, g.offset), want[~bad])


def test_replay_with_the_float64_row_scalar_is_the_float64_index_away_from_ties():
    """The two norm oracles agree with each other: replaying a row with the fp32 rounding of the float64 row scalar gives the float64
    oracle's index wherever `tie` is clear (RMSNorm, every GPU width)."""
    for cols, _ in C.NORM_COLS:
        c = C.norm_case(C.NORM_ROWS, cols, False, True, True, 8)
        r = C.norm_oracle(c)
        rp = O.prefill_norm_replay(r["xi"], r["r64"].astype(F32)[:, None], 0.0, c["w"], c["b"], False, c["out_q"], c["shift"])
        assert np.array_equal(rp["q8"][~r["tie"]], r["q8"][~r["tie"]]), cols
        assert np.abs(rp["q8"].astype(int) - r["q8"].astype(int)).max() <= 1


# ---- the caps of the GPU file, on its inputs ------------------------------------------------------------------------------------
def test_norm_caps_hold_on_the_gpu_inputs():
    """LayerNorm with an 8-bit output grid: the oracle's own flagged share is within 0.1 % in every case the GPU file launches (the
    figure DESIGN.md section 3 states).  RMSNorm: every row has at least one and at most 256 fp32 candidates for r."""
    worst, flagged, total, worst_cand = (-1.0, ()), 0, 0, 0
    assert len(C.NORM_CASES) == len(list(C.all_norm_cases()))          # tags are unique: the GPU file looks its cases up by tag
    for tag, c in C.NORM_CASES.items():
        if tag[0] == "nonfinite":
            continue
        r = C.norm_oracle(c)
        if c["layernorm"]:
            if c["out_q"] is not None and c["out_q"].bitwidth == 8:
                share = float(r["tie"].mean())
                flagged, total = flagged + int(r["tie"].sum()), total + r["tie"].size
                worst = max(worst, (share, tuple(map(str, tag))))
                assert share <= CAP, (tag, share)
        else:
            for lo, hi in zip(r["r64"] - r["r_err"], r["r64"] + r["r_err"]):
                n = len(O.f32_between(lo, hi))
                worst_cand = max(worst_cand, n)
                assert 1 <= n <= 256, (tag, n)
    print("LayerNorm flagged share: worst case %.4f %% %s, overall %.4f %% (%d of %d); RMSNorm: at most %d candidates of r per row"
          % (100 * worst[0], worst[1], 100.0 * flagged / total, flagged, total, worst_cand))


@pytest.mark.parametrize("act,mid_on,in_on", C.ACT_CONFIGS)
def test_act_caps_hold_on_the_gpu_inputs(act, mid_on, in_on):
    """mq_act_quant: per quantizer, the share of the base inputs within 2^-17 relative of a rounding boundary is within 0.1 %; every
    numel of the GPU file is a prefix of the periodic continuation of that base, the largest one 2042 whole periods and 13 elements."""
    in_q, mid_q, out_q = C.act_grids(act, mid_on, in_on)
    r = O.prefill_act(C.act_base(), act, in_q, mid_q, out_q)
    for name, t in (("mid", r["t_mid"]), ("out", r["t_act"])):
        if t is None:
            continue
        with np.errstate(invalid="ignore"):
            near = O._tie_dist(t) <= 2.0 ** -17 * np.abs(t) + 1e-30
        print("act %d mid %d in %d: %s quantizer flags %d of %d (%.4f %%)" % (act, mid_on, in_on, name, near.sum(), near.size, 100 * near.mean()))
        assert near.mean() <= CAP, (name, near.mean())
        for n in C.ACT_NUMEL:
            assert np.resize(near, n).mean() <= CAP, (name, n)
    assert r["tie"].mean() <= 2 * CAP


@pytest.mark.parametrize("act", [0, 1])
def test_gated_observation_has_no_flagged_input(act):
    """The gated routes are held exactly GIVEN mq_act_quant's value at the 256 values of w1's grid, and that launch is itself held to
    the oracle only where `tie` is clear.  256 inputs: the 0.1 % cap per quantizer means none may be flagged, so that every one of the 256
    observed values -- every row of the table, every element of every route -- is the oracle's bit for bit.  Realised: 0 of 256, both
    activations."""
    va256, grids, _ = C.gated_observation(act)
    r = O.prefill_act(va256, act, *grids)
    for name, t in (("mid", r["t_mid"]), ("out", r["t_act"])):
        if t is not None:
            near = O._tie_dist(t) <= 2.0 ** -17 * np.abs(t) + 1e-30
            print("gated observation, act %d: %s quantizer flags %d of 256" % (act, name, near.sum()))
            assert near.mean() <= CAP, (name, np.nonzero(near)[0])
    assert not r["tie"].any()
