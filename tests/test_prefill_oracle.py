"""CPU: the prefill attention row oracle (oracle.prefill_attention_rows) is attention_sim(..., exact_int=True) row for row, bit for bit,
and its error envelope (oracle.prefill_envelope) holds both the fp32 oracle and the float64 result while staying narrow on ordinary
data."""
import numpy as np
import pytest

from oracle import mq_oracle as O

F32 = np.float32


def _grid(bits, lo, hi):
    g = O.QuantizerOracle(bitwidth=bits)
    g.set_from_minmax(F32(lo), F32(hi))
    return g


def _rope(S, rot):
    inv = 1.0 / (10000.0 ** (np.arange(0, rot, 2, dtype=F32) / rot))
    ang = np.outer(np.arange(S, dtype=F32), inv).astype(F32)
    ang = np.concatenate((ang, ang), -1)
    return np.cos(ang).astype(F32), np.sin(ang).astype(F32)


def _out_index_of_p(r, p_idx, pv):
    """Output indices [R, heads*D] that a given set of probability indices leads to (division form)."""
    pa, pb, po = pv
    H, R, S = p_idx.shape
    acc = O.decode_pv_sums(p_idx.reshape(H * R, S), r["iv"], pa, pb).reshape(H, R, -1)
    pre = (acc.astype(np.float64) * np.float64(F32(F32(pa.scale) * F32(pb.scale)))).astype(F32)
    out = O._index(pre, po) if po is not None else pre
    return out.transpose(1, 0, 2).reshape(R, -1)


CASES = [  # D, H, KV, rot, qk_out bits, pv_a (bits, lo, hi), pv_out bits
    (64, 4, 4, 64, 16, (16, 0.0, 1.0), 8),          # MHA, production shape
    (64, 4, 2, 16, 16, (16, -0.25, 1.0), 8),        # GQA, StableLM-2 rotary, probability zero point != 0
    (64, 4, 1, 32, 16, (12, 0.0, 0.5), 8),          # MQA, rot_dim 32, a probability grid that cuts [0, 1] (the clamp)
    (64, 2, 1, 64, 0, (8, -0.1, 1.0), 8),           # no score grid, 8-bit probabilities with a zero point
    (128, 4, 2, 128, 16, (16, 0.0, 1.0), 0),        # no output grid
    (128, 2, 2, 128, 0, (16, -0.5, 1.0), 8),
    (256, 4, 1, 256, 16, (16, 0.0, 1.0), 8),
    (256, 2, 1, 256, 0, (12, -0.05, 1.0), 0),
]


@pytest.mark.parametrize("D,H,KV,rot,qk_bits,pa,po_bits", CASES)
@pytest.mark.parametrize("index_inputs", [False, True])
def test_prefill_rows_are_attention_sim_rows(D, H, KV, rot, qk_bits, pa, po_bits, index_inputs):
    rng = np.random.default_rng(D + H + KV + rot + qk_bits + po_bits + int(index_inputs))
    S = 150
    q, k, v = (rng.standard_normal((S, n * D), dtype=F32) * F32(1.5) for n in (H, KV, KV))
    k[40] = np.tile(q[40, :D], KV)                          # one score that stands out
    cos, sin = _rope(S, rot)
    qk = (_grid(8, -4.0, 4.0), _grid(8, -4.5, 4.5), _grid(qk_bits, -40.0, 40.0) if qk_bits else None)
    pv = (_grid(*pa), _grid(8, -4.0, 4.0), _grid(po_bits, -1.5, 1.5) if po_bits else None)
    kw = {}
    if index_inputs:                                        # the fused q|k|v GEMM's uint8 indices, three input grids
        ins = (_grid(8, -4.0, 4.0), _grid(8, -3.5, 5.0), _grid(8, -3.0, 3.0))
        idx = rng.integers(0, 256, (S, (H + 2 * KV) * D)).astype(np.uint8)
        seg = idx.reshape(S, H + 2 * KV, D).astype(F32)
        q, k, v = (O.dequantize_index(seg[:, a:b], g.scale, g.offset).reshape(S, -1)
                   for (a, b), g in zip(((0, H), (H, H + KV), (H + KV, H + 2 * KV)), ins))
        kw = dict(qkv_idx=idx, in_grids=ins)
    want = O.attention_sim(q, k, v, cos, sin, H, KV, qk, pv, exact_int=True)
    rows = np.array([0, 1, 39, 40, 41, 63, 64, 65, 127, 128, S - 1])
    r = O.prefill_attention_rows(None if index_inputs else q, None if index_inputs else k, None if index_inputs else v,
                                 cos, sin, H, KV, qk, pv, rows, **kw)
    assert np.array_equal(r["y"], want[rows])
    # K / V images: the indices of the RoPE'd keys and of the values
    kr = O.rope_partial(k.reshape(S, KV, D).transpose(1, 0, 2), cos, sin)
    assert np.array_equal(r["ik8"].astype(np.int64) + 128, O._index(kr, qk[1]))
    assert np.array_equal(r["iv8"].astype(np.int64) + 128, O._index(v.reshape(S, KV, D).transpose(1, 0, 2), pv[1]))
    # the envelope holds the fp32 oracle and the float64 softmax's result
    env = O.prefill_envelope(r, qk, pv)
    got32 = r["out_idx"] if pv[2] is not None else r["y"]
    got64 = _out_index_of_p(r, r["p_idx64"], pv)
    for name, got in (("fp32", got32), ("float64", got64)):
        bad = (got < env["lo"]) | (got > env["hi"])
        assert not bad.any(), (name, int(bad.sum()))
    assert ((r["p_idx"] >= env["p_lo"]) & (r["p_idx"] <= env["p_hi"])).all()
    assert ((r["p_idx64"] >= env["p_lo"]) & (r["p_idx64"] <= env["p_hi"])).all()
    # a masked key contributes exactly the zero point
    assert (r["p_idx"][~np.broadcast_to(r["live"], r["p_idx"].shape)] == int(pv[0].offset)).all()


@pytest.mark.parametrize("D,qk_bits,pa_bits,S", [(64, 16, 16, 1000), (128, 16, 12, 700), (256, 0, 16, 700), (64, 16, 8, 1000)])
def test_prefill_envelope_is_narrow_on_ordinary_data(D, qk_bits, pa_bits, S):
    """Random data: at most a few probability indices per row are ambiguous and an output index range spans at most three steps
    (two where both ends of the sum land in one grid cell), most of them one."""
    rng = np.random.default_rng(S + D + pa_bits)
    H, KV = 2, 1
    q, k, v = (rng.standard_normal((S, n * D), dtype=F32) * F32(1.5) for n in (H, KV, KV))
    cos, sin = _rope(S, D)
    qk = (_grid(8, -4.0, 4.0), _grid(8, -4.5, 4.5), _grid(qk_bits, -40.0, 40.0) if qk_bits else None)
    pv = (_grid(pa_bits, 0.0, 1.0), _grid(8, -4.0, 4.0), _grid(8, -1.5, 1.5))
    rows = np.array([0, 63, 64, 200, S - 1])
    r = O.prefill_attention_rows(q, k, v, cos, sin, H, KV, qk, pv, rows)
    env = O.prefill_envelope(r, qk, pv)
    width = env["hi"] - env["lo"]
    n_live = int(np.broadcast_to(r["live"], r["p_idx"].shape).sum())
    print(f"D={D} S={S}: width max {width.max()}, mean {width.mean():.3f}; {env['n_amb_p']} of {n_live} p indices ambiguous, "
          f"{env['n_amb_score']} score indices")
    assert width.max() <= 2 and width.mean() <= 0.5
    assert env["n_amb_p"] <= 0.02 * n_live


def test_prefill_fixed_ref_follows_the_grid_span():
    assert O.prefill_fixed_ref(_grid(16, -40.0, 40.0), 64)
    assert not O.prefill_fixed_ref(_grid(16, -2000.0, 2000.0), 64)
    assert not O.prefill_fixed_ref(None, 64)
