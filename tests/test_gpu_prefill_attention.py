"""GPU: the prefill attention (mq_attention_quant through ops.attention_quant) against the exact row oracle
(oracle.prefill_attention_rows: rows of attention_sim(exact_int=True)) up to the 65 536-token limit.

Every core-kernel instantiation the production library builds runs at S >= 8 192, the production one at S = 65 536; structured fills
run at S = 2 048 / 2 000.  Rows checked per run: every row of the first and last query blocks and of the blocks around the points where
the parked / recomputed mix of exponentials changes (3 / 10 key blocks in the f16 form, 5 / 10 in the deep int8 form, 3 with the small
cache), rows on both sides of 64-row boundaries, the last real row and a seeded sample.  What must hold, with no exception:
  1. every output index lies in oracle.prefill_envelope's range (derived from the kernel's rounding points; v_exp_f32 assumed within
     oracle.EXP2_ULP ulp -- unmeasured);
  2. every output index is within one step of the fp32 oracle (the number that differ is printed);
  3. the int8 image holds the fp32 output's index - 128, its row sums are exact, and no row outside this sequence's changes;
  4. after each chunk of a cache continuation the K / V cache images are the oracle's, byte for byte (include/mobilequant_amd.h)."""
import contextlib
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import mq_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
SENT = 77                                    # sentinel byte of the int8 image / row sums


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    import mobilequant_amd._lib as L
    assert L.device_info()["arch"].startswith("gfx950")
    return torch.device("cuda:0")


@contextlib.contextmanager
def _knobs(f16=1, fused_q=1, cache=0):
    from mobilequant_amd import _lib
    L = _lib.load()
    try:
        L.mq_attention_set_f16(f16)
        L.mq_attention_set_fused_q(fused_q)
        L.mq_attention_set_cache(cache)
        yield
    finally:
        L.mq_attention_set_f16(1)
        L.mq_attention_set_fused_q(1)
        L.mq_attention_set_cache(0)


def _g(bits, lo, hi):
    g = O.QuantizerOracle(bitwidth=bits)
    g.set_from_minmax(F32(lo), F32(hi))
    return g


def _gt(o, dev):
    return None if o is None else (torch.tensor([float(o.scale)], device=dev), torch.tensor([float(o.offset)], device=dev),
                                   float(o.qmin), float(o.qmax))


def _rope(S, rot, identity=False):
    if identity:
        return np.ones((S, rot), F32), np.zeros((S, rot), F32)
    inv = 1.0 / (10000.0 ** (np.arange(0, rot, 2, dtype=F32) / rot))
    ang = np.outer(np.arange(S, dtype=F32), inv).astype(F32)
    ang = np.concatenate((ang, ang), -1)
    return np.cos(ang).astype(F32), np.sin(ang).astype(F32)


@dataclasses.dataclass
class Case:
    D: int = 64
    H: int = 2
    KV: int = 1
    S: int = 2048
    rot: int = 0                  # 0: D
    fill: str = "random"
    qk_out: tuple = (16, -60.0, 60.0)   # None: no score grid
    pv_a: tuple = (16, 0.0, 1.0)
    pv_out: tuple = (8, -1.5, 1.5)      # None: no output grid
    knobs: tuple = (1, 1, 0)            # f16, fused_q, cache
    idx_inputs: bool = False
    seed: int = 0

    def grids(self):
        if self.fill == "offgrid":            # q / k offsets far outside [-256, 511]: ti >= 2^24 (int -> float rounds)
            qk = (_g(8, 5.0, 6.0), _g(8, 4.9, 6.1), _g(16, 1000.0, 2600.0))
        else:
            qk = (_g(8, -6.0, 6.0), _g(8, -6.5, 6.5), _g(*self.qk_out) if self.qk_out else None)
        pv = (_g(*self.pv_a), _g(8, -4.0, 4.0), _g(*self.pv_out) if self.pv_out else None)
        return qk, pv

    def inputs(self):
        """q [S, H*D], k / v [S, KV*D] fp32, cos / sin [S, rot]; or the same from uint8 indices (then also (idx, in_grids))."""
        S, H, KV, D = self.S, self.H, self.KV, self.D
        rng = np.random.default_rng(self.seed)
        rot = self.rot or D
        q, k, v = (rng.standard_normal((S, n * D), dtype=F32) * F32(1.5) for n in (H, KV, KV))
        cos, sin = _rope(S, rot, identity=self.fill == "offgrid")
        f = self.fill
        if f == "flat":
            k[:] = k[:1]
        elif f.startswith("hot"):
            k *= F32(0.1)
            at = {"hot0": [0], "hotmid": [S // 2], "hotdiag": list(range(0, S, 97))}[f]
            k[at] = q[at, :KV * D] * F32(3.0)              # on the diagonal: each hot key is its own row's query
        elif f == "saturate":
            q *= F32(3.0)
            k *= F32(3.0)
        elif f == "v_zero":
            v[:] = 0
        elif f in ("v_max", "zp_sat"):
            v[:] = np.where(rng.integers(0, 2, v.shape) > 0, F32(9.0), F32(-9.0)) if f == "v_max" else F32(-9.0)
        elif f == "offgrid":
            q = F32(5.5) + q * F32(0.2)
            k = F32(5.5) + k * F32(0.2)
        idx = None
        if self.idx_inputs:
            ins = (_g(8, -5.0, 5.0), _g(8, -4.5, 5.5), _g(8, -3.0, 3.0))
            idx = rng.integers(0, 256, (S, (H + 2 * KV) * D)).astype(np.uint8)
            seg = idx.reshape(S, H + 2 * KV, D).astype(F32)
            q, k, v = (O.dequantize_index(seg[:, a:b], g.scale, g.offset).reshape(S, -1)
                       for (a, b), g in zip(((0, H), (H, H + KV), (H + KV, H + 2 * KV)), ins))
            idx = (idx, ins)
        return q, k, v, cos, sin, idx


def _rows(S_real, seed, lo=0):
    """Query rows to check in [lo, S_real): whole blocks where the exponential cache mix changes, first / last blocks, boundaries."""
    nb = (S_real - lo + 63) // 64
    blocks = {0, 1, 2, 3, 4, 8, 9, nb - 1}
    rows = {lo + 64 * b + i for b in blocks if b < nb for i in range(64)}
    rows |= {lo + 64 * m + d for m in np.linspace(1, nb - 1, 12).astype(int) for d in (-1, 0)}
    rows |= {S_real - 1} | set(np.random.default_rng(seed).integers(lo, S_real, 32).tolist())
    return np.array(sorted(r for r in rows if lo <= r < S_real))


def _oracle_check(case, qk, pv, inp, got, rows, tally, what):
    """Checks 1 and 2 for the given absolute rows; got [S_real, H*D] fp32 kernel output (rows indexed absolutely)."""
    q, k, v, cos, sin, idx = inp
    n_diff = n_amb = width = 0
    for c0 in range(0, len(rows), 16):
        rr = rows[c0:c0 + 16]
        kw = dict(qkv_idx=idx[0], in_grids=idx[1]) if idx is not None else {}
        r = O.prefill_attention_rows(None if idx else q, None if idx else k, None if idx else v, cos, sin, case.H, case.KV, qk, pv, rr, **kw)
        env = O.prefill_envelope(r, qk, pv)
        g = got[rr].astype(np.float64)
        if pv[2] is not None:
            g = np.rint(g / np.float64(F32(pv[2].scale))) + np.float64(F32(pv[2].offset))
            ref = r["out_idx"].astype(np.float64)
            assert np.abs(g - ref).max() <= 1, (what, float(np.abs(g - ref).max()))
            n_diff += int((g != ref).sum())
            width = max(width, float((env["hi"] - env["lo"]).max()))
        else:
            ref = r["y"].astype(np.float64)
            n_diff += int((g != ref).sum())
        bad = (g < env["lo"]) | (g > env["hi"])
        assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4], g[bad][:4], env["lo"][bad][:4], env["hi"][bad][:4])
        n_amb += env["n_amb_p"]
    tally.append((what, n_diff, n_amb, width))
    print(f"{what}: {len(rows)} rows, {n_diff} outputs off the fp32 oracle, {n_amb} ambiguous p indices, envelope width <= {width}")


def _untile(img, rows, K):
    """Fragment-blocked [ceil16(rows), K] image -> row-major (byte 16 ((row & 15) + 16 ((k & 63) >> 4)) + (k & 15) of 1-KiB block
    (row >> 4, k >> 6))."""
    R16 = img.shape[0]
    t = img.reshape(R16 // 16, K // 64, 4, 16, 16).transpose(0, 3, 1, 2, 4)
    return t.reshape(R16, K)[:rows]


def _image_check(case, pv, out, img, rs, row0, S_real, tiled, what):
    """Check 3: the sequence's image rows are the output's indices - 128, exact row sums, every other row untouched."""
    K = case.H * case.D
    im = img.cpu().numpy()
    im = _untile(im, im.shape[0], K) if tiled else im
    want = (np.rint(out.astype(np.float64) / np.float64(F32(pv[2].scale))) + np.float64(F32(pv[2].offset)) - 128).astype(np.int64)
    assert np.array_equal(im[row0:row0 + S_real].astype(np.int64), want), what
    assert (im[:row0] == SENT).all() and (im[row0 + S_real:] == SENT).all(), what
    r = rs.cpu().numpy()
    assert np.array_equal(r[row0:row0 + S_real], want.sum(1)), what
    assert (r[:row0] == SENT).all() and (r[row0 + S_real:] == SENT).all(), what


def _launch(case, qk, pv, inp, dev, row0=5, tiled=False, **kw):
    from mobilequant_amd import ops
    q, k, v, cos, sin, idx = inp
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)                 # noqa: E731
    grids = dict(zip(("qk_a", "qk_b", "qk_out", "pv_a", "pv_b", "pv_out"), (_gt(o, dev) for o in (*qk, *pv))))
    S = q.shape[0]
    image = None
    if pv[2] is not None:
        rows = row0 + S + 40
        img = torch.full(((rows + 15) // 16 * 16 if tiled else rows, case.H * case.D), SENT, dtype=torch.int8, device=dev)
        rs = torch.full((rows,), SENT, dtype=torch.int32, device=dev)
        image = (img, rs, row0, 128, tiled)
    qkv = None
    if idx is not None:
        qkv = (t(idx[0]), tuple((torch.tensor([float(g.scale)], device=dev), torch.tensor([float(g.offset)], device=dev)) for g in idx[1]))
    with _knobs(*case.knobs):
        out = ops.attention_quant(None if idx else t(q), None if idx else t(k), None if idx else t(v), t(cos), t(sin), case.H, case.KV,
                                  grids, image=image, want_out=True, qkv_idx=qkv, head_dim=case.D, **kw)
        torch.cuda.synchronize()
    return out.cpu().numpy(), image


def _run(case, dev, tally, S_real=None, tiled=False):
    qk, pv = case.grids()
    inp = case.inputs()
    if S_real is not None:                                                          # ragged: the first S_real positions
        inp = tuple(a[:S_real] for a in inp[:5]) + ((inp[5][0][:S_real], inp[5][1]) if inp[5] is not None else None,)
    S_real = inp[0].shape[0]
    out, image = _launch(case, qk, pv, inp, dev, tiled=tiled)
    assert out.shape == (S_real, case.H * case.D) and np.isfinite(out).all(), case
    what = f"D={case.D} H={case.H}/{case.KV} S={S_real} rot={case.rot or case.D} {case.fill} knobs={case.knobs} qk_out={case.qk_out} " \
           f"pv_a={case.pv_a} pv_out={case.pv_out}{' idx' if case.idx_inputs else ''}"
    if image is not None:
        _image_check(case, pv, out, image[0], image[1], image[2], S_real, tiled, what)
    _oracle_check(case, qk, pv, inp, out, _rows(S_real, case.seed), tally, what)


# every core-kernel instantiation of the production library (attention_quant_kernel<D, QK_OUT, BIG, QPREP, F16>), with the score grid
# that keeps the grid top as exponent reference and with one wide enough to need the running maximum
INSTANTIATIONS = {
    "64,T,T,T,T": dict(D=64),
    "64,T,T,F,T": dict(D=64, rot=32, H=4, KV=2),
    "64,T,T,T": dict(D=64, knobs=(0, 1, 0), H=4, KV=4),
    "64,T,T": dict(D=64, rot=32, knobs=(0, 1, 0)),
    "64,T": dict(D=64, knobs=(1, 1, 1), H=4, KV=2),
    "64,F": dict(D=64, qk_out=None, H=2, KV=2),
    "128,T": dict(D=128),
    "128,F": dict(D=128, qk_out=None, H=2, KV=2),
    "256,T": dict(D=256, H=4, KV=1),
    "256,F": dict(D=256, qk_out=None),
}
WIDE = (16, -3000.0, 3000.0)          # (qmax - qmin) cexp > 96: no fixed reference


@pytest.mark.parametrize("inst", list(INSTANTIATIONS))
def test_every_instantiation_against_the_row_oracle_at_8192(dev, inst):
    tally = []
    kw = INSTANTIATIONS[inst]
    _run(Case(S=8192, seed=11, **kw), dev, tally)
    if kw.get("qk_out", 1) is not None:
        assert O.prefill_fixed_ref(Case(**kw).grids()[0][2], kw["D"]) and not O.prefill_fixed_ref(_g(*WIDE), kw["D"])
        _run(Case(S=2048, seed=12, **dict(kw, qk_out=WIDE)), dev, tally)
    _run(Case(S=2048, seed=13, idx_inputs=True, **kw), dev, tally, S_real=2000, tiled=True)


FILLS = ("flat", "hot0", "hotmid", "hotdiag", "saturate", "v_zero", "v_max", "offgrid")


@pytest.mark.parametrize("D", [64, 256])
def test_structured_fills_and_grids(dev, D):
    tally = []
    for i, fill in enumerate(FILLS):
        _run(Case(D=D, S=2048, fill=fill, seed=20 + i), dev, tally)
    for i, extra in enumerate((dict(pv_a=(16, -0.25, 1.0)), dict(pv_a=(16, 0.0, 0.4)), dict(pv_a=(12, 0.0, 1.0)), dict(pv_a=(8, -0.1, 1.0)),
                               dict(pv_out=None), dict(qk_out=None, pv_a=(12, -0.05, 1.0)), dict(pv_out=(8, -0.3, 0.2)))):
        _run(Case(D=D, S=2048, seed=40 + i, **extra), dev, tally, S_real=2000 if i % 2 else None, tiled=bool(i % 2))
    _run(Case(D=D, S=64, seed=50), dev, tally)
    _run(Case(D=D, S=128, seed=51), dev, tally, S_real=65)


def test_production_at_the_65536_limit(dev):
    """The production instantiation at seq = 65 536, random, and with every probability index near the top of its grid (zero point
    65 534) against values at their minimum: acc_hi / acc_lo near -2^30, acc_v / psum / v_prefix at their largest."""
    tally = []
    _run(Case(S=65536, seed=60), dev, tally)
    _run(Case(S=65536, seed=61, fill="zp_sat", pv_a=(16, -1.0, 1e-5), pv_out=(8, -8.0, 8.0)), dev, tally)
    _run(Case(D=256, S=16384, seed=62, fill="zp_sat", pv_a=(16, -1.0, 1e-5), pv_out=(8, -8.0, 8.0)), dev, tally)


def test_batch_runs_every_sequence_as_alone(dev):
    from mobilequant_amd import ops
    tally = []
    for D in (64, 128):
        case = Case(D=D, S=1000, seed=70)
        qk, pv = case.grids()
        seqs = [Case(D=D, S=1000, seed=70 + b).inputs() for b in range(3)]
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)            # noqa: E731
        grids = dict(zip(("qk_a", "qk_b", "qk_out", "pv_a", "pv_b", "pv_out"), (_gt(o, dev) for o in (*qk, *pv))))
        cos, sin = seqs[0][3], seqs[0][4]
        img = torch.full((3 * 1000 + 16, case.H * D), SENT, dtype=torch.int8, device=dev)
        rs = torch.full((3 * 1000 + 16,), SENT, dtype=torch.int32, device=dev)
        out = ops.attention_quant(*(t(np.stack([s[i] for s in seqs])) for i in range(3)), t(cos), t(sin), case.H, case.KV, grids,
                                  image=(img, rs, 16, 128, False), want_out=True, head_dim=D).cpu().numpy()
        for b in range(3):
            sub = img[16 + 1000 * b:16 + 1000 * (b + 1)].cpu().numpy().astype(np.int64)
            want = (np.rint(out[b].astype(np.float64) / np.float64(F32(pv[2].scale))) + np.float64(F32(pv[2].offset)) - 128)
            assert np.array_equal(sub, want) and np.array_equal(rs[16 + 1000 * b:16 + 1000 * (b + 1)].cpu().numpy(), want.sum(1))
            _oracle_check(case, qk, pv, seqs[b], out[b], _rows(1000, b), tally, f"batch D={D} b={b}")
        assert (img[:16].cpu().numpy() == SENT).all() and (img[3016:].cpu().numpy() == SENT).all()


def _cache_check(cache, r_full, qk, case, upto, f16):
    """Check 4: the cache images of positions 0 .. upto - 1 (layout: include/mobilequant_amd.h)."""
    KV, D = case.KV, case.D
    rows = cache["rows"]
    ik8, iv8 = r_full["ik8"][:, :upto].astype(np.int64), r_full["iv8"][:, :upto].astype(np.int64)
    k = cache["k_i8"].view(KV, rows, D)[:, :upto].cpu().numpy().astype(np.int64)
    assert np.array_equal(k, ik8)
    zq = int(qk[0].offset) - 128
    assert np.array_equal(cache["k_rs"].view(KV, rows)[:, :upto].cpu().numpy().astype(np.int64), -zq * ik8.sum(-1))
    nb = upto // 64
    vt = cache["vt_i8"].view(KV, rows // 64, D, 4, 4, 4)[:, :nb].cpu().numpy().astype(np.int64)   # [.., d, tq, j, e]
    vt = vt.transpose(0, 1, 4, 3, 5, 2).reshape(KV, nb * 64, D)                                      # key t = 16 j + 4 tq + e
    assert np.array_equal(vt, iv8[:, :nb * 64])
    if D == 64 and f16:
        h = cache["k_f16"].view(KV, rows // 64, 4, 2, 4, 16, 8)[:, :nb].cpu().numpy()  # [.., r / 16, (d % 16) / 8, d / 16, r % 16, d % 8]
        h = h.transpose(0, 1, 2, 5, 4, 3, 6).reshape(KV, nb * 64, D).astype(np.float64)
        assert np.array_equal(h, ik8[:, :nb * 64] + 128 - float(qk[1].offset))
    if D != 64:
        vp = cache["v_pre"].view(KV, rows // 64, D)[:, :nb].cpu().numpy().astype(np.int64)
        assert np.array_equal(vp, np.cumsum(iv8[:, :nb * 64].reshape(KV, nb, 64, D).sum(2), axis=1))


@pytest.mark.parametrize("D,knobs,chunks", [(64, (1, 1, 0), (1024, 4096, 3000)), (64, (0, 1, 0), (64, 2048, 130)),
                                             (64, (1, 1, 1), (128, 1000)), (256, (1, 1, 0), (2048, 2048, 3333)), (128, (1, 1, 0), (4096, 77))])
def test_cache_continuation_in_chunks(dev, D, knobs, chunks):
    """Chunked prefill into a caller-owned image cache: after every chunk the cache images are the oracle's and the chunk's rows
    are checked against the oracle of the whole sequence; the last chunk is ragged."""
    from mobilequant_amd import ops
    tally = []
    S = sum(chunks)
    case = Case(D=D, S=S, knobs=knobs, seed=80 + D)
    qk, pv = case.grids()
    inp = case.inputs()
    cache = ops.attention_image_cache(case.KV, D, (S + 63) // 64 * 64, dev)
    r_full = O.prefill_attention_rows(*inp[:5], case.H, case.KV, qk, pv, np.array([0]))
    pos = 0
    for n in chunks:
        sl = tuple(a[pos:pos + n] for a in inp[:5]) + (None,)
        out, image = _launch(case, qk, pv, sl, dev, cache=cache, pos0=pos)
        _image_check(case, pv, out, image[0], image[1], image[2], n, False, f"chunk at {pos}")
        _cache_check(cache, r_full, qk, case, pos + n // 64 * 64, f16=knobs[0] == 1 and knobs[2] == 0)
        got = np.zeros((pos + n, case.H * D), F32)
        got[pos:] = out
        _oracle_check(case, qk, pv, inp, got, _rows(pos + n, pos, lo=pos), tally, f"D={D} knobs={knobs} chunk {pos}..{pos + n}")
        pos += n


def test_fused_layer_with_q_k_offsets_outside_the_f16_window_matches_the_module_chain(dev):
    """q / k grids of a narrow range away from zero (offsets < -256): the f16 score contraction cannot hold them, so the fused layer
    must take the int8 contraction.  Logits equal the module chain's within test_gpu_decode_long's bars."""
    from test_gpu_decode_long import _model
    from mobilequant_amd import llama, ops
    m = _model(dev, 64)
    at = m.layers[0].self_attn
    at.pv_bmm.input_quantizer.qcfg.bitwidth = 16
    at.pv_bmm.input_quantizer.set_scale_offset_from_minmax(torch.tensor(0.0), torch.tensor(1.0), "buffer", dev)
    for q in (at.qk_bmm.input_quantizer, at.qk_bmm.input2_quantizer):
        q.set_scale_offset_from_minmax(torch.tensor(0.3), torch.tensor(0.5), "buffer", dev)      # offset -382
        assert not ops.attention_f16_offsets_ok(float(q.offset))
    ids = torch.randint(0, m.shape.vocab, (1, 256), generator=torch.Generator().manual_seed(5)).to(dev)
    with torch.no_grad():
        want = m(ids)[0].float().cpu().numpy()
        assert llama.fuse_decoder_layer(m) == 1
        got = m(ids)[0].float().cpu().numpy()
    assert np.isfinite(got).all()
    d = np.abs(got - want) / float(np.ptp(want))
    assert d.max() <= 0.02 and np.quantile(d, 0.99) <= 0.006 and np.median(d) <= 5e-6, (d.max(), np.quantile(d, 0.99), np.median(d))
