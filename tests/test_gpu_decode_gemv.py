"""GPU: the decode step's weight-streaming launches -- mq_decode_gemv (all 16 instantiations), mq_decode_head and mq_decode_embed -- each
run on its own against an exact oracle (oracle.decode_gemv_* / decode_head_*), at real model shapes and at the C entries' limits.

mq_decode_gemv.  The int8 image a launch contracts comes from an fp32 norm whose reduction order the oracle does not replay, so it is
OBSERVED: a probe launch with the same prologue fields streams identity rows (alpha 1, zp 0, ct 0, output grid off), so that y[i] is
image element ks[i], and one zero row with w_zp = -1, whose y is the row sum.  Non-gate launches also carry identity rows of their own
behind their real rows (a last segment, output grid off: the last workgroup), which must agree with the probe (whose rows spread over
all workgroups, the first included).  The prologue runs the same arithmetic whatever the stream does, and an OPRE launch's norm is a
plain NORM / LNORM prologue on its own x_mid (XPRE 2 or 4 only changes how many float4 a thread may hold: for K <= 4096 the loops over
the extra slots are skipped as a whole).  Per case:
  1. the image is the float64 oracle's except where the pre-rounding value is within the fp32 bound of a tie, and by one step there;
  2. given that image, every y / gate_q / x_mid is the oracle's epilogue bit for bit (gate_q: except at flagged exp / erf near-ties);
  3. y / gate_q are within one step of the reference's division-form quantizers, y only at near-ties of the two forms, and equal on
     >= 99.9 % of all outputs of the module;
  4. nothing is written past the outputs; zero_acc clears exactly [0, zero_n); every x_mid element is written.
mq_decode_head: every logit within the derived fp32 bound of the float64 oracle, canary after V, argmax where the margin allows it.
mq_decode_embed: bit-exact gathers at the table's and the rope tables' ends."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import mq_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
CANARY_F, CANARY_I8, CANARY_I32 = -7777.0, 85, 7


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _call(name, *args):
    from mobilequant_amd import _lib
    _lib.call(name, *args)


class Grid:
    """A static per-tensor grid on the device and its oracle twin."""

    def __init__(self, dev, bits, lo, hi):
        self.o = O.QuantizerOracle(bitwidth=bits)
        self.o.set_from_minmax(F32(lo), F32(hi))
        self.s = torch.tensor([float(self.o.scale)], device=dev)
        self.off = torch.tensor([float(self.o.offset)], device=dev)

    @staticmethod
    def of(q, dev):
        """Oracle twin of a module quantizer (None when absent or bypassed), with the device tensors the module holds."""
        if q is None or q.bypassed():
            return None
        g = Grid.__new__(Grid)
        g.o = O.quantizer_oracle_from(float(q.scale.reshape(-1)[0]), float(q.offset.reshape(-1)[0]), q.qmin, q.qmax)
        g.s, g.off = q.scale.detach().float().reshape(1).to(dev).contiguous(), q.offset.detach().float().reshape(1).to(dev).contiguous()
        return g


def _mg(g):
    from mobilequant_amd._lib import MqGrid
    return MqGrid(None, None, 0.0, 0.0) if g is None else MqGrid(g.s.data_ptr(), g.off.data_ptr(), float(g.o.qmin), float(g.o.qmax))


def _oo(g):
    return None if g is None else g.o


def _t(a, dev, keep, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    if dtype is not None:
        t = t.to(dtype)
    keep.append(t)
    return t.data_ptr()


def _pack_consts(a, dev, keep):
    from mobilequant_amd._lib import MqGrid
    grids = [a.norm_in, a.a_grid, a.out_grid[0], a.out_grid[1], a.out_grid[2], a.gate_mid, a.gate_actout, a.gate_out, a.o_out]
    out = torch.zeros(64, device=dev)
    _call("mq_decode_pack_grids", (MqGrid * 9)(*grids), 9, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    keep.append(out)
    a.consts = out.data_ptr()


def _geometry(a):
    n, per, tot = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    _call("mq_decode_gemv_geometry", ctypes.byref(a), ctypes.byref(n), ctypes.byref(per), ctypes.byref(tot))
    row = (2 if a.gate_q else 1) * (a.K // 2 if a.w4 else a.K)
    return n.value, per.value // row


def _launch(a):
    _call("mq_decode_gemv", ctypes.byref(a), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


def _id_ks(K):
    """Image elements the identity rows observe: all of them up to K = 8192, else both ends and a spread in between."""
    if K <= 8192:
        return np.arange(K)
    return np.unique(np.concatenate([np.arange(1024), np.arange(K - 1024, K), np.arange(1024, K - 1024, 61)]))


def _id_rows(K, ks, w4):
    """Identity rows for ks plus the row-sum row (all-zero weights, w_zp = -1): bytes, alpha, w_zp, col_term."""
    n = len(ks) + 1
    wb = np.zeros((n, K), np.int64)
    wb[np.arange(len(ks)), ks] = 1
    w = O.pack_w4(wb, 0) if w4 else wb.astype(np.int8)
    zp = np.zeros(n, np.int32)
    zp[-1] = -1
    return w, np.ones(n, F32), zp, np.zeros(n, np.int32)


def _prologue_fields(p, dev, keep, a):
    """Set the prologue fields of a (mq_decode_gemv_args) from the case dict p."""
    if p.get("xq") is not None:
        a.xq = _t(p["xq"], dev, keep)
    else:
        a.x = _t(p["x"], dev, keep)
    if p.get("norm_w") is not None:
        a.norm_w = _t(p["norm_w"], dev, keep)
        a.layernorm = int(p.get("layernorm", 0))
        if p.get("norm_bias") is not None:
            a.norm_bias = _t(p["norm_bias"], dev, keep)
    a.norm_in, a.eps, a.a_grid = _mg(p.get("norm_in")), float(p.get("eps", 1e-5)), _mg(p["a_grid"])


def _probe(p, K, dev, x=None):
    """(image [len(ks)] int8 at ks, rs) as a plain launch with p's prologue sees it; x replaces the fp32 row (an OPRE launch's x_mid)."""
    from mobilequant_amd._lib import MqDecodeGemvArgs
    keep = []
    ks = _id_ks(K)
    w, al, zp, ct = _id_rows(K, ks, False)
    a = MqDecodeGemvArgs()
    q = dict(p)
    if x is not None:
        q["x"] = x
    _prologue_fields(q, dev, keep, a)
    a.K, a.N = K, len(ks) + 1
    a.w, a.alpha, a.w_zp, a.col_term = _t(w, dev, keep), _t(al, dev, keep), _t(zp, dev, keep), _t(ct, dev, keep)
    a.seg_end[0] = a.seg_end[1] = a.N
    y = torch.full((a.N + 64,), CANARY_F, device=dev)
    a.y = y.data_ptr()
    _pack_consts(a, dev, keep)
    _launch(a)
    yh = y.cpu().numpy()
    assert np.all(yh[a.N:] == CANARY_F)
    img = yh[:len(ks)]
    assert np.all(img == np.rint(img)) and np.abs(img).max() <= 128
    return ks, img.astype(np.int64).astype(np.int8), int(yh[len(ks)])


def _check_image(tag, pro, ks, img, rs, K, xq=None):
    """Assert 1 (the observed image against the oracle's); returns the full image to drive the epilogue with."""
    if xq is not None:
        assert np.array_equal(img, np.asarray(xq)[ks]) and rs == int(np.asarray(xq, np.int64).sum()), tag
        return np.asarray(xq, np.int8)
    assert len(ks) == K
    want, tie = pro["image"], pro["tie"]
    d = np.abs(img.astype(np.int64) - want.astype(np.int64))
    assert np.all(d[~tie] == 0), (tag, int((d[~tie] > 0).sum()), np.nonzero(d * ~tie)[0][:8])
    assert d.max() <= 1, tag
    assert rs == int(img.astype(np.int64).sum()), tag
    print(f"[image] {tag}: {int(tie.sum())} near-tie elements, {int((d > 0).sum())} differ by one")
    _check_image.diffs += int((d > 0).sum())
    return img


_check_image.diffs = 0


def _check_div(tag, y, y_div, lsb, t):
    """3: y within one step of the division form; they may differ only where t = e / s, the division form's pre-rounding value, lies
    within 4 u |t| of a tie (fl(e fl(1 / s)) and fl(e / s) are both within 2 u |t| of e / s).  The share of exact rows is printed, and
    the whole module's share must reach 99.9 % (test_zz_report_counts)."""
    d = np.abs(y.astype(np.float64) - y_div.astype(np.float64))
    tol = lsb * (1 + 1e-5) + 4 * np.spacing(np.abs(y_div)).astype(np.float64)
    assert np.all(d <= tol), (tag, float((d / tol).max()))
    near = O._tie_dist(t) <= 4 * O.U32 * np.abs(t) + 1e-30
    assert np.all((d == 0) | near), (tag, np.nonzero((d > 0) & ~near)[0][:8])
    _check_div.rows += d.size
    _check_div.diff += int((d > 0).sum())
    print(f"[div] {tag}: {int((d > 0).sum())} of {d.size} rows one step from the division form")


_check_div.rows = _check_div.diff = 0


def run_gemv_case(dev, tag, K, rows, pro, gate=False, w4=False, seg_end=None, out_grid=(None, None, None), resid=None,
                  gate_act=0, gate_mid=None, gate_actout=None, gate_out=None, opre=None, zero_n=0, embed_id=False, x_mid_k=None):
    """One launch of hand-built or engine-lowered fields: rows = (wb [N, K] int64 weight bytes (index - 128 or nibble), alpha, w_zp,
    col_term, bias or None); pro = prologue fields of the case (x / xq, norm_w, norm_bias, layernorm, norm_in, eps, a_grid: Grid);
    opre = dict(o_acc, o_alpha, o_ct, o_bias, o_out).  Returns a small dict of what was seen."""
    from mobilequant_amd._lib import MqDecodeGemvArgs
    keep = []
    wb, alpha, zp, ct, bias = rows
    N = wb.shape[0]
    NL = N // 2 if gate else N
    n_id = 0
    if embed_id:                                      # identity rows behind the real ones: a last segment with its grid off
        assert not gate and out_grid[2] is None and seg_end is not None and seg_end[1] == N
        ks_e = _id_ks(K)[:: max(1, K // 64)]
        w_i, al_i, zp_i, ct_i = _id_rows(K, ks_e, False)
        n_id = len(ks_e) + 1
        wb = np.concatenate([wb, w_i.astype(np.int64)])
        alpha, zp, ct = np.concatenate([alpha, al_i]), np.concatenate([zp, zp_i]), np.concatenate([ct, ct_i])
        bias = None if bias is None else np.concatenate([bias, np.zeros(n_id, F32)])
        resid = None if resid is None else np.concatenate([resid, np.zeros(n_id, F32)])
    Nt = N + n_id
    a = MqDecodeGemvArgs()
    p = {k: (v.o if isinstance(v, Grid) else v) for k, v in pro.items()}
    _prologue_fields(pro, dev, keep, a)
    a.K, a.N, a.w4 = K, Nt, int(w4)
    w_img = O.pack_w4(wb, 0).view(np.int8) if w4 else wb.astype(np.int8)
    a.w = _t(w_img, dev, keep)
    a.alpha, a.w_zp, a.col_term = _t(alpha.astype(F32), dev, keep), _t(zp.astype(np.int32), dev, keep), _t(ct.astype(np.int32), dev, keep)
    if bias is not None:
        a.bias = _t(bias.astype(F32), dev, keep)
    a.seg_end[0], a.seg_end[1] = seg_end if seg_end is not None else (Nt, Nt)
    for k in range(3):
        a.out_grid[k] = _mg(out_grid[k])
    if resid is not None:
        a.resid = _t(resid.astype(F32), dev, keep)
    ny = NL if gate else Nt
    y = torch.full((ny + 64,), CANARY_F, device=dev)
    a.y = y.data_ptr()
    gq = None
    if gate:
        gq = torch.full((NL + 64,), CANARY_I8, dtype=torch.int8, device=dev)
        a.gate_q, a.gate_act = gq.data_ptr(), gate_act
        a.gate_mid, a.gate_actout, a.gate_out = _mg(gate_mid), _mg(gate_actout), _mg(gate_out)
    za = None
    if zero_n:
        za = torch.full((zero_n + 64,), CANARY_I32, dtype=torch.int32, device=dev)
        a.zero_acc, a.zero_n = za.data_ptr(), zero_n
    xm = None
    if opre is not None:
        a.o_acc, a.o_alpha, a.o_ct = _t(opre["o_acc"].astype(np.int32), dev, keep), _t(opre["o_alpha"], dev, keep), _t(opre["o_ct"].astype(np.int32), dev, keep)
        if opre.get("o_bias") is not None:
            a.o_bias = _t(opre["o_bias"], dev, keep)
        a.o_out = _mg(opre.get("o_out"))
        xm = torch.full((K + 64,), float("nan"), device=dev)
        a.x_mid = xm.data_ptr()
    _pack_consts(a, dev, keep)
    wgs, rpw = _geometry(a)
    _launch(a)
    return _judge(tag, K, a, pro, p, dict(wb=wb, alpha=alpha, zp=zp, ct=ct, bias=bias, resid=resid, N=N, n_id=n_id, w4=w4, gate=gate,
                  seg_end=tuple(a.seg_end), out_grid=[_oo(g) for g in out_grid], gate_act=gate_act, gate_mid=_oo(gate_mid),
                  gate_actout=_oo(gate_actout), gate_out=_oo(gate_out), opre=opre, zero_n=zero_n, wgs=wgs, rpw=rpw),
                  y.cpu().numpy(), None if gq is None else gq.cpu().numpy(), None if za is None else za.cpu().numpy(),
                  None if xm is None else xm.cpu().numpy(), dev)


def _judge(tag, K, a, pro, p, c, y, gq, za, xm, dev):
    N, n_id, gate = c["N"], c["n_id"], c["gate"]
    NL = N // 2 if gate else N
    ny = NL if gate else N + n_id
    # canaries
    assert np.all(y[ny:] == CANARY_F), (tag, "y written past its end")
    if gate:
        assert np.all(gq[NL:] == CANARY_I8), (tag, "gate_q written past its end")
    if za is not None:
        assert np.all(za[:c["zero_n"]] == 0) and np.all(za[c["zero_n"]:] == CANARY_I32), (tag, "zero_acc")
    # the oracle's prologue (OPRE: x_mid first, bit for bit)
    opre = c["opre"]
    ofields = {}
    if opre is not None:
        ofields = dict(o_acc=opre["o_acc"], o_alpha=opre["o_alpha"], o_ct=opre["o_ct"], o_bias=opre.get("o_bias"), o_out=_oo(opre.get("o_out")))
    pro_o = O.decode_gemv_prologue(K, x=p.get("x"), xq=p.get("xq"), norm_w=p.get("norm_w"), norm_bias=p.get("norm_bias"),
                                   layernorm=p.get("layernorm", 0), norm_in=p.get("norm_in"), eps=p.get("eps", 1e-5), a_grid=p["a_grid"],
                                   **ofields)
    x_probe = None
    if opre is not None:
        assert not np.isnan(xm[:K]).any() and np.all(np.isnan(xm[K:])), (tag, "x_mid not written exactly over [0, K)")
        assert np.array_equal(xm[:K].view(np.uint32), pro_o["x_mid"].view(np.uint32)), (tag, "x_mid")
        x_probe = xm[:K].copy()
    ks, img, rs = _probe(pro, K, dev, x_probe)
    img = _check_image(tag, pro_o, ks, img, rs, K, p.get("xq"))
    rs = int(img.astype(np.int64).sum())
    wb = c["wb"]
    sums = np.rint(wb[:N].astype(np.float64) @ img.astype(np.float64)).astype(np.int64)
    ep = O.decode_gemv_epilogue(sums, rs, c["alpha"][:N], c["zp"][:N], c["ct"][:N], None if c["bias"] is None else c["bias"][:N],
                                (min(c["seg_end"][0], N), min(c["seg_end"][1], N)), c["out_grid"],
                                None if c["resid"] is None else c["resid"][:N], gate, c["gate_act"], c["gate_mid"], c["gate_actout"], c["gate_out"])
    tt_max = int(np.abs(ep["tt"].astype(np.int64)).max())
    if gate:
        dq = np.abs(gq[:NL].astype(np.int64) - ep["gate_q"].astype(np.int64))
        assert np.all(dq[~ep["tie"]] == 0), (tag, int((dq[~ep["tie"]] > 0).sum()), np.nonzero(dq * ~ep["tie"])[0][:8])
        assert dq.max() <= 1, tag
        nmis = int((dq > 0).sum())
        print(f"[gate] {tag}: {int(ep['tie'].sum())} flagged, {nmis} gate_q differ by one")
        run_gemv_case.gate_mismatch += nmis
        dd = np.abs(gq[:NL].astype(np.int64) - ep["gate_q_div"].astype(np.int64))
        assert dd.max() <= 1, (tag, int(dd.max()))
        _check_div.rows += dd.size
        _check_div.diff += int((dd > 0).sum())
        fine = ~ep["tie"]
        assert c.get("skip_y") or np.array_equal(y[:NL][fine].view(np.uint32), ep["prod"][fine].view(np.uint32)), (tag, "y (gate product)")
    else:
        assert np.array_equal(y[:N].view(np.uint32), ep["y"].view(np.uint32)), (tag, np.nonzero(y[:N] != ep["y"])[0][:8])
        lsb, t = np.zeros(N), np.zeros(N)
        s0, s1 = min(c["seg_end"][0], N), min(c["seg_end"][1], N)
        for k, (lo, hi) in enumerate(((0, s0), (s0, s1), (s1, N))):
            if c["out_grid"][k] is not None:
                lsb[lo:hi] = float(c["out_grid"][k].scale)
                t[lo:hi] = ep["e"][lo:hi].astype(np.float64) / np.float64(F32(c["out_grid"][k].scale))
        _check_div(tag, y[:N], ep["y_div"], lsb, t)
        if n_id:                                     # the last workgroup saw the probe's image
            ks_e = _id_ks(K)[:: max(1, K // 64)]
            emb = y[N:N + n_id]
            assert np.array_equal(emb[:-1].astype(np.int64), img[ks_e].astype(np.int64)) and int(emb[-1]) == rs, (tag, "embedded identity rows")
    print(f"[gemv] {tag}: K={K} N={N} workgroups={c['wgs']} rows/wg={c['rpw']} max|tt|={tt_max}")
    return dict(tt_max=tt_max, wgs=c["wgs"], rpw=c["rpw"])


run_gemv_case.gate_mismatch = 0


# ---- hand-built cases -----------------------------------------------------------------------------------------------------------------
def _case(dev, rng, K, NL, mode, gate=False, w4=False, opre=False, fill="rand", act=0, bias_norm=True, norm16=True):
    """Fields of one hand-built launch.  mode: NORM / LNORM / F32 / I8."""
    pro = dict(a_grid=Grid(dev, 8, -2.5, 3.0), eps=1e-5)
    if mode == "I8":
        pro["xq"] = rng.integers(-128, 128, K).astype(np.int8)
        if fill == "sat":
            pro["xq"] = np.where(rng.random(K) < 0.5, -128, 127).astype(np.int8)
    else:
        x = (rng.standard_normal(K) * 1.7 + 0.3).astype(F32)
        if fill == "sat":
            x = (rng.standard_normal(K) * 40).astype(F32)
            pro["a_grid"] = Grid(dev, 8, -0.4, 0.5)
        elif fill == "const":
            x = np.full(K, 0.8125, F32)
        elif fill == "zero":
            x = np.zeros(K, F32)
        pro["x"] = x
        if mode in ("NORM", "LNORM"):
            pro["norm_w"] = O.fake_quant(rng.uniform(0.3, 1.7, K).astype(F32), *O.scale_offset_from_min_max(0.0, 1.7, 16, False))
            pro["layernorm"] = int(mode == "LNORM")
            if mode == "LNORM" and bias_norm:
                pro["norm_bias"] = (rng.standard_normal(K) * 0.2).astype(F32)
            if norm16:
                pro["norm_in"] = Grid(dev, 16, -60.0, 60.0)
    N = 2 * NL if gate else NL
    hi = 16 if w4 else 256
    wb = rng.integers(0, hi, (N, K)) - (0 if w4 else 128)
    if fill == "wext":
        wb = np.where(rng.random((N, K)) < 0.5, 0 if w4 else -128, 15 if w4 else 127)
    zp = rng.integers(-20, 21, N).astype(np.int32) if not w4 else rng.integers(0, 16, N).astype(np.int32)
    ct = rng.integers(-50000, 50001, N).astype(np.int32)
    if fill == "zpext":
        assert mode == "I8"
        rs = int(pro["xq"].astype(np.int64).sum())
        zp = np.where(np.arange(N) % 2 == 0, 2 ** 30 + 12345, -(2 ** 31) + 7).astype(np.int64)
        ct = O._wrap32(zp * rs + rng.integers(-1000, 1000, N)).astype(np.int32)    # zp rs and ct wrap, tt = sum + small fits
        zp = zp.astype(np.int32)
    spread = np.sqrt(K) * (4.6 if w4 else 74) * 74 + 1.0
    alpha = (rng.uniform(0.5, 1.5, N) * 1.5 / spread).astype(F32)
    bias = (rng.standard_normal(N) * 0.1).astype(F32)
    kw = dict(gate=gate, w4=w4)
    if gate:
        kw.update(out_grid=(Grid(dev, 8, -3.0, 3.0), Grid(dev, 8, -2.5, 2.5), None), gate_act=act,
                  gate_mid=Grid(dev, 16, 0.0, 1.0) if act == 0 else None, gate_actout=Grid(dev, 16, -1.0, 3.5), gate_out=Grid(dev, 8, -3.0, 3.0))
    else:
        s0 = max(1, min(NL - 1, NL // 3 + 3)) if NL > 1 else 1
        kw.update(seg_end=(s0, NL), out_grid=(Grid(dev, 8, -1.5, 1.5), Grid(dev, 16, -2.0, 2.0), None))
        if mode in ("I8", "F32"):
            kw["resid"] = (rng.standard_normal(NL) * 2).astype(F32)
    if opre:
        kw["opre"] = dict(o_acc=rng.integers(-60000, 60000, K).astype(np.int32), o_alpha=rng.uniform(2e-5, 5e-5, K).astype(F32),
                          o_ct=rng.integers(-3000, 3000, K).astype(np.int32),
                          o_bias=(rng.standard_normal(K) * 0.1).astype(F32) if act == 1 else None, o_out=Grid(dev, 16, -6.0, 6.0))
    return (wb, alpha, zp, ct, bias), pro, kw


INSTANTIATIONS = [(m, g, o, w4) for m in ("NORM", "LNORM") for g, o in ((False, False), (True, False), (True, True)) for w4 in (False, True)] + \
    [(m, False, False, w4) for m in ("F32", "I8") for w4 in (False, True)]


@pytest.mark.parametrize("mode,gate,opre,w4", INSTANTIATIONS)
def test_every_instantiation_at_a_ragged_shape(dev, mode, gate, opre, w4):
    """All 16 kernel instantiations at K = 2304 (not a multiple of 2048: the prologue lanes past the row clamp their loads) and 257
    logical rows (a ragged last workgroup), segment ends off multiples of 8 and of rows_per_wg; identity rows embedded (non-gate)."""
    rng = np.random.default_rng(INSTANTIATIONS.index((mode, gate, opre, w4)))
    act = int(w4)
    rows, pro, kw = _case(dev, rng, 2304, 257, mode, gate, w4, opre, act=act, bias_norm=not w4, norm16=not opre)
    run_gemv_case(dev, f"{mode}{'+GATE' if gate else ''}{'+OPRE' if opre else ''} {'W4' if w4 else 'W8'}", 2304, rows, pro,
                  zero_n=0 if gate else 2300, embed_id=not gate, **kw)


LIMITS = [  # (mode, gate, opre, w4, K, NL, fill)
    ("NORM", False, False, False, 256, 1, "rand"),
    ("NORM", False, False, True, 256, 7, "rand"),
    ("LNORM", False, False, False, 256, 255, "rand"),
    ("NORM", True, False, False, 256, 257, "rand"),
    ("NORM", False, False, False, 256, 131079, "rand"),          # > 256 x 512 rows: the rows_per_wg cap
    ("I8", False, False, True, 256, 131079, "rand"),
    ("NORM", False, False, False, 8192, 7, "rand"),              # the fp32 prologue's largest row
    ("LNORM", False, False, True, 8192, 255, "rand"),
    ("F32", False, False, False, 8192, 257, "rand"),
    ("LNORM", True, True, False, 4096, 255, "rand"),             # OPRE's largest row
    ("NORM", True, True, True, 4096, 257, "rand"),
    ("I8", False, False, False, 32768, 255, "zpext"),            # xq's largest row; zp rs and ct wrap int32
    ("I8", False, False, True, 32768, 257, "wext"),
    ("I8", False, False, False, 32768, 7, "sat"),
    ("NORM", False, False, False, 2048, 300, "sat"),
    ("LNORM", False, False, False, 2048, 300, "const"),          # LayerNorm variance 0
    ("LNORM", True, True, True, 2048, 100, "zero"),
    ("NORM", False, False, True, 2048, 300, "zero"),
    ("NORM", False, False, False, 2304, 300, "wext"),
    ("LNORM", True, False, True, 2304, 300, "wext"),
]


@pytest.mark.parametrize("mode,gate,opre,w4,K,NL,fill", LIMITS)
def test_limits_and_fills(dev, mode, gate, opre, w4, K, NL, fill):
    rng = np.random.default_rng(K * 7 + NL + len(fill))
    rows, pro, kw = _case(dev, rng, K, NL, mode, gate, w4, opre, fill=fill, act=NL % 2)
    if fill == "wext" and not w4:
        rows[2][:] = np.where(np.arange(len(rows[2])) % 2, 127, -128)    # extreme zero points as well
    r = run_gemv_case(dev, f"{mode}{'+GATE' if gate else ''}{'+OPRE' if opre else ''} {'W4' if w4 else 'W8'} {fill}", K, rows, pro, **kw)
    if NL > 131072:
        assert r["rpw"] == 512 and r["wgs"] > 256
    if K == 32768:
        print(f"[tt] K=32768 {fill}: largest |tt| = {r['tt_max']}")


# ---- engine-lowered launches at real model geometry --------------------------------------------------------------------------------
def _engine_model(dev, shape, w4):
    import mobilequant_amd as mq
    from mobilequant_amd.calibration import get_act_range
    from mobilequant_amd.llama import LlamaForCausalLM
    m = LlamaForCausalLM(shape)
    m.reset_parameters(seed=5, std=0.03)
    m = m.to(dev).eval().requires_grad_(False)
    g = torch.Generator().manual_seed(2)
    act = get_act_range(m, [torch.randint(0, shape.vocab, (1, 16), generator=g)])
    wcfg = mq.QuantConfig(bitwidth=4, is_per_channel=True) if w4 else mq.QuantConfig(bitwidth=8)
    mq.create_sim_qmodel(m, wcfg, mq.QuantConfig(bitwidth=8))
    for n, mod in m.named_modules():
        if isinstance(mod, mq.QLinear) and ("w2" in n or "o_proj" in n):
            mod.output_quantizer.qcfg.bitwidth = 16
        elif isinstance(mod, (mq.QRMSNorm, mq.QLayerNorm)):
            mod.input_quantizer.qcfg.bitwidth = 16
            mod.weight_quantizer.qcfg.bitwidth = 16
    mq.set_scale_and_offset(m, act, "buffer")
    mq.wire_integer_inputs(m)
    return m


def _module_rows(lins, a_grid, interleave=False):
    """Weight bytes and epilogue vectors of QLinears from the modules' own weights and quantizers: wb = q - shift (q the weight index,
    shift 128 + qmin for 8 bits, qmin for 4), alpha = fl(sa sw), w_zp = zw - shift, col_term = (128 - za) sum wb + K (128 - za)(shift - zw)."""
    parts = []
    for lin in lins:
        wq = lin.weight_quantizer
        W = lin.weight.detach().float().cpu().numpy()
        N, K = W.shape
        s = wq.scale.detach().float().cpu().numpy().reshape(-1, 1) if wq.scale.numel() > 1 else np.float32(wq.scale.reshape(-1)[0].item())
        o = wq.offset.detach().float().cpu().numpy().reshape(-1, 1) if wq.offset.numel() > 1 else np.float32(wq.offset.reshape(-1)[0].item())
        q = O.quantize_index(W, s, o, wq.qmin, wq.qmax).astype(np.int64)
        shift = wq.qmin if wq.qcfg.bitwidth == 4 else 128 + wq.qmin
        wb = (q - shift).astype(np.int8)
        zw = np.broadcast_to(np.asarray(o, np.float64).reshape(-1), (N,)).astype(np.int64)
        sw = np.broadcast_to(np.asarray(s, F32).reshape(-1), (N,)).astype(F32)
        c = 128 - int(a_grid.offset)
        alpha = (F32(a_grid.scale) * sw).astype(F32)
        zp = (zw - shift).astype(np.int32)
        ct = O._wrap32(c * wb.astype(np.int64).sum(1) + K * c * (shift - zw)).astype(np.int32)
        bias = lin.bias.detach().float().cpu().numpy() if lin.bias is not None else np.zeros(N, F32)
        parts.append((wb, alpha, zp, ct, bias))
    if interleave:
        return tuple(np.stack([p[i] for p in parts], axis=1).reshape(-1, *parts[0][i].shape[1:]) for i in range(5))
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(5))


def _norm_fields(norm, dev):
    from mobilequant_amd.quantization import qmodule as Q
    wq = norm.weight_quantizer
    w = norm.weight.detach().float().cpu().numpy()
    if wq is not None and not wq.bypassed():
        w = O.fake_quant(w, float(wq.scale.reshape(-1)[0]), float(wq.offset.reshape(-1)[0]), wq.qmin, wq.qmax)
    f = dict(norm_w=w, layernorm=int(isinstance(norm, Q.QLayerNorm)), norm_in=Grid.of(norm.input_quantizer, dev), eps=float(norm.eps),
             a_grid=Grid.of(norm.output_quantizer, dev))
    if f["layernorm"] and norm.bias is not None:
        f["norm_bias"] = norm.bias.detach().float().cpu().numpy()
    return f


ENGINES = [(name, L, w4) for name in ("tinyllama", "stablelm_2_1_6b", "gemma_2b") for L in (4, 5) for w4 in (False, True)]


@pytest.mark.parametrize("name,launches,w4", ENGINES)
def test_engine_lowered_launches_at_model_shapes(dev, name, launches, w4):
    """Every mq_decode_gemv block DecodeEngine lowers for a one-layer model at the real geometry, run unmodified, against the oracle built
    from the modules' weights: q|k|v segments, interleaved w1|w3 + gate (+ o_proj's epilogue), w2 / o_proj from the int8 image."""
    from mobilequant_amd.decode import DecodeEngine
    from mobilequant_amd.llama import LlamaShape
    from mobilequant_amd.quantization import qmodule as Q
    shape = getattr(LlamaShape, name)(layers=1, vocab=256, max_pos=64)
    m = _engine_model(dev, shape, w4)
    eng = DecodeEngine(m, cache_len=64, launches=launches, prefetch=0.0)
    assert eng.launches == launches
    layer = m.layers[0]
    attn, mlp = layer.self_attn, layer.mlp
    rng = np.random.default_rng(len(name) * 10 + launches + w4)
    H = shape.hidden
    x = (rng.standard_normal(H) * 1.5).astype(F32)
    gemvs = [a for kind, a in eng.phases if kind == "gemv"]
    # (1) input_layernorm + q|k|v
    nf = _norm_fields(layer.input_layernorm, dev)
    rows = _module_rows([attn.q_proj, attn.k_proj, attn.v_proj], nf["a_grid"].o)
    eng.x.copy_(torch.from_numpy(x))
    _engine_judge(dev, eng, gemvs[0], f"{name} L{launches} {'W4' if w4 else 'W8'} qkv", H, rows, dict(nf, x=x), out=eng.qkv,
                  out_grid=[Grid.of(l.output_quantizer, dev) for l in (attn.q_proj, attn.k_proj, attn.v_proj)],
                  seg_end=(attn.q_proj.weight.shape[0], attn.q_proj.weight.shape[0] + attn.k_proj.weight.shape[0]),
                  zero=eng.o_acc if launches == 4 else None)
    g_o = attn.o_proj.input_quantizer if attn.o_proj.input_quantizer is not None else (
        attn.pv_bmm.output_quantizer if Q._static_per_tensor(attn.pv_bmm.output_quantizer, 8) else attn.o_proj._input_grid)
    go = Grid.of(g_o, dev)
    op_rows = _module_rows([attn.o_proj], go.o)
    gi = 1
    if launches == 5:                                  # o_proj from the int8 image + residual (in place on x)
        xq = rng.integers(-128, 128, op_rows[0].shape[1]).astype(np.int8)
        eng.attn_q.copy_(torch.from_numpy(xq))
        eng.x.copy_(torch.from_numpy(x))
        _engine_judge(dev, eng, gemvs[1], f"{name} L5 {'W4' if w4 else 'W8'} o_proj", op_rows[0].shape[1], op_rows, dict(xq=xq, a_grid=go),
                      out=eng.x, out_grid=[Grid.of(attn.o_proj.output_quantizer, dev), None, None], resid=x)
        gi = 2
    # post_attention_layernorm + w1|w3 + gate (+ OPRE)
    nf2 = _norm_fields(layer.post_attention_layernorm, dev)
    rows13 = _module_rows([mlp.w1, mlp.w3], nf2["a_grid"].o, interleave=True)
    act = mlp.act_fn
    gk = dict(gate_act=0 if isinstance(act, Q.QSiLU) else 1, gate_mid=Grid.of(act.input2_quantizer, dev) if isinstance(act, Q.QSiLU) else None,
              gate_actout=Grid.of(act.output_quantizer, dev), gate_out=Grid.of(mlp.w2.input_quantizer, dev),
              out_grid=[Grid.of(mlp.w1.output_quantizer, dev), Grid.of(mlp.w3.output_quantizer, dev), None])
    opre = None
    if launches == 4:
        o_acc = rng.integers(-40000, 40000, H).astype(np.int32)
        eng.o_acc.copy_(torch.from_numpy(o_acc))
        opre = dict(o_acc=o_acc, o_alpha=op_rows[1], o_ct=op_rows[3], o_bias=op_rows[4] if attn.o_proj.bias is not None else None,
                    o_out=Grid.of(attn.o_proj.output_quantizer, dev))
    eng.x.copy_(torch.from_numpy(x))
    _engine_judge(dev, eng, gemvs[gi], f"{name} L{launches} {'W4' if w4 else 'W8'} w1|w3", H, rows13, dict(nf2, x=x), gate=True, opre=opre, **gk)
    # w2 from the int8 image + residual
    F = shape.ffn
    xq2 = rng.integers(-128, 128, F).astype(np.int8)
    eng.gate_q.copy_(torch.from_numpy(xq2))
    res = (rng.standard_normal(H) * 1.5).astype(F32)
    (eng.x_mid if launches == 4 else eng.x).copy_(torch.from_numpy(res))
    w2g = Grid.of(mlp.w2.input_quantizer, dev)
    _engine_judge(dev, eng, gemvs[gi + 1], f"{name} L{launches} {'W4' if w4 else 'W8'} w2", F, _module_rows([mlp.w2], w2g.o), dict(xq=xq2, a_grid=w2g),
                  out=eng.x, out_grid=[Grid.of(mlp.w2.output_quantizer, dev), None, None], resid=res)


def _engine_judge(dev, eng, a, tag, K, rows, pro, out=None, gate=False, out_grid=(None, None, None), seg_end=None, resid=None, zero=None,
                  opre=None, gate_act=0, gate_mid=None, gate_actout=None, gate_out=None):
    """Run the engine's own block a and judge what it wrote with _judge (no canaries: the engine owns the buffers)."""
    wb, alpha, zp, ct, bias = rows
    assert a.K == K and a.N == wb.shape[0]
    if zero is not None:
        zero.fill_(CANARY_I32)
    if opre is not None:
        eng.x_mid.fill_(float("nan"))
    wgs, rpw = _geometry(a)
    _launch(a)
    N = wb.shape[0]
    NL = N // 2 if gate else N
    if gate:
        gq = np.concatenate([eng.gate_q[:NL].cpu().numpy(), np.full(64, CANARY_I8, np.int8)])
        y = np.full(NL + 64, CANARY_F, F32)
    else:
        y = np.concatenate([out[:N].cpu().numpy(), np.full(64, CANARY_F, F32)])
        gq = None
    za = None
    if zero is not None:
        za = np.concatenate([zero.cpu().numpy(), np.full(64, CANARY_I32, np.int32)])
    xm = None
    if opre is not None:
        xm = np.concatenate([eng.x_mid.cpu().numpy(), np.full(64, np.nan, F32)])
    p = {k: (v.o if isinstance(v, Grid) else v) for k, v in pro.items()}
    c = dict(wb=wb, alpha=alpha, zp=zp, ct=ct, bias=bias, resid=resid, N=N, n_id=0, w4=bool(a.w4), gate=gate,
             seg_end=tuple(seg_end) if seg_end is not None else (N, N), out_grid=[_oo(g) for g in out_grid], gate_act=gate_act,
             gate_mid=_oo(gate_mid), gate_actout=_oo(gate_actout), gate_out=_oo(gate_out), opre=opre, zero_n=K if zero is not None else 0,
             wgs=wgs, rpw=rpw)
    if zero is not None:
        c["zero_n"] = zero.numel()
    if gate:                                           # (the engine's gate launch writes no y: compare gate_q only)
        c["skip_y"] = True
    return _judge(tag, K, a, pro, p, c, y, gq, za, xm, dev)


# ---- mq_decode_head / mq_decode_embed ----------------------------------------------------------------------------------------------
HEAD_NORMS = ["rms", "ln", "ln_noaffine", "ln_nobias", "none"]


def _head_case(dev, K, V, norm, lm_bias, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(K, device=dev, generator=g) * 2 + 0.25
    w = torch.empty(V, K, device=dev)
    for r0 in range(0, V, 16384):                      # (in chunks: V x K reaches 2 GB)
        w[r0:r0 + 16384] = torch.randn(min(16384, V - r0), K, device=dev, generator=g) * 0.03
    nw = torch.rand(K, device=dev, generator=g) + 0.5
    nb = torch.randn(K, device=dev, generator=g) * 0.1
    b = torch.randn(V, device=dev, generator=g) * 0.2 if lm_bias else None
    ln = norm.startswith("ln")
    nwp = None if norm in ("none", "ln_noaffine") else nw
    nbp = nb if norm == "ln" else None
    logits = torch.full((V + 64,), CANARY_F, device=dev)
    _call("mq_decode_head", x.data_ptr(), None if nwp is None else nwp.data_ptr(), None if nbp is None else nbp.data_ptr(), int(ln), 1e-5,
          w.data_ptr(), None if b is None else b.data_ptr(), K, V, logits.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    lg = logits.cpu().numpy()
    assert np.all(lg[V:] == CANARY_F), "logits written past V"
    s64, err = O.decode_head_norm(x.cpu().numpy(), None if nwp is None else nwp.cpu().numpy(), None if nbp is None else nbp.cpu().numpy(), int(ln), 1e-5)
    s64_t, err_t = torch.from_numpy(s64).to(dev), torch.from_numpy(err).to(dev)
    want, bound = [], []
    for r0 in range(0, V, 16384):
        l64, bd = O.decode_head_logits(w[r0:r0 + 16384].double(), s64_t, err_t, None if b is None else b[r0:r0 + 16384].double())
        want.append(l64.cpu().numpy())
        bound.append(bd.cpu().numpy())
    want, bound = np.concatenate(want), np.concatenate(bound)
    d = np.abs(lg[:V].astype(np.float64) - want)
    ratio = float((d / bound).max())
    assert np.all(d <= bound), (K, V, norm, ratio, int(np.argmax(d / bound)))
    order = np.argsort(want)[::-1]
    if V >= 2 and want[order[0]] - want[order[1]] > 2 * bound.max():
        assert int(np.argmax(lg[:V])) == int(order[0]), (K, V, norm)
    print(f"[head] K={K} V={V} norm={norm} bias={lm_bias}: largest error / bound = {ratio:.4f}")
    _head_case.worst = max(_head_case.worst, ratio)
    return ratio


_head_case.worst = 0.0


@pytest.mark.parametrize("K", [256, 2048, 260, 2052, 3072, 12288])
@pytest.mark.parametrize("norm", HEAD_NORMS)
def test_head_norms_and_paths(dev, K, norm):
    """Fast path (K % 256 == 0, K <= 2048) and slow path (up to 12 288) under every final norm, V past the 2048-block cap."""
    _head_case(dev, K, 8193, norm, lm_bias=K % 2 == 0 and norm != "none", seed=K + len(norm))


@pytest.mark.parametrize("V", [1, 3, 5, 8191, 8192, 8193, 16385, 32000, 100352, 256000])
def test_head_vocabularies(dev, V):
    """Vocabularies around the fast path's two-rows-in-flight loop ends and the block cap, up to Gemma's 256 000 rows (2 GB of fp32)."""
    _head_case(dev, 2048, V, "rms", lm_bias=False, seed=V)
    if V <= 100352:
        _head_case(dev, 2052, V, "ln", lm_bias=True, seed=V + 1)
    if V <= 32000:
        _head_case(dev, 256, V, "none", lm_bias=True, seed=V + 2)
    print(f"[head] largest error / bound so far: {_head_case.worst:.4f}")


@pytest.mark.parametrize("hidden,rot", [(2048, 64), (2052, 16), (256, 256)])
def test_embed_rows_at_the_ends(dev, hidden, rot):
    V, max_pos = 1000, 300
    g = torch.Generator(device=dev).manual_seed(hidden)
    table = torch.randn(V, hidden, device=dev, generator=g)
    cos, sin = torch.randn(max_pos, rot, device=dev, generator=g), torch.randn(max_pos, rot, device=dev, generator=g)
    for tok, pos in ((0, 0), (V - 1, max_pos - 1), (V - 1, 0), (0, max_pos - 1)):
        t = torch.tensor([tok], dtype=torch.int64, device=dev)
        p = torch.tensor([pos], dtype=torch.int32, device=dev)
        x = torch.full((hidden + 64,), CANARY_F, device=dev)
        rr = torch.full((2 * rot + 64,), CANARY_F, device=dev)
        _call("mq_decode_embed", table.data_ptr(), t.data_ptr(), hidden, V, cos.data_ptr(), sin.data_ptr(), p.data_ptr(), rot, max_pos,
              x.data_ptr(), rr.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert torch.equal(x[:hidden], table[tok]) and bool((x[hidden:] == CANARY_F).all())
        assert torch.equal(rr[:rot], cos[pos]) and torch.equal(rr[rot:2 * rot], sin[pos]) and bool((rr[2 * rot:] == CANARY_F).all())


def test_zz_report_counts():
    """(Runs last in this module: the totals the PR reports.)"""
    print(f"[totals] image elements one step off at near-ties: {_check_image.diffs}; gate_q one step off at flagged near-ties: "
          f"{run_gemv_case.gate_mismatch}; largest head error / bound: {_head_case.worst:.4f}; outputs one step from the division form: "
          f"{_check_div.diff} of {_check_div.rows}")
    if _check_div.rows:
        assert _check_div.diff <= 0.001 * _check_div.rows
