"""CPU oracle for the MobileQuant simulated-quant hot path.  TEST INFRASTRUCTURE ONLY.

This file is a numpy restatement of the reference's algorithm for the one hot path this
repository accelerates: the fake-quant arithmetic of
``mobilellm/quantization/qmodule.py`` and the running min/max statistics of
``ptq/generate_act_range.py`` / ``ptq/generate_act_scale_shift.py``.  Every function cites
the reference ``file:line`` it follows (paths relative to the reference checkout).

Rules (see DESIGN.md "Oracle"):
  * Only ``tests/``, ``__graft_entry__.smoke()`` and the ``cpu_baseline`` leg of
    ``bench.py`` may import this module.  The product package ``mobilequant_amd`` never does;
    it fails loudly when the HIP library is missing.
  * Parity is PINNED: ``tests/test_oracle_golden.py`` checks every function here bit-exactly
    against ``tests/golden/*.npz``, which ``oracle/gen_golden.py`` produced by importing the
    real reference (torch CPU) in the build container.
  * All arithmetic is IEEE fp32 (numpy float32), same operation order as the reference, so the
    integer indices it yields are the reference's, bit for bit.  The only operation that is NOT
    bit-reproducible is the fp32 matmul inside ``qlinear_sim`` (BLAS summation order); tests
    state a tolerance there and use ``qlinear_int_exact`` for the exact integer contraction.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
CLIPMIN = F32(1e-5)   # qmodule.py:11
CLIPMAX = F32(1e6)    # qmodule.py:12


# ----------------------------------------------------------------------------------------------
# a1  compute_scale_offset_from_min_max            qmodule.py:40-61
# ----------------------------------------------------------------------------------------------
def qrange(bitwidth: int, is_symmetric: bool):
    """(qmin, qmax) integer grid limits.  qmodule.py:48-54."""
    if is_symmetric:
        return -(2 ** (bitwidth - 1)), 2 ** (bitwidth - 1) - 1
    return 0, 2 ** bitwidth - 1


def scale_offset_from_min_max(min_val, max_val, bitwidth: int, is_symmetric: bool):
    """Returns (scale, offset, qmin, qmax); scale/offset are fp32 arrays shaped like min_val.

    qmodule.py:40-61: asymmetric ``alpha = max-min, beta = min``; symmetric
    ``alpha = max(|min|,|max|), beta = 0``; ``scale = clamp(alpha/qmax, 1e-5, 1e6)``;
    ``offset = -round(beta/scale)`` (round half to even; symmetric gives -0.0).
    Python floats enter through ``torch.tensor(v)`` = fp32 (qmodule.py:41-44).
    """
    mn = np.asarray(min_val, dtype=F32)
    mx = np.asarray(max_val, dtype=F32)
    qmin, qmax = qrange(bitwidth, is_symmetric)
    if is_symmetric:
        alpha = np.maximum(np.abs(mn), np.abs(mx))
        beta = np.zeros_like(alpha)
    else:
        alpha = mx - mn
        beta = mn
    scale = (alpha / F32(qmax)).astype(F32)
    scale = np.clip(scale, CLIPMIN, CLIPMAX).astype(F32)
    offset = (-np.rint((beta / scale).astype(F32))).astype(F32)
    return scale, offset, qmin, qmax


# ----------------------------------------------------------------------------------------------
# a2  compute_min_max_from_scale_offset            qmodule.py:66-76
# ----------------------------------------------------------------------------------------------
def min_max_from_scale_offset(scale, offset, bitwidth: int, is_symmetric: bool):
    """Inverse map used by export_act_range (qmodule.py:908-937)."""
    _, qmax = qrange(bitwidth, is_symmetric)
    s = np.clip(np.asarray(scale, dtype=F32), CLIPMIN, CLIPMAX).astype(F32)
    o = np.asarray(offset, dtype=F32)
    alpha = (s * F32(qmax)).astype(F32)
    beta = ((-o) * s).astype(F32)
    max_val = (alpha + beta).astype(F32)
    min_val = (-max_val) if is_symmetric else beta
    return min_val, max_val


# ----------------------------------------------------------------------------------------------
# a3  compute_min_max_from_tensor                  qmodule.py:26-34
# ----------------------------------------------------------------------------------------------
def min_max_from_tensor(x, is_per_channel: bool = False, group_size: int = -1):
    """Per-tensor amin/amax of the flattened tensor, or per-row (last dim, keepdim) /
    per-group (reshape(-1, g) first).  qmodule.py:26-34 and :259-268."""
    x = np.asarray(x)
    if is_per_channel:
        if group_size != -1:
            x = x.reshape(-1, group_size)
        return x.min(axis=-1, keepdims=True), x.max(axis=-1, keepdims=True)
    flat = x.reshape(-1)
    return flat.min(), flat.max()


# ----------------------------------------------------------------------------------------------
# a4/a5  round_ste + Quantizer.forward arithmetic   qmodule.py:17-21, :286-295
# ----------------------------------------------------------------------------------------------
def quantize_index(x, scale, offset, qmin: int, qmax: int):
    """Integer grid index as an fp32 array: ``clamp(round(x/scale) + offset, qmin, qmax)``.

    qmodule.py:286-287.  True IEEE division, round-half-even, fp32 add, clamp.  round_ste
    (qmodule.py:17-21) evaluates ``(round(t) - t) + t``: exact for finite t (the difference is exactly
    representable), NaN for t = +-inf (inf - inf) -- so an infinite input comes out NaN like a NaN one
    (frozen in tests/golden/nonfinite_cases.npz).  np.clip, like torch.clamp, keeps NaN.
    """
    x = np.asarray(x, dtype=F32)
    s = np.asarray(scale, dtype=F32)
    o = np.asarray(offset, dtype=F32)
    with np.errstate(invalid="ignore"):
        t = (x / s).astype(F32)
        r = ((np.rint(t) - t).astype(F32) + t).astype(F32)
        q = (r + o).astype(F32)
    return np.clip(q, F32(qmin), F32(qmax)).astype(F32)


def dequantize_index(q, scale, offset):
    """``(q - offset) * scale`` in fp32.  qmodule.py:290."""
    q = np.asarray(q, dtype=F32)
    s = np.asarray(scale, dtype=F32)
    o = np.asarray(offset, dtype=F32)
    return ((q - o).astype(F32) * s).astype(F32)


def fake_quant(x, scale, offset, qmin: int, qmax: int):
    """quantize -> dequantize, fp32.  qmodule.py:286-290."""
    return dequantize_index(quantize_index(x, scale, offset, qmin, qmax), scale, offset)


def fake_quant_backward(x, grad_y, scale, offset, qmin: int, qmax: int):
    """Gradients of ``y = (clamp(round_ste(x/s) + o, qmin, qmax) - o) * s`` (qmodule.py:17-21, :286-290) as
    torch autograd derives them: round is a straight-through identity, clamp passes the gradient where
    qmin <= q <= qmax.  With t = x/s, r = round(t), q = r + o:
        dL/dx = (g*s)/s      inside | 0                 clamped
        dL/ds = g * (r - t)  inside | g * (clamp(q)-o)  clamped
        dL/do = 0            inside | -g * s            clamped
    scale/offset gradients are summed over the elements that share them (all, or one row).
    Returns (grad_x, grad_scale, grad_offset) with the shapes of x / scale / offset."""
    x = np.asarray(x, dtype=F32)
    g = np.asarray(grad_y, dtype=F32)
    s = np.asarray(scale, dtype=F32)
    o = np.asarray(offset, dtype=F32)
    with np.errstate(invalid="ignore"):
        t = (x / s).astype(F32)
        r = ((np.rint(t) - t).astype(F32) + t).astype(F32)       # round_ste, see quantize_index
        q = (r + o).astype(F32)
    inside = (q >= F32(qmin)) & (q <= F32(qmax))
    qc = np.clip(q, F32(qmin), F32(qmax))
    # autograd chain for x: (g * s) through the clamp mask, then the division's grad / s  -- reproduced
    # op for op so grad_x is bit-identical to torch's (it is g only up to one rounding)
    gx = (np.where(inside, (g * s).astype(F32), F32(0)) / s).astype(F32)
    gs_e = np.where(inside, g * (r - t), g * (qc - o)).astype(np.float64)
    go_e = np.where(inside, 0.0, -g * s).astype(np.float64)
    if s.size == 1:
        return gx, np.asarray(gs_e.sum(), dtype=F32).reshape(s.shape), np.asarray(go_e.sum(), dtype=F32).reshape(o.shape)
    axes = tuple(range(1, x.ndim))
    return gx, gs_e.sum(axis=axes).astype(F32).reshape(s.shape), go_e.sum(axis=axes).astype(F32).reshape(o.shape)


def fake_quant_f16_per_tensor(x, scale, offset, qmin: int, qmax: int):
    """fp16 input with 0-dim fp32 scale/offset: the RESULT dtype stays fp16 (SURVEY 8a' item 4).

    Measured against torch CPU (and frozen in quantizer_cases.npz): each op of qmodule.py:286-290
    is evaluated in float with the half operand widened and the 0-dim fp32 scale/offset used at
    full fp32 precision, and the result is rounded to half once per op.
    """
    H = np.float16
    x = np.asarray(x, dtype=H)
    s = F32(scale)
    o = F32(offset)
    t = (x.astype(F32) / s).astype(H)
    with np.errstate(invalid="ignore"):
        r0 = np.rint(t.astype(F32)).astype(H)
        r = ((r0.astype(F32) - t.astype(F32)).astype(H).astype(F32) + t.astype(F32)).astype(H)   # round_ste in half
    q = (r.astype(F32) + o).astype(H)
    q = np.clip(q, H(qmin), H(qmax)).astype(H)
    d = (q.astype(F32) - o).astype(H)
    return (d.astype(F32) * s).astype(H), q


def fake_quant_f16_per_row(x, scale, offset, qmin: int, qmax: int):
    """fp16 input with a [rows, 1] fp32 scale / offset: torch promotes the whole expression to fp32 and the result is cast back to
    half once (qmodule.py:295; frozen in quantizer_cases.npz) -- fp32 arithmetic on the widened half, ONE final rounding."""
    x = np.asarray(x, dtype=np.float16)
    s = np.asarray(scale, dtype=F32).reshape(-1, 1)
    o = np.asarray(offset, dtype=F32).reshape(-1, 1)
    with np.errstate(over="ignore"):
        return fake_quant(x.astype(F32), s, o, qmin, qmax).astype(np.float16)


def quantize_storage(x, scale, offset, qmin: int, qmax: int, shift: int, chan_scale=None):
    """What mq_quantize / mq_quantize_tiled store for a [rows, cols] activation: (stored int64 [rows, cols], row_sum int32 [rows]).

    stored = quantize_index(x) - shift.  scale / offset hold one element (per-tensor) or `rows` (per-row grids, broadcast down the
    rows).  fp16 input is widened to fp32 first and everything behind is fp32 (NOT the per-op half arithmetic of
    fake_quant_f16_per_tensor).  chan_scale [cols]: the quotient x / chan_scale is rounded to fp32 and THEN quantized (two roundings:
    include/mobilequant_amd.h at mq_quantize).  Integer storage has no NaN: where the reference's index is NaN (the input is NaN or
    +-inf -- round_ste makes inf - inf of it -- or a quotient overflows) the stored value is qmin - shift (csrc/mq_quant.h, storage
    and image forms: "NaN -> qmin"; csrc/mq_common.h at div_by_scale).  Row sums are exact integer sums of the stored values."""
    x = np.asarray(x)
    assert x.ndim == 2 and x.dtype in (np.float32, np.float16)
    xf = x.astype(F32)
    rows = xf.shape[0]
    s = np.asarray(scale, dtype=F32).reshape(-1)
    o = np.asarray(offset, dtype=F32).reshape(-1)
    assert s.size == o.size and s.size in (1, rows)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        if chan_scale is not None:
            xf = (xf / np.asarray(chan_scale, dtype=F32).reshape(1, -1)).astype(F32)
        idx = quantize_index(xf, s.reshape(-1, 1), o.reshape(-1, 1), qmin, qmax)
    stored = np.where(np.isnan(idx), F32(qmin), idx).astype(np.int64) - int(shift)
    rs = stored.sum(axis=1)
    assert np.all(np.abs(rs) < 2 ** 31)
    return stored, rs.astype(np.int32)


def tiled_offset(row, k, cols):
    """Byte offset of element (row, k) in the fragment-blocked int8 image (include/mobilequant_amd.h at mq_quantize_tiled): 1-KiB
    blocks of 16 rows x 64 k ordered [row block][k block]; inside a block byte 16 * ((row & 15) + 16 * ((k & 63) >> 4)) + (k & 15).
    Plain index arithmetic on integers or integer arrays."""
    block = (row >> 4) * (cols >> 6) + (k >> 6)
    return block * 1024 + 16 * ((row & 15) + 16 * ((k & 63) >> 4)) + (k & 15)


def tiled_image_bytes(stored, rows, cols):
    """(image int8 [ceil16(rows) * cols], real bool [same]): `stored` [rows, cols] scattered byte by byte through tiled_offset, and
    the mask of the bytes that belong to real rows (padding rows are "written, never used": their bytes stay 0 here, unmasked)."""
    stored = np.asarray(stored)
    assert stored.shape == (rows, cols) and cols % 64 == 0
    assert stored.min() >= -128 and stored.max() <= 127
    n = (rows + 15) // 16 * 16 * cols
    image, real = np.zeros(n, np.int8), np.zeros(n, bool)
    r, k = np.meshgrid(np.arange(rows, dtype=np.int64), np.arange(cols, dtype=np.int64), indexing="ij")
    off = tiled_offset(r, k, cols)
    image[off] = stored.astype(np.int8)
    real[off] = True
    return image, real


def linear_epilogue_vectors(a_scale, a_offset, a_shift: int, w_scale, w_offset, w_shift: int, w_colsum, K: int):
    """(alpha fp32 [N], w_zp int32 [N], col_term int32 [N]) of mq_linear_epilogue_prepare (include/mobilequant_amd.h):
    alpha = a_scale * w_scale (one fp32 product), w_zp = (int)w_offset - w_shift, col_term = -za * w_colsum + K * za * w_zp with
    za = (int)a_offset - a_shift, evaluated in Python integers and reduced modulo 2^32 to int32 (two's complement).  w_scale /
    w_offset hold one element or N."""
    colsum = np.asarray(w_colsum).reshape(-1)
    n = colsum.size
    ws = np.broadcast_to(np.asarray(w_scale, dtype=F32).reshape(-1), (n,))
    wo = np.broadcast_to(np.asarray(w_offset, dtype=F32).reshape(-1), (n,))
    alpha = (F32(np.asarray(a_scale).reshape(-1)[0]) * ws).astype(F32)
    za = int(np.asarray(a_offset).reshape(-1)[0]) - int(a_shift)
    zw = [int(v) - int(w_shift) for v in wo]
    term = [(-za * int(c) + int(K) * za * z) % (1 << 32) for c, z in zip(colsum, zw)]
    term = [t - (1 << 32) if t >= (1 << 31) else t for t in term]
    return alpha, np.array(zw, dtype=np.int32), np.array(term, dtype=np.int32)


class QuantizerOracle:
    """State machine of ``Quantizer`` (qmodule.py:112-295) without autograd.

    ``forward`` reproduces qmodule.py:251-295: bypass when disabled or bitwidth > 16; optional
    group reshape; (re)compute scale/offset when dynamic / LWC / not cached; fake-quantise.
    """

    def __init__(self, bitwidth=32, group_size=-1, is_symmetric=False, is_per_channel=False,
                 is_dynamic=False):
        self.bitwidth, self.group_size = bitwidth, group_size
        self.is_symmetric, self.is_per_channel, self.is_dynamic = is_symmetric, is_per_channel, is_dynamic
        self.enable = True
        self.scale = self.offset = None
        self.qmin = self.qmax = None

    def set_from_minmax(self, mn, mx):                       # qmodule.py:216-245
        self.scale, self.offset, self.qmin, self.qmax = scale_offset_from_min_max(
            mn, mx, self.bitwidth, self.is_symmetric)

    def forward(self, x, return_index=False):
        if (not self.enable) or self.bitwidth > 16:          # qmodule.py:252-253
            return (x, None) if return_index else x
        x = np.asarray(x, dtype=F32)
        shape = x.shape
        if self.is_per_channel and self.group_size != -1:    # qmodule.py:259-260
            x = x.reshape(-1, self.group_size)
        if self.is_dynamic or self.scale is None:            # qmodule.py:262-277
            mn, mx = min_max_from_tensor(x, self.is_per_channel, -1)
            self.set_from_minmax(mn, mx)
        q = quantize_index(x, self.scale, self.offset, self.qmin, self.qmax)
        y = dequantize_index(q, self.scale, self.offset).reshape(shape)
        return (y, q.reshape(shape)) if return_index else y


# ----------------------------------------------------------------------------------------------
# a8  QLinear.forward                               qmodule.py:341-358
# ----------------------------------------------------------------------------------------------
def qlinear_sim(x, weight, bias, w_q: QuantizerOracle | None, in_q: QuantizerOracle | None,
                out_q: QuantizerOracle | None):
    """The reference's simulated path: fake-quant W, (opt) fake-quant x, fp32 linear, fake-quant out.

    qmodule.py:341-358.  The fp32 matmul's summation order is BLAS-defined, so the pre-output-
    quant values agree with torch only to fp32 round-off (tests state the tolerance).
    """
    w = np.asarray(weight, dtype=F32)
    if w_q is not None:
        w = w_q.forward(w)
    x = np.asarray(x, dtype=F32)
    if in_q is not None:
        x = in_q.forward(x)
    out = x.reshape(-1, w.shape[1]) @ w.T
    if bias is not None:
        out = out + np.asarray(bias, dtype=F32)
    out = out.astype(F32).reshape(*x.shape[:-1], w.shape[0])
    if out_q is not None:
        out = out_q.forward(out)
    return out


def qlinear_int_exact(qa, za, sa, qw, zw, sw, bias=None, blas=False):
    """Integer-GEMM equivalence of QLinear (SURVEY 8a' item 9), exact contraction.

    ``out[m,n] = sa*sw[n] * sum_k (qa[m,k]-za)(qw[n,k]-zw[n]) + bias[n]``.  The contraction is
    done in int64 (exact); the scaling mirrors the HIP epilogue: one int->fp32 conversion, one
    multiply by fp32(sa*sw[n]), one add.  Returns (acc_int64, out_fp32).
    blas=True: the same contraction as a float64 BLAS product -- still exact (every partial sum is an integer below
    K * 511 * 511 < 2^53 for K <= 65536), and fast enough to check EVERY output of the full-size BASELINE shapes.
    """
    qa = np.asarray(qa, dtype=np.int64)
    qw = np.asarray(qw, dtype=np.int64)
    za_i = np.asarray(za, dtype=np.int64)
    zw_i = np.asarray(zw, dtype=np.int64).reshape(-1, 1) if np.ndim(zw) else np.int64(zw)
    if blas:
        assert qa.shape[1] * 511 * 511 < 2 ** 53
        acc = np.rint((qa - za_i).astype(np.float64) @ (qw - zw_i).astype(np.float64).T).astype(np.int64)
    else:
        acc = (qa - za_i) @ (qw - zw_i).T
    alpha = (F32(sa) * np.asarray(sw, dtype=F32).reshape(-1)).astype(F32)
    out = (acc.astype(F32) * alpha).astype(F32)
    if bias is not None:
        out = (out + np.asarray(bias, dtype=F32)).astype(F32)
    return acc, out


# ----------------------------------------------------------------------------------------------
# a12  update_act_range                             ptq/generate_act_range.py:55-69
# ----------------------------------------------------------------------------------------------
class ActRangeOracle:
    """Running min/max per (module name, field) over a stream of tensors.

    per-tensor: Python ``min``/``max`` of ``.min().item()/.max().item()`` (generate_act_range.py:65-69);
    per-channel: ``reshape(-1, C)``, min/max over dim 0, running ``minimum``/``maximum`` kept as a
    ``[2, C]`` tensor (generate_act_range.py:57-63).
    """

    def __init__(self, per_channel: bool = False):
        self.per_channel = per_channel
        self.act_dict: dict = {}

    def update(self, name: str, field: str, t):
        t = np.asarray(t, dtype=F32)
        entry = self.act_dict.setdefault(name, {})
        if self.per_channel:
            t2 = t.reshape(-1, t.shape[-1])
            cur = np.stack((t2.min(axis=0), t2.max(axis=0)), axis=0)
            if field in entry:
                cur[0] = np.minimum(entry[field][0], cur[0])
                cur[1] = np.maximum(entry[field][1], cur[1])
            entry[field] = cur
        else:
            mn, mx = float(t.min()), float(t.max())
            if field in entry:
                mn, mx = min(entry[field][0], mn), max(entry[field][1], mx)
            entry[field] = [mn, mx]

    @staticmethod
    def merge(dicts, per_channel: bool):
        """Min/max merge of several shards' act_dicts: what the all-reduce computes."""
        out: dict = {}
        for d in dicts:
            for name, fields in d.items():
                for field, v in fields.items():
                    e = out.setdefault(name, {})
                    if field not in e:
                        e[field] = np.array(v, dtype=F32).copy() if per_channel else list(v)
                    elif per_channel:
                        e[field][0] = np.minimum(e[field][0], v[0])
                        e[field][1] = np.maximum(e[field][1], v[1])
                    else:
                        e[field] = [min(e[field][0], v[0]), max(e[field][1], v[1])]
        return out


# ----------------------------------------------------------------------------------------------
# a13  stat_tensor (SmoothQuant absmax)             ptq/generate_act_scale_shift.py:47-55
# ----------------------------------------------------------------------------------------------
class ActScaleOracle:
    """Running per-channel absmax keyed ``"<module>_<field>"`` (generate_act_scale_shift.py:47-55)."""

    def __init__(self):
        self.act_scales: dict = {}

    def update(self, name: str, field: str, t):
        t = np.asarray(t, dtype=F32)
        cur = np.abs(t.reshape(-1, t.shape[-1])).max(axis=0)
        key = f"{name}_{field}"
        self.act_scales[key] = np.maximum(self.act_scales[key], cur) if key in self.act_scales else cur


# ----------------------------------------------------------------------------------------------
# Storage formats the integer path adds (no reference counterpart; defined in DESIGN.md).
# The values they carry are the reference's indices from quantize_index().
# ----------------------------------------------------------------------------------------------
def qrmsnorm(x, weight, bias, eps, in_q, w_q, out_q):
    """QRMSNorm.forward (qmodule.py:518-530 around HFRMSNorm.forward_impl, hf_model.py:184-195), fp32:
    ``Qout( Qw(weight) * (xi * rsqrt(mean(xi^2, -1) + eps)) (+ bias) )`` with ``xi = Qin(x)``; any quantizer may be
    None.  rsqrt is 1/sqrt with both operations correctly rounded (what torch's CPU kernel computes); the mean is
    numpy's pairwise sum / n, which is not torch's summation order: agreement with the frozen reference outputs
    is within one output LSB on a vanishing fraction of elements (tests state the bound)."""
    x = np.asarray(x, dtype=F32)
    w = np.asarray(weight, dtype=F32)
    xi = in_q.forward(x) if in_q is not None else x
    wq = w_q.forward(w) if w_q is not None else w
    ms = (xi * xi).astype(F32).mean(axis=-1, keepdims=True, dtype=F32)
    r = (F32(1.0) / np.sqrt((ms + F32(eps)).astype(F32)).astype(F32)).astype(F32)
    y = (wq * (xi * r).astype(F32)).astype(F32)
    if bias is not None:
        y = (y + np.asarray(bias, dtype=F32)).astype(F32)
    return out_q.forward(y) if out_q is not None else y


def qlayernorm(x, weight, bias, eps, in_q, w_q, out_q):
    """QLayerNorm.forward (qmodule.py:624-640 around F.layer_norm), fp32: mean and biased variance over the last dim,
    ``y = (xi * rstd + (-rstd * mean)) * Qw(weight) + bias`` (the expression of torch's CPU kernel; bias is not
    quantised), then the output quantizer.  Same summation-order caveat as qrmsnorm."""
    x = np.asarray(x, dtype=F32)
    xi = in_q.forward(x) if in_q is not None else x
    wq = w_q.forward(np.asarray(weight, dtype=F32)) if w_q is not None else np.asarray(weight, dtype=F32)
    mu = xi.mean(axis=-1, keepdims=True, dtype=F32)
    d = (xi - mu).astype(F32)
    var = (d * d).astype(F32).mean(axis=-1, keepdims=True, dtype=F32)
    rstd = (F32(1.0) / np.sqrt((var + F32(eps)).astype(F32)).astype(F32)).astype(F32)
    y = (((xi * rstd).astype(F32) + (-rstd * mu).astype(F32)).astype(F32) * wq).astype(F32)
    if bias is not None:
        y = (y + np.asarray(bias, dtype=F32)).astype(F32)
    return out_q.forward(y) if out_q is not None else y


def qsilu(x, in_q, mid_q, out_q):
    """QSiLU.forward (qmodule.py:739-754): ``Qout( xi * Qmid(sigmoid(xi)) )``, ``xi = Qin(x)``; fp32, sigmoid =
    1 / (1 + exp(-x)).  exp is the platform's (<= 1 ulp), so agreement with the frozen reference output is up to
    one output LSB on a vanishing fraction of elements."""
    x = np.asarray(x, dtype=F32)
    xi = in_q.forward(x) if in_q is not None else x
    with np.errstate(over="ignore"):
        g = (F32(1.0) / (F32(1.0) + np.exp(-xi).astype(F32)).astype(F32)).astype(F32)
    g = mid_q.forward(g) if mid_q is not None else g
    y = (xi * g).astype(F32)
    return out_q.forward(y) if out_q is not None else y


def qgelu(x, in_q, out_q):
    """QGELU.forward (qmodule.py:790-798): ``Qout( 0.5 * xi * (1 + erf(xi / sqrt 2)) )``, fp32."""
    from scipy.special import erf
    x = np.asarray(x, dtype=F32)
    xi = in_q.forward(x) if in_q is not None else x
    e = erf((xi * F32(0.7071067811865476)).astype(F32).astype(np.float64)).astype(F32)
    y = ((F32(0.5) * xi).astype(F32) * (F32(1.0) + e).astype(F32)).astype(F32)
    return out_q.forward(y) if out_q is not None else y


def index_to_i8(q, qmin: int):
    """Signed-byte storage of an 8-bit index: unsigned grids [0,255] are stored as q-128
    (MFMA i8 is signed), signed grids [-128,127] as is.  Returns (int8 array, shift)."""
    shift = 128 if qmin == 0 else 0
    return (np.asarray(q, dtype=np.int32) - shift).astype(np.int8), shift


def pack_w4(q, qmin: int):
    """Pack 4-bit weight indices [N,K] two per byte, K-interleaved in blocks of 32:
    byte j of a 16-byte group holds element j (low nibble) and element j+16 (high nibble) of the
    32-element K block.  Nibbles are stored unsigned (q - qmin).  K must be a multiple of 32."""
    q = np.asarray(q, dtype=np.int32) - qmin
    n, k = q.shape
    assert k % 32 == 0 and q.min() >= 0 and q.max() <= 15
    blk = q.reshape(n, k // 32, 2, 16)
    return (blk[:, :, 0, :] | (blk[:, :, 1, :] << 4)).astype(np.uint8).reshape(n, k // 2)


def unpack_w4(packed, qmin: int):
    p = np.asarray(packed, dtype=np.uint8)
    n, kh = p.shape
    blk = p.reshape(n, kh // 16, 16).astype(np.int32)
    out = np.stack((blk & 15, blk >> 4), axis=2).reshape(n, kh * 2)
    return out + qmin


# ----------------------------------------------------------------------------------------------
# a7  learnable weight clipping                      qmodule.py:133-185, :262-277
# ----------------------------------------------------------------------------------------------
def sigmoid_f32(x):
    """torch.sigmoid in fp32 (vectorised CPU kernels differ from this expression by at most one ulp; tests state it)."""
    x = np.asarray(x, dtype=F32)
    return (F32(1.0) / (F32(1.0) + np.exp(-x).astype(F32))).astype(F32)


def lwc_range(w, up_factor, low_factor, is_per_channel: bool):
    """Clipped range of a weight under LWC: ``max * sigmoid(upbound_factor)``, ``min * sigmoid(lowbound_factor)``
    (qmodule.py:271-273; the same lines in run_lwc :172-174)."""
    mn, mx = min_max_from_tensor(w, is_per_channel, -1)
    return (sigmoid_f32(low_factor) * mn).astype(F32), (sigmoid_f32(up_factor) * mx).astype(F32)


def lwc_forward(w, up_factor, low_factor, bitwidth: int, is_symmetric: bool, is_per_channel: bool):
    """Quantizer.forward with LWC enabled (qmodule.py:262-290): grid from the clipped range, then fake-quant.
    Returns (y, scale, offset)."""
    mn, mx = lwc_range(w, up_factor, low_factor, is_per_channel)
    scale, offset, qmin, qmax = scale_offset_from_min_max(mn, mx, bitwidth, is_symmetric)
    return fake_quant(w, scale, offset, qmin, qmax), scale, offset


def run_lwc(w, up_factor, low_factor, is_per_channel: bool):
    """Quantizer.run_lwc (qmodule.py:159-185): clamp the weight to its clipped range."""
    mn, mx = lwc_range(w, up_factor, low_factor, is_per_channel)
    return np.clip(np.asarray(w, dtype=F32), mn, mx).astype(F32)


def lwc_backward(w, up_factor, low_factor, grad_y, bitwidth: int, is_symmetric: bool, is_per_channel: bool):
    """Gradients of ``(lwc_forward(w) * grad_y).sum()`` w.r.t. upbound_factor, lowbound_factor and w, as torch autograd derives
    them from qmodule.py:262-290 + :40-61: through fake_quant to (scale, offset) (fake_quant_backward), through
    ``scale = clamp(alpha / qmax)``, ``offset = -round(beta / scale)`` (round: zero gradient) to the clipped (min, max), through
    the sigmoid to the factors, and through amin / amax (gradient to the extreme element, split evenly between ties) to w."""
    w = np.asarray(w, dtype=F32)
    mn0, mx0 = min_max_from_tensor(w, is_per_channel, -1)
    su, sl = sigmoid_f32(up_factor), sigmoid_f32(low_factor)
    mn, mx = (sl * mn0).astype(F32), (su * mx0).astype(F32)
    scale, offset, qmin, qmax = scale_offset_from_min_max(mn, mx, bitwidth, is_symmetric)
    gx, gs, go = fake_quant_backward(w, grad_y, scale, offset, qmin, qmax)
    # offset = -round(beta / scale): torch.round has zero gradient -> nothing flows through the offset
    raw = (mx - mn) / F32(qmax) if not is_symmetric else np.maximum(np.abs(mn), np.abs(mx)) / F32(qmax)
    inside = ((raw >= CLIPMIN) & (raw <= CLIPMAX)).astype(F32)            # clamp(min=1e-5, max=1e6)
    g_alpha = gs.reshape(np.shape(scale)) * inside / F32(qmax)
    if is_symmetric:
        take_max = (np.abs(mx) >= np.abs(mn)).astype(F32)                 # torch.maximum: gradient to the larger (ties: split)
        tie = (np.abs(mx) == np.abs(mn)).astype(F32)
        wmx = take_max - 0.5 * tie
        wmn = (1 - take_max) + 0.5 * tie
        g_mx = g_alpha * wmx * np.sign(mx)
        g_mn = g_alpha * wmn * np.sign(mn)
    else:
        g_mx, g_mn = g_alpha, -g_alpha
    g_up = (g_mx * mx0 * su * (1 - su)).astype(F32)
    g_lo = (g_mn * mn0 * sl * (1 - sl)).astype(F32)
    # amax / amin backward: the extreme element(s) of each reduction group
    is_mx = (w == mx0).astype(F32)
    is_mn = (w == mn0).astype(F32)
    ax = -1 if is_per_channel else None
    g_w = gx + (g_mx * su) * is_mx / is_mx.sum(axis=ax, keepdims=is_per_channel) \
             + (g_mn * sl) * is_mn / is_mn.sum(axis=ax, keepdims=is_per_channel)
    return g_up, g_lo, g_w.astype(F32)


# ----------------------------------------------------------------------------------------------
# a10  QMatMul.forward                               qmodule.py:453-466
# ----------------------------------------------------------------------------------------------
def qmatmul_sim(a, b, q1: QuantizerOracle | None, q2: QuantizerOracle | None, out_q: QuantizerOracle | None):
    """fake-quant both operands, fp32 matmul (summation order BLAS-defined), fake-quant the product."""
    a = np.asarray(a, dtype=F32)
    b = np.asarray(b, dtype=F32)
    if q1 is not None:
        a = q1.forward(a)
    if q2 is not None:
        b = q2.forward(b)
    out = np.matmul(a, b).astype(F32)
    return out_q.forward(out) if out_q is not None else out


def qmatmul_int_exact(qa, za, sa, qb, zb, sb):
    """Integer equivalent of the product inside QMatMul: ``sa*sb * sum_k (qa-za)(qb-zb)`` with an exact contraction (float64
    BLAS over integers), scaled once: one int -> fp32 conversion, one multiply by fp32(sa*sb).  qa [..., M, K], qb [..., K, N]."""
    acc = np.rint(np.matmul((np.asarray(qa, np.float64) - np.float64(za)), (np.asarray(qb, np.float64) - np.float64(zb)))).astype(np.int64)
    return acc, (acc.astype(F32) * (F32(sa) * F32(sb))).astype(F32)


# ----------------------------------------------------------------------------------------------
# a10 (in context)  attention core around the two QMatMuls      hf_model.py:486-534
# ----------------------------------------------------------------------------------------------
def rope_rotate_half(x, cos, sin):
    """x [..., S, D], cos / sin [S, D]:  x * cos + rotate_half(x) * sin  (hf_model.py:486-488 -> apply_rotary_pos_emb)."""
    x = np.asarray(x, dtype=F32)
    h = x.shape[-1] // 2
    rot = np.concatenate((-x[..., h:], x[..., :h]), axis=-1)
    return (x * cos.astype(F32)).astype(F32) + (rot * sin.astype(F32)).astype(F32)


def rope_partial(x, cos, sin):
    """Partial rotary embedding (hf_model.py:489-500): cos / sin [S, rot] with rot < D rotate the first rot dims of x [..., S, D],
    the rest passes through; rot == D is the plain rotate-half form (hf_model.py:487)."""
    rot = cos.shape[-1]
    x = np.asarray(x, dtype=F32)
    if rot == x.shape[-1]:
        return rope_rotate_half(x, cos, sin)
    return np.concatenate((rope_rotate_half(x[..., :rot], cos, sin), x[..., rot:]), axis=-1)


def _qmatmul_exact(a, b, q1: QuantizerOracle, q2: QuantizerOracle, out_q: QuantizerOracle | None, double_scale: bool):
    """QMatMul with its contraction carried out EXACTLY over the quantizer indices (what the MFMA / dot4 kernels compute), where the
    reference's fp32 matmul rounds after every product: s_a s_b sum_k (ia - za)(ib - zb), one rounding of fl32(s_a * s_b), then either
    one fp32 multiply of the (exact in fp32: |sum| < 2^24) integer (double_scale False: the q.k^T product) or one rounding of the
    double product (True: the p.v product, whose integer sums exceed 2^24 -- mq_attention.hip / mq_decode.hip)."""
    _, ia = q1.forward(np.asarray(a, F32), return_index=True)
    _, ib = q2.forward(np.asarray(b, F32), return_index=True)
    acc = np.rint(np.matmul(ia.astype(np.float64) - np.float64(q1.offset), ib.astype(np.float64) - np.float64(q2.offset))).astype(np.int64)
    alpha = F32(F32(q1.scale) * F32(q2.scale))
    out = (acc.astype(np.float64) * np.float64(alpha)).astype(F32) if double_scale else (acc.astype(F32) * alpha).astype(F32)
    return out_q.forward(out) if out_q is not None else out


def qmatmul_exact(a, b, q1: QuantizerOracle, q2: QuantizerOracle, out_q: QuantizerOracle | None):
    """What mq_qmatmul (the standalone integer QMatMul, qmodule.py:453-466) computes: the exact contraction over the indices, one
    rounding -- single-precision scale for operands of at most 8 bits, the rounded double product when the first operand is wider
    (its integer sums exceed 2^24) -- then the output quantizer."""
    return _qmatmul_exact(a, b, q1, q2, out_q, double_scale=q1.bitwidth > 8)


def attention_sim(q, k, v, cos, sin, heads, kv_heads, qk: tuple, pv: tuple, exact_int: bool = False):
    """Causal prefill attention of one sequence as the reference computes it: q [S, heads*D], k / v [S, kv_heads*D] projection
    outputs; RoPE (cos / sin [S, rot_dim]: full or partial, hf_model.py:486-500); repeat_kv (hf_model.py:509-510); qk_bmm (a QMatMul:
    qk = (input, input2, output) QuantizerOracles) / sqrt(D); + causal mask; fp32 softmax; pv_bmm (pv = its three quantizers).
    Returns [S, heads*D] (the layout o_proj reads).
    exact_int: both contractions exact over the indices (_qmatmul_exact) instead of the reference's fp32 matmuls -- the arithmetic
    of the integer kernels WITHOUT their fast quantizer / exponential forms: what separates "the integer path differs from an fp32
    matmul by that matmul's own rounding" from "the kernel's approximations flipped an index" in the tests."""
    S = q.shape[0]
    D = q.shape[1] // heads
    qh = rope_partial(np.asarray(q, F32).reshape(S, heads, D).transpose(1, 0, 2), cos, sin)
    kh = rope_partial(np.asarray(k, F32).reshape(S, kv_heads, D).transpose(1, 0, 2), cos, sin)
    vh = np.asarray(v, F32).reshape(S, kv_heads, D).transpose(1, 0, 2)
    rep = heads // kv_heads
    kh, vh = np.repeat(kh, rep, axis=0), np.repeat(vh, rep, axis=0)
    if exact_int:
        att = _qmatmul_exact(qh, kh.transpose(0, 2, 1), *qk, double_scale=False) / F32(np.sqrt(F32(D)))
    else:
        att = qmatmul_sim(qh, kh.transpose(0, 2, 1), *qk) / F32(np.sqrt(F32(D)))
    mask = np.triu(np.full((S, S), -np.inf, dtype=F32), 1)
    att = (att + mask).astype(F32)
    att = att - att.max(axis=-1, keepdims=True)
    e = np.exp(att, dtype=F32)
    p = (e / e.sum(axis=-1, keepdims=True, dtype=F32)).astype(F32)
    out = _qmatmul_exact(p, vh, *pv, double_scale=True) if exact_int else qmatmul_sim(p, vh, *pv)
    return out.transpose(1, 0, 2).reshape(S, heads * D)


# ----------------------------------------------------------------------------------------------
# a10 (one decode step)  row `pos` of attention_sim from a KV cache of int8 indices
# ----------------------------------------------------------------------------------------------
def quantizer_oracle_from(scale, offset, qmin, qmax) -> QuantizerOracle:
    """A static per-tensor QuantizerOracle on a given grid (e.g. a torch Quantizer's scale / offset / qmin / qmax)."""
    g = QuantizerOracle(bitwidth=int(round(np.log2(float(qmax) - float(qmin) + 1))))
    g.scale, g.offset, g.qmin, g.qmax = F32(scale), F32(offset), int(qmin), int(qmax)
    return g


def _index(x, g: QuantizerOracle):
    return quantize_index(x, g.scale, g.offset, g.qmin, g.qmax)


def decode_attention_step(q, k, v, k_cache, v_cache, pos, cos_row, sin_row, heads, kv_heads, qk: tuple, pv: tuple,
                          o_in: QuantizerOracle | None = None):
    """One head-group's decode step at position `pos` as the reference computes row `pos` of attention_sim(..., exact_int=True), from
    the engine's state: q [heads*D], k / v [kv_heads*D] fp32 rows of the new token (before RoPE); k_cache / v_cache [kv_heads, >= pos, D]
    int8 indices - 128 on qk.input2 / pv.input2 (the LOGICAL value layout); cos_row / sin_row [rot_dim] (rot_dim < D: partial rotary).
    qk = (input, input2, output) and pv = (input, input2, output) QuantizerOracles; o_in: the grid o_proj reads pv's output on (None: pv's
    output grid).  The softmax is evaluated twice: in fp32 in the reference's order (np.exp, np.sum of the row, one division) and in
    float64 (from the same fp32 scores).  Returns a dict:
      k_new / v_new [kv_heads, D] int8   the bytes the step appends at `pos`
      scores [heads, T] fp32             qk_bmm output / sqrt(D), T = pos + 1
      p_idx / p_idx64 [heads, T] int64   pv.input indices of the probabilities (fp32 / float64 softmax)
      p_t64 [heads, T] float64           the float64 probabilities divided by pv.input's scale (pre-rounding value of the index)
      iv [kv_heads, T, D] fp32           the value indices (0 .. 255) incl. the new position's
      acc [heads, D] int64               sum_t (ip - zp)(iv - zv) from the fp32 probabilities
      y [heads*D] fp32                   pv_bmm's output (row `pos` of attention_sim)
      out_q [heads*D] int8               o_proj's input image (index on o_in - 128): what attn_q / out_q hold
    """
    qa, qb, qo = qk
    pa, pb, po = pv
    o_in = po if o_in is None else o_in
    q = np.asarray(q, F32).reshape(heads, 1, -1)
    D = q.shape[-1]
    k = np.asarray(k, F32).reshape(kv_heads, 1, D)
    v = np.asarray(v, F32).reshape(kv_heads, D)
    cos_row, sin_row = np.asarray(cos_row, F32)[None], np.asarray(sin_row, F32)[None]
    T = int(pos) + 1
    iq = _index(rope_partial(q, cos_row, sin_row)[:, 0], qa)                        # [heads, D]
    ik_new = _index(rope_partial(k, cos_row, sin_row)[:, 0], qb)
    iv_new = _index(v, pb)
    k_new = (ik_new.astype(np.int64) - 128).astype(np.int8)
    v_new = (iv_new.astype(np.int64) - 128).astype(np.int8)
    ik = np.concatenate([np.asarray(k_cache)[:, :pos].astype(F32) + F32(128), ik_new[:, None]], axis=1)        # [kv, T, D] indices
    iv = np.concatenate([np.asarray(v_cache)[:, :pos].astype(F32) + F32(128), iv_new[:, None]], axis=1)
    rep = heads // kv_heads
    # q.k^T exactly over the indices (every partial sum is an integer below D 255^2 < 2^24: exact in fp32), one fp32 multiply, the output
    # quantizer, / sqrt(D)       (_qmatmul_exact, double_scale False; a KV head's query heads together: no repeat_kv copy)
    acc_qk = np.matmul((iq - F32(qa.offset)).reshape(kv_heads, rep, D), (ik - F32(qb.offset)).transpose(0, 2, 1)).reshape(heads, T)
    acc_qk = np.rint(acc_qk).astype(np.int64)
    alpha_qk = F32(F32(qa.scale) * F32(qb.scale))
    scores = (qo.forward((acc_qk.astype(F32) * alpha_qk).astype(F32)) / F32(np.sqrt(F32(D)))).astype(F32)
    # softmax: fp32 in attention_sim's order, and float64
    x = (scores - scores.max(axis=-1, keepdims=True)).astype(F32)
    e = np.exp(x, dtype=F32)
    p = (e / e.sum(axis=-1, keepdims=True, dtype=F32)).astype(F32)
    s64 = scores.astype(np.float64)
    e64 = np.exp(s64 - s64.max(axis=-1, keepdims=True))
    p_t64 = e64 / e64.sum(axis=-1, keepdims=True) / np.float64(F32(pa.scale))
    p_idx = _index(p, pa).astype(np.int64)
    p_idx64 = np.clip(np.rint(p_t64) + np.float64(F32(pa.offset)), pa.qmin, pa.qmax).astype(np.int64)
    acc = decode_pv_sums(p_idx, iv, pa, pb)
    y, out_q = decode_pv_output(acc, pa, pb, po, o_in)
    return dict(k_new=k_new, v_new=v_new, iv=iv, scores=scores, p_idx=p_idx, p_idx64=p_idx64, p_t64=p_t64, acc=acc, y=y, out_q=out_q)


def decode_pv_sums(p_idx, iv, pa: QuantizerOracle, pb: QuantizerOracle, p_hi=None):
    """Exact p.v sums [heads, D] of one decode step: sum_t (ip - zp)(iv - zv) from the probability indices p_idx [heads, T] and the value
    indices iv [kv_heads, T, D] (0 .. 255; float64 products and sums of integers below 2^53: exact).  p_hi: per-position upper indices --
    then (lowest, highest) sums over every choice of indices between p_idx and p_hi (the sum is linear in each index)."""
    kv, T, D = iv.shape
    heads = p_idx.shape[0]
    w = np.asarray(iv, np.float64) - np.float64(pb.offset)
    pl = (np.asarray(p_idx, np.float64) - np.float64(pa.offset)).reshape(kv, heads // kv, T)
    mm = lambda a, b: np.rint(np.matmul(a, b)).astype(np.int64).reshape(heads, D)      # noqa: E731
    if p_hi is None:
        return mm(pl, w)
    ph = (np.asarray(p_hi, np.float64) - np.float64(pa.offset)).reshape(kv, heads // kv, T)
    wp, wn = np.maximum(w, 0.0), np.minimum(w, 0.0)
    return mm(pl, wp) + mm(ph, wn), mm(ph, wp) + mm(pl, wn)


def decode_pv_output(acc, pa: QuantizerOracle, pb: QuantizerOracle, po: QuantizerOracle, o_in: QuantizerOracle):
    """Exact p.v sums acc [heads, D] -> (pv output y [heads*D] fp32, o_proj's input image [heads*D] int8); monotone in acc."""
    alpha = F32(F32(pa.scale) * F32(pb.scale))
    y = po.forward((np.asarray(acc).astype(np.float64) * np.float64(alpha)).astype(F32)).reshape(-1)
    out_q = (_index(y, o_in).astype(np.int64) - 128).astype(np.int8)
    return y, out_q


def oproj_int_sums(w, w_zp, a8):
    """o_proj's exact split-K sums over an int8 image: sum_k w[n, k] a8[k] - w_zp[n] sum_k a8[k]  (w [N, K] int8, a8 [K] int8)."""
    a = np.asarray(a8).astype(np.int64)
    return np.asarray(w).astype(np.int64) @ a - np.asarray(w_zp).astype(np.int64) * a.sum()


# ----------------------------------------------------------------------------------------------
# a8 / a9 (one decode step)  mq_decode_gemv and mq_decode_head launch by launch
# ----------------------------------------------------------------------------------------------
U32 = 2.0 ** -24                 # unit roundoff of fp32


def _gamma(n):
    """gamma_n = n u / (1 - n u): the relative error bound of n fp32 roundings in a row (Higham, Lemma 3.1)."""
    return n * U32 / (1.0 - n * U32)


def _tie_dist(t):
    """Distance of each pre-rounding value t (float64) from the nearest rounding boundary (a half-integer)."""
    t = np.asarray(t, np.float64)
    return np.abs(np.abs(t - np.floor(t) - 0.5))


def _fq_div(v, g):
    """Division-form fake quant (the reference's, and the kernel's Grid.fq); g None: the grid is off."""
    if g is None:
        return np.asarray(v, F32)
    return dequantize_index(quantize_index(v, g.scale, g.offset, g.qmin, g.qmax), g.scale, g.offset)


def _inv(g):
    """1 / scale rounded to fp32, as mq_decode_pack_grids stores it."""
    return (F32(1.0) / F32(g.scale)).astype(F32)


def _fq_recip(v, g):
    """The GEMV epilogues' output quantizer in its reciprocal form: clamp(rint(v * fl(1/s)) + o) -> (q - o) s; fminf / fmaxf clamp."""
    v = np.asarray(v, F32)
    if g is None:
        return v
    q = (np.rint((v * _inv(g)).astype(F32)) + F32(g.offset)).astype(F32)
    q = np.minimum(np.maximum(q, F32(g.qmin)), F32(g.qmax))
    return ((q - F32(g.offset)).astype(F32) * F32(g.scale)).astype(F32)


def _wrap32(v):
    return (np.asarray(v, np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def decode_gemv_prologue(K, x=None, xq=None, norm_w=None, norm_bias=None, layernorm=0, norm_in=None, eps=0.0, a_grid=None,
                         o_acc=None, o_alpha=None, o_ct=None, o_bias=None, o_out=None):
    """The int8 activation image a mq_decode_gemv launch contracts, from the fields of mq_decode_gemv_args (grids: QuantizerOracle or
    None for an absent grid; norm_w is the already fake-quantised weight vector the engine passes).  Modes as the C entry picks them:
    xq -> the image as given (XM_I8); norm_w -> QRMSNorm / QLayerNorm (XM_NORM / XM_LNORM: norm_in fake quant, then the norm); else the
    fp32 row itself (XM_F32).  o_acc given (OPRE): the row is first x + Qo(fl(fl(float(acc + ct)) o_alpha) + o_bias)) in the kernel's
    order, Qo in the reciprocal form -- returned as x_mid, bit for bit.
    Returns a dict:
      image [K] int8      index - 128 on a_grid, with the norm evaluated in float64 (rint of t64: the exact image away from ties)
      rs int              sum of the image
      t64 [K] float64     the pre-rounding value of each index: (norm value in float64) / scale (None for XM_I8)
      tie [K] bool        where the kernel's fp32 norm may round to the neighbouring index: |t64| within the fp32 error bound of the
                          kernel's documented order (prologue reduction: <= 16 adds per thread, a 6-level DPP tree, 8 waves in turn)
                          of a rounding boundary
      x_mid [K] fp32      (OPRE) the activation row behind o_proj's epilogue and the residual add"""
    if xq is not None:
        img = np.asarray(xq, np.int8).reshape(-1)[:K].copy()
        return dict(image=img, rs=int(img.astype(np.int64).sum()), t64=None, tie=np.zeros(K, bool), x_mid=None)
    x = np.asarray(x, F32).reshape(-1)[:K].copy()
    x_mid = None
    if o_acc is not None:
        tt = _wrap32(np.asarray(o_acc, np.int64) + np.asarray(o_ct, np.int64))
        f = (tt.astype(F32) * np.asarray(o_alpha, F32)).astype(F32)
        f = (f + (np.asarray(o_bias, F32) if o_bias is not None else F32(0))).astype(F32)
        x = (x + _fq_recip(f, o_out)).astype(F32)
        x_mid = x.copy()
    n_red = 4 * ((K + 2047) // 2048) + 6 + 8       # adds on the longest path of the prologue's float reductions
    if norm_w is None:                             # XM_F32: the row itself
        v64, err = x.astype(np.float64), np.zeros(K)
    else:
        xi = _fq_div(x, norm_in).astype(np.float64)
        w = np.asarray(norm_w, F32).astype(np.float64)
        b = np.asarray(norm_bias, F32).astype(np.float64) if norm_bias is not None else None
        v64, err = _norm64(xi, w, b, bool(layernorm), float(F32(eps)), n_red)
    s, o = np.float64(F32(a_grid.scale)), np.float64(F32(a_grid.offset))
    t64 = v64 / s
    idx = np.clip(np.rint(t64) + o, a_grid.qmin, a_grid.qmax)
    bound = (err + U32 * np.abs(v64)) / s * (1.0 + 1e-6) + 1e-300   # + the quotient's rounding (div_by_scale is the IEEE quotient)
    tie = _tie_dist(t64) <= bound
    img = (idx.astype(np.int64) - 128).astype(np.int8)
    return dict(image=img, rs=int(img.astype(np.int64).sum()), t64=t64, tie=tie, x_mid=x_mid)


def _norm64(xi, w, b, layernorm, eps, n_red):
    """Norm value of an fp32 row in float64 and a per-element bound of the fp32 kernel's error against it, for a reduction whose
    longest accumulation path has n_red adds; then ((xi r + (-r mu)) w + b) (LayerNorm) or w (xi r) (RMS) in fp32 rounding.
    w / b None: no weight / bias (the head's optional affine)."""
    K = xi.shape[0]
    ax = np.abs(xi)
    if layernorm:
        mu = xi.sum() / K
        var = ((xi - mu) ** 2).sum() / K
        r = 1.0 / np.sqrt(var + eps)
        z = (xi - mu) * r
        e_mu = _gamma(n_red + 1) * ax.sum() / K
        dv = (_gamma(n_red + 4) * (var + e_mu ** 2) + e_mu ** 2) / (var + eps) + 2 * U32
        dr = dv / 2 + dv * dv + 3 * U32
        ez = dr * np.abs(z) + r * (1 + dr) * (e_mu + U32 * (ax + abs(mu) + e_mu))
        ez = ez + U32 * (np.abs(z) + ez)
    else:
        ms = (xi * xi).sum() / K
        r = 1.0 / np.sqrt(ms + eps)
        z = xi * r
        ez = _gamma(n_red + 5) * np.abs(z)          # squares, the reduction, / K, + eps, sqrt, 1 / ., x r
    v, ev = z, ez
    if w is not None:
        v = z * w
        ev = np.abs(w) * ez + U32 * (np.abs(v) + np.abs(w) * ez)
    if b is not None:
        v = v + b
        ev = ev + U32 * (np.abs(v) + ev)
    return v, ev


def decode_gemv_sums(image, w, w4=False):
    """Exact contractions sum_k w[n, k] image[k] (int64) of the launch's weight rows: w int8 [N, K] (index - 128) or, w4, packed unsigned
    nibbles [N, K / 2] (pack_w4's layout: 16-byte group g of a row holds k = 32 g + j in the low and 32 g + j + 16 in the high nibble
    of byte j).  Gate launches: rows 2i / 2i+1 are w1 / w3 row i; [N] in row order either way.  (float64 products and sums of integers
below 2^53: exact.)"""
    a = np.asarray(image, np.int64)
    wi = unpack_w4(w, 0) if w4 else np.asarray(w, np.int8)
    assert wi.shape[1] * 128 * 128 < 2 ** 53
    return np.rint(wi.astype(np.float64) @ a.astype(np.float64)).astype(np.int64)


def decode_gemv_epilogue(sums, rs, alpha, w_zp, col_term, bias=None, seg_end=None, out_grid=(None, None, None), resid=None, gate=False,
                         gate_act=0, gate_mid=None, gate_actout=None, gate_out=None):
    """The epilogue of mq_decode_gemv, bit for bit in fp32: tt = sum - zp rs + ct (int32 wraparound), e = fl(fl(float(tt) alpha) + bias)
    (two roundings, no fma); not gate: the output quantizer of row n's segment (seg_end) in the reciprocal form, then fl(resid + .);
    gate: fa / fb = Qout0 / Qout1 of rows 2i / 2i+1 (reciprocal form), QSiLU (gate_act 0: fa Qmid(1 / (1 + exp(-fa))) ) or QGELU
    (0.5 fa (1 + erf(fa / sqrt 2))), Qactout, the product with fb, and the index on gate_out (division form) - 128.
    Every quantizer is also evaluated in the reference's division form (qmodule.py): `y_div`, `gate_q_div`.
    Returns a dict: tt [N] int32, e [N] fp32, y [N or N / 2] fp32, y_div; gate: fa, fb, gate_q [N / 2] int8, gate_q_div, prod (fp32,
    what y holds in gate mode), and for the transcendental chain (exp / erf are not correctly rounded anywhere) the pre-rounding value
    of each quantizer in float64 (t_mid, t_act, t_out; None where the grid is off) and `tie`: where one of them lies within 2^-17
    relative of a rounding boundary, so that a different last bit of exp / erf may move gate_q by one."""
    sums = np.asarray(sums, np.int64)
    N = sums.shape[0]
    tt = _wrap32(sums - np.asarray(w_zp, np.int64) * np.int64(rs) + np.asarray(col_term, np.int64))
    e = (tt.astype(F32) * np.asarray(alpha, F32)).astype(F32)
    e = (e + (np.asarray(bias, F32) if bias is not None else F32(0))).astype(F32)
    out = dict(tt=tt, e=e)
    if not gate:
        s0, s1 = (seg_end if seg_end is not None else (N, N))
        rows = np.arange(N)
        seg = np.where(rows < s0, 0, np.where(rows < s1, 1, 2))
        y, y_div = e.copy(), e.copy()
        for k in range(3):
            m = seg == k
            y[m], y_div[m] = _fq_recip(e[m], out_grid[k]), _fq_div(e[m], out_grid[k])
        if resid is not None:
            r = np.asarray(resid, F32)
            y, y_div = (r + y).astype(F32), (r + y_div).astype(F32)
        out.update(y=y, y_div=y_div)
        return out
    ea, eb = e[0::2], e[1::2]
    fa, fb = _fq_recip(ea, out_grid[0]), _fq_recip(eb, out_grid[1])
    chain = _gate_chain(fa, fb, gate_act, gate_mid, gate_actout, gate_out)
    chain_div = _gate_chain(_fq_div(ea, out_grid[0]), _fq_div(eb, out_grid[1]), gate_act, gate_mid, gate_actout, gate_out)
    out.update(fa=fa, fb=fb, gate_q=chain["q"], prod=chain["prod"], y=chain["prod"], t_mid=chain["t_mid"], t_act=chain["t_act"],
               t_out=chain["t_out"], tie=chain["tie"], gate_q_div=chain_div["q"], y_div=chain_div["prod"], tie_div=chain_div["tie"])
    return out


def _gate_chain(fa, fb, act, g_mid, g_act, g_out):
    """The gate chain of decode_gemv_epilogue (see there): Qact(act(fa)) * fb -> index on g_out, with `tie` over the three quantizers.
    g_out None: the activation alone (prefill_act) -- prod is Qact(act(fa)) * fb, no product grid, q and t_out None."""
    tol = 2.0 ** -17

    def near(t):
        return _tie_dist(t) <= tol * np.abs(t) + 1e-30

    tie = np.zeros(fa.shape, bool)
    t_mid = t_act = None
    if act == 0:
        with np.errstate(over="ignore"):
            g = (F32(1.0) / (F32(1.0) + np.exp(-fa).astype(F32)).astype(F32)).astype(F32)
            g64 = 1.0 / (1.0 + np.exp(-fa.astype(np.float64)))
        if g_mid is not None:
            t_mid = g64 / np.float64(F32(g_mid.scale))
            tie |= near(t_mid)
        rr = (fa * _fq_div(g, g_mid)).astype(F32)
        rr64 = fa.astype(np.float64) * (_fq_div(g, g_mid).astype(np.float64) if g_mid is not None else g64)
    else:
        from scipy.special import erf
        h = (fa * F32(0.70710678118654752440)).astype(F32)
        rr = ((F32(0.5) * fa).astype(F32) * (F32(1.0) + erf(h.astype(np.float64)).astype(F32)).astype(F32)).astype(F32)
        rr64 = 0.5 * fa.astype(np.float64) * (1.0 + erf(fa.astype(np.float64) / np.sqrt(2.0)))
    if g_act is not None:
        t_act = rr64 / np.float64(F32(g_act.scale))
        tie |= near(t_act)
        a64 = _fq_div(rr, g_act).astype(np.float64)
    else:
        a64 = rr64
    prod = (_fq_div(rr, g_act) * fb).astype(F32)
    if g_out is None:                              # the activation alone (prefill_act): no product grid behind it
        return dict(q=None, prod=prod, t_mid=t_mid, t_act=t_act, t_out=None, tie=tie)
    t_out = a64 * fb.astype(np.float64) / np.float64(F32(g_out.scale))
    tie |= near(t_out)
    qi = quantize_index(prod, g_out.scale, g_out.offset, g_out.qmin, g_out.qmax)
    qi = np.where(np.isnan(qi), F32(g_out.qmin), qi)
    q = (qi.astype(np.int64) - 128).astype(np.int8)
    return dict(q=q, prod=prod, t_mid=t_mid, t_act=t_act, t_out=t_out, tie=tie)


def decode_gemv_launch(K, N, w, alpha, w_zp, col_term, w4=False, gate=False, bias=None, seg_end=None, out_grid=(None, None, None),
                       resid=None, gate_act=0, gate_mid=None, gate_actout=None, gate_out=None, **prologue):
    """One mq_decode_gemv launch from the fields of mq_decode_gemv_args: decode_gemv_prologue (the image and its row sum) ->
    decode_gemv_sums -> decode_gemv_epilogue.  Returns the epilogue's dict plus image, rs, t64, tie_image (the prologue's `tie`), x_mid."""
    pro = decode_gemv_prologue(K, **prologue)
    sums = decode_gemv_sums(pro["image"], w, w4)
    assert sums.shape[0] == N
    out = decode_gemv_epilogue(sums, pro["rs"], alpha, w_zp, col_term, bias, seg_end, out_grid, resid, gate, gate_act, gate_mid,
                               gate_actout, gate_out)
    out.update(image=pro["image"], rs=pro["rs"], t64=pro["t64"], tie_image=pro["tie"], x_mid=pro["x_mid"], sums=sums)
    return out


def decode_head_norm(x, norm_w=None, norm_b=None, layernorm=0, eps=1e-5):
    """mq_decode_head's activation row in float64 and a per-element bound of the kernel's fp32 error on it: final RMSNorm
    (w (x r), r = 1 / sqrt(mean(x^2) + eps); no weight: x itself, unnormalised) or LayerNorm (x r + (-r mu), then * w, + b, each
    optional).  The kernel's reductions: ceil(K / 256) adds per thread, a 6-level DPP tree, then (s0 + s1) + (s2 + s3).
    Returns (s64 [K], err [K])."""
    x = np.asarray(x, F32).reshape(-1).astype(np.float64)
    K = x.shape[0]
    n_red = (K + 255) // 256 + 6 + 2
    w = np.asarray(norm_w, F32).astype(np.float64) if norm_w is not None else None
    b = np.asarray(norm_b, F32).astype(np.float64) if norm_b is not None else None
    if not layernorm and w is None:
        return x, np.zeros(K)
    return _norm64(x, w, b if layernorm else None, bool(layernorm), float(F32(eps)), n_red)


def decode_head_logits(w64, s64, err, bias64=None):
    """Logits of rows of the fp32 lm_head in float64 and a per-logit bound of the kernel's fp32 error: w64 [R, K] float64 rows (numpy or
    torch: only @, abs and arithmetic are used), s64 / err [K] from decode_head_norm (same array type).  The kernel's dot product:
    one rounded product per term, 4 ceil(K / 256) terms added in order per lane, a 6-level DPP tree, then fl(acc + bias).
    Returns (logits64 [R], bound [R])."""
    K = s64.shape[0]
    n = 4 * ((K + 255) // 256) + 6
    aw = abs(w64)
    lg = w64 @ s64
    mag = aw @ (abs(s64) + err)
    bound = aw @ err + _gamma(n) * mag + K * 2.0 ** -52 * mag        # (the last term: this float64 evaluation's own rounding)
    if bias64 is not None:
        lg = lg + bias64
        bound = bound + U32 * (abs(lg) + bound)
    return lg, bound


# ----------------------------------------------------------------------------------------------
# a10 (prefill, by rows)  rows of attention_sim(exact_int=True) for one sequence, and the kernel's error envelope
# ----------------------------------------------------------------------------------------------
def prefill_attention_rows(q, k, v, cos, sin, heads, kv_heads, qk: tuple, pv: tuple, rows, qkv_idx=None, in_grids=None):
    """The requested query rows of attention_sim(..., exact_int=True) for one sequence of S positions, without an S x S tensor: the
    cost is rows x S.  q [S, heads*D], k / v [S, kv_heads*D] fp32 before RoPE -- or qkv_idx uint8 [S, (heads + 2 kv_heads) * D] with
    in_grids = (q_in, k_in, v_in) (anything with .scale / .offset): each segment reads (idx - o) * s in fp32, as mq_attention_quant
    does.  cos / sin [S, rot_dim]; qk = (input, input2, output) and pv = (input, input2, output) QuantizerOracles (qk[2] / pv[2] may be
    None); rows: absolute query positions.  Returns a dict (R = len(rows), T = S: keys past a row are masked):
      ik8 / iv8 [kv, S, D] int8       the K / V images (index - 128) of every position
      acc_qk [heads, R, T] int64      sum_d (iq - zq)(ik - zk), exact (0 where masked)
      t64 [heads, R, T] float64       pre-rounding score index acc alpha / s_out + o (qk[2] None: acc alpha / sqrt(D), the value)
      s_idx [heads, R, T] fp32        the reference's division-form score index (qk[2] None: the fp32 score)
      scores [heads, R, T] fp32       qk_bmm output / sqrt(D), -inf where masked
      p [heads, R, T] fp32            softmax in attention_sim's order (row of length S, masked terms 0, numpy's fp32 row sum)
      p64 [heads, R, T] float64       softmax of the same scores in float64
      p_idx / p_idx64 [heads, R, T]   pv.input indices of p / p64 (int64; masked keys: the zero point)
      acc [heads, R, D] int64         sum_t (ip - zp)(iv - zv), exact
      y [R, heads*D] fp32             pv_bmm's output (rows of attention_sim)
      out_idx [R, heads*D]            its index on pv[2] (None when pv[2] is None)"""
    qa, qb, qo = qk
    pa, pb, po = pv
    rows = np.asarray(rows, np.int64)
    H, KV = int(heads), int(kv_heads)
    if qkv_idx is not None:
        idx = np.asarray(qkv_idx)
        S = idx.shape[0]
        D = idx.shape[1] // (H + 2 * KV)
        idx = idx.reshape(S, H + 2 * KV, D).astype(F32)
        q, k, v = (dequantize_index(idx[:, a:b], g.scale, g.offset).reshape(S, -1)
                   for (a, b), g in zip(((0, H), (H, H + KV), (H + KV, H + 2 * KV)), in_grids))
    S = np.asarray(k).shape[0]
    D = np.asarray(q).shape[1] // H
    cos, sin = np.asarray(cos, F32), np.asarray(sin, F32)
    kr = rope_partial(np.asarray(k, F32).reshape(S, KV, D).transpose(1, 0, 2), cos, sin)
    ik = _index(kr, qb)                                                               # [kv, S, D]
    iv = _index(np.asarray(v, F32).reshape(S, KV, D).transpose(1, 0, 2), pb)
    qr = rope_partial(np.asarray(q, F32)[rows].reshape(len(rows), H, D).transpose(1, 0, 2), cos[rows], sin[rows])
    iq = _index(qr, qa)                                                               # [heads, R, D]
    rep, R = H // KV, len(rows)
    acc_qk = np.matmul((iq.astype(np.float64) - np.float64(qa.offset)).reshape(KV, rep * R, D),
                       (ik.astype(np.float64) - np.float64(qb.offset)).transpose(0, 2, 1))
    acc_qk = np.rint(acc_qk).astype(np.int64).reshape(H, R, S)
    live = np.arange(S)[None, None, :] <= rows[None, :, None]
    acc_qk = np.where(live, acc_qk, 0)
    alpha_qk = F32(F32(qa.scale) * F32(qb.scale))
    sqrt_d = F32(np.sqrt(F32(D)))
    x32 = (acc_qk.astype(F32) * alpha_qk).astype(F32)
    if qo is not None:
        t64 = acc_qk.astype(np.float64) * np.float64(alpha_qk) / np.float64(F32(qo.scale)) + np.float64(F32(qo.offset))
        s_idx = _index(x32, qo)
        sval = dequantize_index(s_idx, qo.scale, qo.offset)
        v64 = (s_idx.astype(np.float64) - np.float64(F32(qo.offset))) * np.float64(F32(qo.scale)) / np.sqrt(np.float64(D))
    else:
        t64 = acc_qk.astype(np.float64) * np.float64(alpha_qk) / np.sqrt(np.float64(D))
        s_idx = sval = x32
        v64 = t64
    scores = np.where(live, (sval / sqrt_d).astype(F32), F32(-np.inf)).astype(F32)
    att = (scores - scores.max(axis=-1, keepdims=True)).astype(F32)
    e = np.exp(att, dtype=F32)
    p = (e / e.sum(axis=-1, keepdims=True, dtype=F32)).astype(F32)
    v64 = np.where(live, v64, -np.inf)
    e64 = np.exp(v64 - v64.max(axis=-1, keepdims=True))
    p64 = e64 / e64.sum(axis=-1, keepdims=True)
    p_idx = _index(p, pa).astype(np.int64)
    p_idx64 = np.clip(np.rint(p64 / np.float64(F32(pa.scale))) + np.float64(F32(pa.offset)), pa.qmin, pa.qmax).astype(np.int64)
    acc = decode_pv_sums(p_idx.reshape(H * R, S), iv, pa, pb).reshape(H, R, D)
    alpha_pv = F32(F32(pa.scale) * F32(pb.scale))
    pre = (acc.astype(np.float64) * np.float64(alpha_pv)).astype(F32)
    y = po.forward(pre) if po is not None else pre
    out_idx = _index(pre, po) if po is not None else None
    lay = lambda a: a.transpose(1, 0, 2).reshape(R, H * D)                          # noqa: E731  [heads, R, D] -> [R, heads*D]
    return dict(ik8=(ik.astype(np.int64) - 128).astype(np.int8), iv8=(iv.astype(np.int64) - 128).astype(np.int8), iv=iv, rows=rows,
                acc_qk=acc_qk, t64=t64, s_idx=s_idx, scores=scores, p=p, p64=p64, p_idx=p_idx, p_idx64=p_idx64, acc=acc,
                y=lay(y), out_idx=None if out_idx is None else lay(out_idx), live=live, D=D)


def prefill_fixed_ref(qo, D):
    """mq_attention_quant's choice of the grid top as the exponent reference: a score grid whose span is < 96 in exp2 units."""
    if qo is None:
        return False
    inv = {64: F32(0.125), 128: F32(0.08838834764831845), 256: F32(0.0625)}[D]
    cexp = F32(F32(F32(qo.scale) * inv) * F32(1.4426950408889634))
    flo, fhi = F32(12582912.0) + F32(qo.qmin), F32(12582912.0) + F32(qo.qmax)
    return bool(F32(F32(fhi - flo) * cexp) < F32(96.0))


EXP2_ULP = 8          # assumed error of v_exp_f32, in ulp of its result (unmeasured on gfx950; the ISA documents 1 ulp)


def prefill_envelope(r, qk: tuple, pv: tuple, exp2_ulp: int = EXP2_ULP):
    """Sound per-output range for mq_attention_quant on the rows of r = prefill_attention_rows(...): every output index the kernel may
    produce given its documented rounding points, and every one attention_sim's fp32 order produces.  Interval arithmetic in float64
    (u = 2^-24; relative errors below are bounds, each counted generously):
      * Score index.  The kernel evaluates rint(ti beta + o) as fma(float(ti), beta, o + 1.5 2^23) clamped by med3, with
        beta = fl(fl(s_a s_b) fl(1 / s_out)); the reference divides: rint(fl(fl(ti) alpha) / s_out) + o.  Both are rint of
        t = ti alpha / s_out times (1 + d), |d| <= 3u, + u once |ti| >= 2^24 (ti -> float).  So the index lies in
        [ceil(t - e|t| - 1/2), floor(t + e|t| + 1/2)] + o: both neighbours where t lies within e|t| of a half-integer.  Without an output
        grid the score value itself carries 4u (head_dim 128: RN(1 / sqrt 128) against fl(sqrt 128)).
      * Exponentials.  exp2(fma(f, cexp, -R)): cexp = fl(fl(s_out / sqrt D) log2e) carries <= 3u; with f = magic + index the fma is exact
        up to its result's rounding, so the argument x_t (log2 distance from R: the grid top when fixed_ref, the row maximum otherwise)
        is off by <= 4u |x_t|; v_exp_f32 adds exp2_ulp ulp (2u each: an assumption, not a measurement).  The reference rounds each fp32
        score (2u |s_t|) and s_t - max (u |s_t - max|) and calls numpy's expf (covered by the same ulp allowance).  So e_t carries
        a_t = 8u (ln2 |x_t| + |s_t| + |s_max|) + 2u exp2_ulp + 4u.
      * Row sum l.  16 terms per lane per key block in order, one partial per block into the lane's l (running form: l * exp2(R - Rn)
        + bs, two roundings), two cross-lane adds: at most n = 2 nkb + 24 roundings on the path of any term (numpy's pairwise row sum
        needs fewer): gamma_n.  Each rescale of the running form multiplies by one more v_exp_f32 result: (2u exp2_ulp + 2u) per
        rescale, counted per row as the blocks whose highest score can exceed every lower score before them.
      * p index.  rp = fl(fl(1 / s_p) / l), rint(fma(e, rp, zp + magic)): e rp carries 2u beyond e / (l s_p); the reference's fl(e / sum)
        and fl(p / s_p) as much.  t_p = p / s_p lies in [E_lo (1 - a) / L_hi, E_hi (1 + a) / L_lo] / s_p (1 -+ 4u), the index in
        [ceil(lo - 1/2), floor(hi + 1/2)] + zp, clamped.  Masked keys: exactly zp.
      * Output.  The exact sums over each p index range (decode_pv_sums(p_hi=...)); the double product with fl(s_p s_v) rounded once,
        as the kernel and the reference do; then the index in both the division form (reference) and a_index_fast's reciprocal form,
        the lower of both at the low end and the higher at the high end (all four are monotone in the sum).  pv_out None: the fp32
        interval of the pre-quantizer value.
    Returns dict(p_lo, p_hi [heads, R, T], acc_lo, acc_hi [heads, R, D], lo, hi [R, heads*D] (indices, or fp32 values without an
    output grid), n_amb_score, n_amb_p)."""
    qa, qb, qo = qk
    pa, pb, po = pv
    u = 2.0 ** -24
    D, live, acc_qk, rows = r["D"], r["live"], r["acc_qk"], r["rows"]
    H, R, S = acc_qk.shape
    big = np.abs(acc_qk) >= 2 ** 24
    alpha = np.float64(F32(F32(qa.scale) * F32(qb.scale)))
    sd = np.sqrt(np.float64(D))
    if qo is not None:
        so, oo = np.float64(F32(qo.scale)), np.float64(F32(qo.offset))
        t = acc_qk * alpha / so
        e = (3 * u + u * big) * np.abs(t)
        j_lo = np.clip(np.ceil(t - e - 0.5) + oo, qo.qmin, qo.qmax)
        j_hi = np.clip(np.floor(t + e + 0.5) + oo, qo.qmin, qo.qmax)
        sv_lo, sv_hi = (j_lo - oo) * so / sd, (j_hi - oo) * so / sd
        n_amb_score = int(((j_hi != j_lo) & live).sum())
    else:
        t = acc_qk * alpha / sd
        e = (4 * u + u * big) * np.abs(t)
        sv_lo, sv_hi = t - e, t + e
        n_amb_score = 0
    sv_lo, sv_hi = np.where(live, sv_lo, -np.inf), np.where(live, sv_hi, -np.inf)
    M = sv_hi.max(axis=-1, keepdims=True)
    log2e, ln2 = 1.0 / np.log(2.0), np.log(2.0)
    fixed = prefill_fixed_ref(qo, D)
    x = np.where(live, (M - sv_lo) * log2e, 0.0)
    if fixed:
        x = np.maximum(x, np.where(live, (qo.qmax - j_lo) * so / sd * log2e, 0.0))
    a = 8 * u * (ln2 * x + np.abs(np.where(live, sv_hi, 0.0)) + np.abs(M)) + 2 * u * exp2_ulp + 4 * u
    E_lo = np.where(live, np.exp(sv_lo - M), 0.0) * (1 - a)
    E_hi = np.where(live, np.exp(sv_hi - M), 0.0) * (1 + a)
    nkb = rows // 64 + 1                                                              # [R]
    gam = (2 * nkb + 24) * u / (1 - (2 * nkb + 24) * u)
    if fixed:
        n_r = np.zeros((H, R))
    else:                                                                             # blocks that may raise the running maximum
        nb = S // 64 if S % 64 == 0 else S // 64 + 1
        pad = nb * 64 - S
        bl = np.pad(sv_lo, ((0, 0), (0, 0), (0, pad)), constant_values=-np.inf).reshape(H, R, nb, 64).max(-1)
        bh = np.pad(sv_hi, ((0, 0), (0, 0), (0, pad)), constant_values=-np.inf).reshape(H, R, nb, 64).max(-1)
        run = np.maximum.accumulate(bl, axis=-1)
        n_r = ((bh[..., 1:] > run[..., :-1]) & (bh[..., 1:] > -np.inf)).sum(-1).astype(np.float64)
    er = n_r * (2 * u * exp2_ulp + 2 * u)
    L_lo = E_lo.sum(-1) * (1 - gam[None]) * (1 - er)
    L_hi = E_hi.sum(-1) * (1 + gam[None]) * (1 + er)
    sp, zp = np.float64(F32(pa.scale)), np.float64(F32(pa.offset))
    tp_lo = E_lo / L_hi[..., None] / sp * (1 - 4 * u) - 1e-12
    tp_hi = E_hi / L_lo[..., None] / sp * (1 + 4 * u) + 1e-12
    p_lo = np.where(live, np.clip(np.ceil(tp_lo - 0.5) + zp, pa.qmin, pa.qmax), zp).astype(np.int64)
    p_hi = np.where(live, np.clip(np.floor(tp_hi + 0.5) + zp, pa.qmin, pa.qmax), zp).astype(np.int64)
    acc_lo, acc_hi = decode_pv_sums(p_lo.reshape(H * R, S), r["iv"], pa, pb, p_hi=p_hi.reshape(H * R, S))
    acc_lo, acc_hi = acc_lo.reshape(H, R, D), acc_hi.reshape(H, R, D)
    alpha_pv = np.float64(F32(F32(pa.scale) * F32(pb.scale)))
    pre_lo, pre_hi = ((a_.astype(np.float64) * alpha_pv).astype(F32) for a_ in (acc_lo, acc_hi))
    if po is not None:
        def recip(x):
            inv = (F32(1.0) / F32(po.scale)).astype(F32)
            return np.clip((np.rint((x * inv).astype(F32)) + F32(po.offset)).astype(F32), F32(po.qmin), F32(po.qmax))
        lo = np.minimum(_index(pre_lo, po), recip(pre_lo))
        hi = np.maximum(_index(pre_hi, po), recip(pre_hi))
    else:
        lo, hi = pre_lo, pre_hi
    lay = lambda z: z.transpose(1, 0, 2).reshape(R, H * D)                          # noqa: E731
    return dict(p_lo=p_lo, p_hi=p_hi, acc_lo=acc_lo, acc_hi=acc_hi, lo=lay(lo), hi=lay(hi), n_amb_score=n_amb_score,
                n_amb_p=int(((p_hi != p_lo) & live).sum()))


# ----------------------------------------------------------------------------------------------
# a10 (prefill, element-wise)  mq_rmsnorm_quant / mq_layernorm_quant, mq_act_quant and the gated-activation routes
# ----------------------------------------------------------------------------------------------
def prefill_norm_n_red(cols):
    """Adds on the longest path of the float reductions of mq_norm.hip's launch for rows of `cols` floats, branch by branch
    (launch_norm).  A thread owns the float4 vectors lane, lane + TPR, ... of its row and adds their four squares one after the other
    into one accumulator: 4 ceil(nvec / TPR) sequential adds, nvec = cols / 4 (a slot past the row's end is skipped, so this is at
    most 4 V for the register forms and 4 ceil(nvec / 256) on the re-read path; LayerNorm's sum of (x + y) + (z + w) per vector and
    its four squared deviations per vector are no longer).  Then the six levels of wave_sum_f_readlane (four DPP steps inside a
    16-lane row, then (r0 + r1) + (r2 + r3)), then block_sum4's (s0 + s1) + (s2 + s3) where a workgroup owns the row:
      cols < 1024            V = 4, TPR = 64 (a wave per row)     4 ceil(nvec / 64) + 6       <= 22
      cols <= 1024           V = 1, TPR = 256                     4 + 6 + 2                   =  12
      cols <= 2048           V = 2                                8 + 6 + 2                   =  16
      cols <= 4096           V = 4                                16 + 6 + 2                  =  24
      cols <= 8192           V = 8                                32 + 6 + 2                  =  40
      beyond (re-read)       V = 0                                4 ceil(nvec / 256) + 6 + 2     (12288: 56)
    norm_tiled8_kernel<V, LN, GRPS> (1024 <= cols <= 4096) runs the arithmetic of the TPR = 256 form of its V in either GRPS."""
    nvec = int(cols) // 4
    tpr = 64 if cols < 1024 else 256
    return 4 * ((nvec + tpr - 1) // tpr) + 6 + (0 if tpr == 64 else 2)


def f32_between(lo, hi):
    """Every fp32 value in [lo, hi] (0 < lo <= hi finite, float64), ascending: consecutive bit patterns."""
    a, b = F32(lo), F32(hi)
    if np.float64(a) < lo:
        a = np.nextafter(a, F32(np.inf))
    if np.float64(b) > hi:
        b = np.nextafter(b, F32(-np.inf))
    ia, ib = int(a.view(np.uint32)), int(b.view(np.uint32))
    return np.arange(ia, ib + 1, dtype=np.uint32).view(F32)


def prefill_norm_rows(x, weight, bias, eps, layernorm, in_q, out_q, q_shift, n_red):
    """mq_rmsnorm_quant / mq_layernorm_quant row by row in float64: x [rows, cols] fp32, weight the (already fake-quantised) vector the
    kernel is given, bias or None, in_q / out_q QuantizerOracles or None.  The input quantizer is the reference's division form in fp32
    (bit-exact: it is element-wise); the norm of each row is _norm64 with the reduction depth n_red (prefill_norm_n_red(cols): the
    derivation is there), so `err` bounds the fp32 kernel's |value - v64| element by element.
    Returns a dict ([rows, cols] unless noted; the index fields are None without an output grid):
      xi      fp32     the input-quantised row the kernel normalises
      v64     float64  the norm value;  err  float64  the fp32 error bound on it
      t64     float64  v64 / scale: the pre-rounding value on the output grid
      idx     float64  clip(rint(t64) + offset, qmin, qmax)  (NaN where v64 is)
      q8      int8     idx - q_shift, NaN -> qmin - q_shift (the kernel's integer image);  rs [rows] int64 its row sums
      tie     bool     _tie_dist(t64) within (err + u |v64|) / scale: the kernel's fp32 value may round to the neighbouring index (the
                       quotient's own rounding is the u |v64| term: div_by_scale is the IEEE quotient)
      r64 [rows] float64   (RMS) 1 / sqrt(mean(xi^2) + eps);  r_err [rows]: bound of |r - r64| for the kernel's fp32
                       r = fl(1 / fl(sqrt(fl(fl(ss / cols) + eps)))): ss carries gamma(n_red + 1) (the squares' rounding and the adds; all terms
                       positive), / cols and + eps one u each -> gamma(n_red + 3) under the root, which halves it (to first order; the
                       factor 1.001 covers the second), + u for the root and + u for the reciprocal."""
    x = np.asarray(x, F32)
    rows, cols = x.shape
    with np.errstate(all="ignore"):
        xi = _fq_div(x, in_q).astype(F32)
        w = np.asarray(weight, F32).astype(np.float64)
        b = np.asarray(bias, F32).astype(np.float64) if bias is not None else None
        e = float(F32(eps))
        v64, err = np.empty((rows, cols)), np.empty((rows, cols))
        for i in range(rows):
            v64[i], err[i] = _norm64(xi[i].astype(np.float64), w, b, bool(layernorm), e, n_red)
        out = dict(xi=xi, v64=v64, err=err, t64=None, idx=None, q8=None, rs=None, tie=None, r64=None, r_err=None)
        if not layernorm:
            x64 = xi.astype(np.float64)
            r64 = 1.0 / np.sqrt((x64 * x64).sum(axis=1) / cols + e)
            out.update(r64=r64, r_err=r64 * (_gamma(n_red + 3) / 2 + 2 * U32) * 1.001)
        if out_q is None:
            return out
        s, o = np.float64(F32(out_q.scale)), np.float64(F32(out_q.offset))
        t64 = v64 / s
        idx = np.clip(np.rint(t64) + o, out_q.qmin, out_q.qmax)
        bound = (err + U32 * np.abs(v64)) / s * (1.0 + 1e-6) + 1e-300
        tie = _tie_dist(t64) <= bound
        st = np.where(np.isnan(idx), np.float64(out_q.qmin), idx) - q_shift
    q8 = st.astype(np.int64).astype(np.int8)
    out.update(t64=t64, idx=idx, q8=q8, rs=q8.astype(np.int64).sum(axis=1), tie=tie)
    return out


def prefill_norm_replay(xi, r, shift, weight, bias, layernorm, out_q, q_shift):
    """The `emit` of mq_norm.hip in fp32, op for op, given the row scalars: xi [..., cols] fp32 (prefill_norm_rows' xi), r and shift
    fp32 (scalars, or [..., 1]).  RMS: fl(w fl(xi r)); LayerNorm: fl(fl(fl(xi r) + shift) w); + bias; then the value-form index
    (quantize_index: NaN stays NaN), y = dequant(index), and the integer image index - q_shift with NaN -> qmin.  No approximation:
    every operation is one IEEE fp32 operation in the kernel's order.  Returns dict(y fp32, idx fp32 | None, q8 int8 | None,
    rs int64 [...] | None); without an output grid y is the norm value itself."""
    xi, r, w = np.asarray(xi, F32), np.asarray(r, F32), np.asarray(weight, F32)
    with np.errstate(all="ignore"):
        z = (xi * r).astype(F32)
        if layernorm:
            y = ((z + np.asarray(shift, F32)).astype(F32) * w).astype(F32)
        else:
            y = (w * z).astype(F32)
        if bias is not None:
            y = (y + np.asarray(bias, F32)).astype(F32)
        if out_q is None:
            return dict(y=y, idx=None, q8=None, rs=None)
        idx = quantize_index(y, out_q.scale, out_q.offset, out_q.qmin, out_q.qmax)
        yq = dequantize_index(idx, out_q.scale, out_q.offset)
    q8 = (np.where(np.isnan(idx), F32(out_q.qmin), idx).astype(np.int64) - int(q_shift)).astype(np.int8)
    return dict(y=yq, idx=idx, q8=q8, rs=q8.astype(np.int64).sum(axis=-1))


def prefill_act(x, act, in_q, mid_q, out_q):
    """mq_act_quant (QSiLU act 0 / QGELU act 1): xi = Qin(x), then _gate_chain's activation with b = 1 and no product grid.  Returns
    dict(y fp32, xi, t_mid, t_act (float64 pre-rounding values, None where the grid is off), tie)."""
    with np.errstate(all="ignore"):
        xi = _fq_div(np.asarray(x, F32), in_q).astype(F32)
        c = _gate_chain(xi, np.ones_like(xi), int(act), mid_q, out_q, None)
    return dict(y=c["prod"], xi=xi, t_mid=c["t_mid"], t_act=c["t_act"], tie=c["tie"])


def prefill_gate(y1, vb, out_q, q_shift):
    """The gated FFN's product behind an OBSERVED activation value: prod = fl(y1 vb) (ElementwiseMul is not quantised), w2's input
    index in the division form and its integer image index - q_shift, NaN -> qmin (mq_activation.hip gated_store).  Broadcasts.
    Returns dict(prod fp32, idx fp32 (NaN kept), q8 int8)."""
    with np.errstate(all="ignore"):
        prod = (np.asarray(y1, F32) * np.asarray(vb, F32)).astype(F32)
        idx = quantize_index(prod, out_q.scale, out_q.offset, out_q.qmin, out_q.qmax)
    q8 = (np.where(np.isnan(idx), F32(out_q.qmin), idx).astype(np.int64) - int(q_shift)).astype(np.int8)
    return dict(prod=prod, idx=idx, q8=q8)


# ----------------------------------------------------------------------------------------------
# a12 (calibration passes)  mq_calib_attention_probs(_causal), mq_calib_norm, mq_calib_gated, mq_calib_rope(_qkv)  (csrc/mq_reduce.hip)
# ----------------------------------------------------------------------------------------------
def calib_probs(raw, inv_sqrt_d, mask=None, causal=False):
    """The calibration score chain (hf_model.py:513-530): raw [rows, cols] fp32, inv_sqrt_d = float32(1 / float32(sqrt_d)), mask None or an
    additive fp32 [mask_rows, cols] (row r takes mask[r % mask_rows]), causal: square blocks of cols rows, row r masks the columns
    > r % cols.  x is formed op for op in fp32 -- ONE rounded multiply, then ONE rounded add of the mask or of the causal -inf / 0 -- and the
    softmax of that fp32 x is float64: exp(x - max x) / sum.  Row disposition: a row whose x holds a NaN or +inf, or no finite entry at
    all (max x = -inf: every x - max is inf - inf), is NaN in every entry -- torch's softmax and the kernel alike; -inf entries of any
    other row are exactly 0.  Returns dict(x fp32, p float64 (NaN rows all-NaN), nan_row bool [rows], masked bool: x == -inf)."""
    raw = np.asarray(raw, F32)
    rows, cols = raw.shape
    with np.errstate(all="ignore"):
        x = (raw * F32(inv_sqrt_d)).astype(F32)
        if mask is not None:
            m = np.asarray(mask, F32)
            x = (x + m[np.arange(rows) % m.shape[0]]).astype(F32)
        if causal:
            above = np.arange(cols)[None, :] > (np.arange(rows) % cols)[:, None]
            x = (x + np.where(above, F32(-np.inf), F32(0))).astype(F32)
        mx = x.max(axis=1)                                            # np.max propagates NaN
        nan_row = np.isnan(mx) | np.isinf(mx)                         # NaN inside, +inf inside (inf - inf), or nothing but -inf
        x64 = x.astype(np.float64)
        e = np.exp(x64 - np.where(nan_row, 0.0, mx.astype(np.float64))[:, None])
        p = e / e.sum(axis=1, keepdims=True)
        p[nan_row] = np.nan
    return dict(x=x, p=p, nan_row=nan_row, masked=np.isneginf(x))


def calib_norm_n_red(cols, layernorm):
    """(n_mu, n_r): fp32 roundings on the longest path of calib_norm_kernel<VPT, LN>'s two row sums, VPT = 1 | 2 | 4 | 8 for cols <= 1024 |
    2048 | 4096 | 8192.  A thread forms a 4-term sum per float4, (a + b) + (c + d): 2 adds; adds it into its accumulator: VPT adds;
    wave_sum_f_readlane: 6 levels; the four wave partials (s0 + s1) + (s2 + s3): 2 -- VPT + 10 adds.
      mean (LayerNorm)      the terms are h itself:                         n_mu = VPT + 10, + 1 for the divide by cols
      sum of squares (RMS)  + 1 for each square's rounding:                 n_r  = VPT + 11
      squared deviations    + 1 for d = fl(h - mu), squared (2 u), rounded: n_r  = VPT + 13
    Under the root come / cols and + eps (one u each): gamma(n_r + 2), which the root halves; + u for the root, + u for the reciprocal."""
    vpt = 1 if cols <= 1024 else 2 if cols <= 2048 else 4 if cols <= 4096 else 8
    return vpt + 11, vpt + (13 if layernorm else 11)


def calib_norm_r_width(n_r):
    """Relative half-width of the fp32 r = fl(1 / fl(sqrt(fl(fl(ss / cols) + eps)))) around its float64 value: gamma(n_r + 2) / 2 + 2 u (the
    factor 1.001 covers the second-order terms); the candidates number at most 2 width / u + 1 <= n_r + 8 (fp32 spacing >= u |r|)."""
    return (_gamma(n_r + 2) / 2 + 2 * U32) * 1.001


def calib_norm_candidates(h_row, eps, layernorm, cols=None):
    """The fp32 row scalars mq_calib_norm can have formed for one row h (fp32): a list of (mu fp32, r candidates fp32 array).  RMS: mu = 0
    and every fp32 r within calib_norm_r_width of float64 1 / sqrt(mean(h^2) + eps).  LayerNorm: every fp32 mu within
    gamma(n_mu) sum|h| / cols of the float64 mean (the sum's error is relative to sum|h|, not to the mean), and for EACH of them the r
    candidates around float64 1 / sqrt(mean((h - mu)^2) + eps) with that fp32 mu."""
    h64 = np.asarray(h_row, F32).astype(np.float64)
    cols = h64.size if cols is None else cols
    n_mu, n_r = calib_norm_n_red(cols, layernorm)
    e, w = float(F32(eps)), calib_norm_r_width(n_r)
    if not layernorm:
        r64 = 1.0 / np.sqrt((h64 * h64).sum() / cols + e)
        return [(F32(0), f32_between(r64 * (1 - w), r64 * (1 + w)))]
    m64, a = h64.sum() / cols, _gamma(n_mu) * 1.001 * np.abs(h64).sum() / cols
    lo, hi = m64 - a, m64 + a
    assert lo > 0.0 or hi < 0.0, "calib_norm_candidates: the row mean's error interval holds 0 -- no finite candidate list"
    mus = f32_between(lo, hi) if lo > 0.0 else -f32_between(-hi, -lo)[::-1]
    out = []
    for mu in mus:
        d = (np.asarray(h_row, F32) - mu).astype(F32).astype(np.float64)
        r64 = 1.0 / np.sqrt((d * d).sum() / cols + e)
        out.append((mu, f32_between(r64 * (1 - w), r64 * (1 + w))))
    return out


def calib_norm_emit(h_row, mu, r, weight, bias, layernorm):
    """calib_norm_kernel's elementwise expression in fp32, op for op: RMS fl(w fl(h r)); LayerNorm fl(fl(fl(h - mu) r) w) (+ bias)."""
    h, w = np.asarray(h_row, F32), np.asarray(weight, F32)
    with np.errstate(all="ignore"):
        if not layernorm:
            return (w * (h * F32(r)).astype(F32)).astype(F32)
        y = (((h - F32(mu)).astype(F32) * F32(r)).astype(F32) * w).astype(F32)
        return (y + np.asarray(bias, F32)).astype(F32) if bias is not None else y


def calib_norm_rows(x, delta, weight, bias, eps, layernorm, candidates=True):
    """mq_calib_norm: h = fl(x + delta) (fp32, bit for bit), the float64 norm y64 of each row of h, and each row's candidate list.
    err bounds |y - y64| of the fp32 kernel element by element (the row scalars' widths of calib_norm_candidates pushed through the
    elementwise expression).  Returns dict(h fp32, y64, err float64, cand: per row a list of (mu, r array), None without `candidates`)."""
    x = np.asarray(x, F32)
    h = (x + np.asarray(delta, F32)).astype(F32) if delta is not None else x
    h64, w64 = h.astype(np.float64), np.asarray(weight, F32).astype(np.float64)
    e, cols = float(F32(eps)), h.shape[1]
    n_mu, n_r = calib_norm_n_red(cols, layernorm)
    wr = calib_norm_r_width(n_r)
    if layernorm:
        d = h64 - h64.mean(axis=1, keepdims=True)
        r64 = 1.0 / np.sqrt((d * d).mean(axis=1, keepdims=True) + e)
        t64 = d * r64 * w64
        a_mu = _gamma(n_mu) * 1.001 * np.abs(h64).sum(axis=1, keepdims=True) / cols
        y64 = t64 + np.asarray(bias, F32).astype(np.float64) if bias is not None else t64
        # mu moves d by a_mu (and r, through the variance, by less than a_mu r^2 |mean d| = 0 to first order: doubled instead), then
        # fl(h - mu), the two products and the bias add: 4 u
        err = (np.abs(t64) * (wr + 4 * U32) + 2 * a_mu * r64 * np.abs(w64)) * 1.01 + 2 * U32 * np.abs(y64)
    else:
        y64 = w64 * (h64 / np.sqrt((h64 * h64).mean(axis=1, keepdims=True) + e))
        err = np.abs(y64) * (wr + 3 * U32) * 1.01
    return dict(h=h, y64=y64, err=err + 1e-45, cand=None if not candidates else [calib_norm_candidates(h[i], eps, layernorm) for i in range(h.shape[0])])


def calib_norm_replay(y_row, h_row, cand, weight, bias, layernorm, probe=16):
    """The (mu, r) pairs of `cand` whose calib_norm_emit equals y_row bit for bit (NaN never matches).  The first `probe` columns sift the
    pairs, the survivors are replayed over the whole row.  Returns the list of matching (mu, r)."""
    y, h, w = np.asarray(y_row, F32), np.asarray(h_row, F32), np.asarray(weight, F32)
    b = np.asarray(bias, F32) if bias is not None else None
    k = min(probe, y.size)
    hits = []
    for mu, rs in cand:
        for r in rs:
            if np.array_equal(calib_norm_emit(h[:k], mu, r, w[:k], b[:k] if b is not None else None, layernorm).view(np.uint32), y[:k].view(np.uint32)) \
                    and np.array_equal(calib_norm_emit(h, mu, r, w, b, layernorm).view(np.uint32), y.view(np.uint32)):
                hits.append((mu, r))
    return hits


def _erf64(x):
    import math
    u, inv = np.unique(np.asarray(x, np.float64), return_inverse=True)
    return np.frompyfunc(math.erf, 1, 1)(u).astype(np.float64)[inv].reshape(np.shape(x))


def calib_gated(a, b, act):
    """mq_calib_gated in float64: act 0 SiLU a / (1 + exp(-a)), act 1 GELU a (1 + erf(a / sqrt 2)) / 2.  Returns (act(a) * b, act(a))."""
    a64, b64 = np.asarray(a, F32).astype(np.float64), np.asarray(b, F32).astype(np.float64)
    with np.errstate(all="ignore"):
        s = a64 / (1.0 + np.exp(-a64)) if int(act) == 0 else 0.5 * a64 * (1.0 + _erf64(a64 / np.sqrt(2.0)))
    return s * b64, s


def repeat_kv(x, rep):
    """x [B, KV, S, D] -> [B, KV * rep, S, D], every head rep times in a row (hf_model.py:509-510): index arithmetic."""
    return np.repeat(np.asarray(x), int(rep), axis=1)


def calib_rope(x_lin, heads, head_dim, cos, sin, rotate=True, rep=1):
    """One segment of mq_calib_rope(_qkv): x_lin [B, S, heads * D] as the linear wrote it -> [B, heads * rep, S, D], the first rot dims
    rotated with cos / sin [S, rot] (rope_partial: two rounded products and one rounded sum) when `rotate`, every head rep times."""
    x = np.asarray(x_lin, F32)
    B, S = x.shape[:2]
    x = x.reshape(B, S, heads, head_dim).transpose(0, 2, 1, 3)
    if rotate:
        x = rope_partial(x, np.asarray(cos, F32), np.asarray(sin, F32)).astype(F32)
    return np.ascontiguousarray(repeat_kv(x, rep))


# ----------------------------------------------------------------------------------------------
# a7 (prefill)  the GEMM family's fused epilogues   csrc/mq_gemm.hip, tools/gen_fr_asm.py
# ----------------------------------------------------------------------------------------------
def fma_f32(a, b, c):
    """The correctly rounded fp32 of a * b + c for fp32 arrays (v_fma_f32, __builtin_fmaf), finite results.

    The float64 product of two fp32 values is exact (48 significant bits); the float64 sum s = p + c is not, and float32(s) can round
    twice.  TwoSum gives the sum's residual e exactly (p + c = s + e).  float32(s) is wrong only where s lies exactly on the midpoint
    of two neighbouring fp32 values and e != 0: a float64 that is no midpoint is at least one float64 ulp away from every midpoint,
    |e| is at most half of one, so s + e is on the same side of every midpoint as s.  On a midpoint the sign of e decides."""
    a64, b64, c64 = (np.asarray(v, F32).astype(np.float64) for v in (a, b, c))
    p = a64 * b64
    s = p + c64
    bb = s - p
    e = (p - (s - bb)) + (c64 - bb)                   # TwoSum (Knuth): exact residual of the float64 add
    r = s.astype(F32)
    d = s - r.astype(np.float64)                      # exact: r is the fp32 next to s
    other = np.nextafter(r, np.where(d > 0, F32(np.inf), F32(-np.inf)).astype(F32)).astype(F32)
    midpoint = (d != 0) & (s == (r.astype(np.float64) + other.astype(np.float64)) * 0.5)
    toward_other = midpoint & (e != 0) & ((e > 0) == (d > 0))
    # on a midpoint with e == 0 the tie is real and r (ties-to-even) stands; with e pointing back to r, r stands as well
    return np.where(toward_other, other, r).astype(F32)


def prefill_gemm_acc(a_idx, w_idx, a_rowsum, w_zp, col_term):
    """int32 [M, N]: wrap32(a . w^T - w_zp[n] * a_rowsum[m] + col_term[n]), what the accumulators hold in front of every prefill GEMM
    epilogue (they START at the zero-point correction, in int32 wrap-around arithmetic, and the MFMAs add the contraction).  a_idx
    [M, K] and w_idx [N, K] are the stored integers (packed 4-bit weights: the unsigned nibbles).  The contraction is a float64 BLAS
    product, exact below 2^53 as in qlinear_int_exact(blas=True).  a_rowsum None: no correction term (the caller guarantees w_zp == 0)."""
    a = np.asarray(a_idx)
    w = np.asarray(w_idx)
    assert a.shape[1] == w.shape[1] and a.shape[1] * 255 * 255 < 2 ** 53
    acc = np.rint(a.astype(np.float64) @ w.astype(np.float64).T).astype(np.int64)
    zp = np.asarray(w_zp, np.int64).reshape(1, -1)
    if a_rowsum is not None:
        acc = acc - zp * np.asarray(a_rowsum, np.int64).reshape(-1, 1)
    else:
        assert not zp.any(), "a_rowsum None needs w_zp == 0"
    return _wrap32(acc + np.asarray(col_term, np.int64).reshape(1, -1))


PREFILL_GEMM_STORAGE = {"f32": np.float32, "f16": np.float16, "u8": np.uint8, "i8": np.int8, "u16": np.uint16, "i16": np.int16}


def prefill_gemm_columns(N, grids, seg_end):
    """(scale fp32 [N], offset fp32 [N]): grids = [(scale, offset)] per column segment, seg_end their increasing ends (the last is N; a
    single segment may come without ends)."""
    ends = [int(N)] if len(grids) == 1 else [int(v) for v in seg_end]
    assert len(ends) == len(grids) and ends[-1] == N and all(b > a for a, b in zip([0] + ends, ends))
    sc, oo = np.empty(N, F32), np.empty(N, F32)
    lo = 0
    for (s, o), hi in zip(grids, ends):
        sc[lo:hi], oo[lo:hi] = F32(s), F32(o)
        lo = hi
    return sc, oo


def prefill_gemm_epilogue(t, alpha, bias=None, grids=None, seg_end=None, out_qmin=0, out_qmax=255, out_dtype="f32", resid=None):
    """What every prefill GEMM stores for the int32 accumulators t [M, N] (prefill_gemm_acc), one rounding per step: the C++ epilogue
    of gemm_i8_kernel and the generated one of tools/gen_fr_asm.py are the same fixed sequence of correctly rounded fp32 operations
    (the library is built with -ffp-contract=off).  Returns (stored [M, N] in the storage type, q float64, tie float64): q is the value
    in front of the rounding to an index (the fma's fp32 result; without a grid, the fp32 output) and tie its distance to the nearest
    half-integer, so that a failure can say how close to a rounding boundary the element was.

    grids None (f32 / f16 output only):  fl(fl(float(t) * alpha) + bias), bias 0.0f when absent; f16 rounds once more.
    grids = [(scale, offset)] per column segment (prefill_gemm_columns), per column n:
        inv = fl(1 / scale),  A' = fl(alpha * inv),  B' = fl(bias * inv) (bias 0.0f when absent),
        B' = fl(B' + offset)  when out_qmax - out_qmin <= 255 (the offset rides in the addend for EVERY storage type),
        q  = fma(float(t), A', B')   with float(t) = int32 -> fp32, round to nearest even (v_cvt_f32_i32),
        r  = rint(q) (to even);  r = fl(r + offset) when the offset was not folded;  r = clamp(r, out_qmin, out_qmax).
    Storage: u8 the index (saturated to 0..255, what v_cvt_pk_u8_f32 does); i8 on the grid 0..255 byte ^ 0x80 (= index - 128), on
    any other grid int & 0xff; u16 / i16 int & 0xffff; f32 / f16 fl(fl(r - offset) * scale), f16 rounded once more.  resid (f32
    only): fl(resid + y).

    Where this differs from the plain reading of "clamp(round(v / scale) + offset)": the kernels multiply by the rounded reciprocal and
    fold alpha and the bias into it BEFORE the contraction's value is known, so v itself is never formed.  The unsigned 8-bit fast path
    (grid 0..255, u8 / i8 storage) has no rint and no clamp instruction: v_cvt_pk_u8_f32 rounds to nearest even and saturates, which
    is the same function.  A dequantised output (f32 / f16) takes scale and offset of the FIRST grid only: the kernels read column
    segments for u8 / i8 storage alone, and the entry points pass them nowhere else."""
    t = np.asarray(t)
    assert t.dtype == np.int32 and t.ndim == 2
    N = t.shape[1]
    tf = t.astype(F32)                                             # int32 -> fp32, round to nearest even
    al = np.asarray(alpha, F32).reshape(1, N)
    bs = np.zeros((1, N), F32) if bias is None else np.asarray(bias, F32).reshape(1, N)
    st = PREFILL_GEMM_STORAGE[out_dtype]
    if grids is None:
        assert out_dtype in ("f32", "f16")
        with np.errstate(over="ignore"):
            v = ((tf * al).astype(F32) + bs).astype(F32)
        q = v.astype(np.float64)
    else:
        qmin, qmax = F32(out_qmin), F32(out_qmax)
        fold = (qmax - qmin) <= F32(255.0)
        assert len(grids) == 1 or out_dtype in ("u8", "i8"), "column segments: index outputs only"
        sc, oo = prefill_gemm_columns(N, grids, seg_end)
        inv = (F32(1.0) / sc).astype(F32).reshape(1, N)
        oo = oo.reshape(1, N)
        a1 = (al * inv).astype(F32)
        b1 = (bs * inv).astype(F32)
        if fold:
            b1 = (b1 + oo).astype(F32)
        qf = fma_f32(tf, np.broadcast_to(a1, tf.shape), np.broadcast_to(b1, tf.shape))
        q = qf.astype(np.float64)
        r = np.rint(qf).astype(F32)
        if not fold:
            r = (r + oo).astype(F32)
        r = np.minimum(np.maximum(r, qmin), qmax)
        ri = r.astype(np.int64)
        if out_dtype == "u8":
            v = np.clip(ri, 0, 255).astype(np.uint8)
        elif out_dtype == "i8":
            v = ((np.clip(ri, 0, 255) ^ 0x80) if out_qmin == 0 else (ri & 0xFF)).astype(np.uint8).view(np.int8)
        elif out_dtype in ("u16", "i16"):
            v = (ri & 0xFFFF).astype(np.uint16).view(st)
        else:
            v = ((r - oo).astype(F32) * sc.reshape(1, N)).astype(F32)
    if out_dtype in ("f32", "f16"):
        if resid is not None:
            assert out_dtype == "f32"
            v = (np.asarray(resid, F32) + v).astype(F32)
        with np.errstate(over="ignore"):
            v = v.astype(st)
    return v, q, _tie_dist(q)


def prefill_gemm_gated(ia, ib, table):
    """w2's int8 input image from the gated pair: table[ia * 256 + ib] for w1's indices ia and w3's indices ib (u8 [M, N]; table int8
    [65536], mq_gated_table).  Returns (image int8 [M, N] row-major, (bytes int8 [ceil16(M) * N], real bool) in the fragment-blocked
    layout of tiled_image_bytes, row sums int32 [M])."""
    ia, ib = np.asarray(ia).astype(np.int64), np.asarray(ib).astype(np.int64)
    assert ia.shape == ib.shape and ia.min() >= 0 and ib.min() >= 0 and ia.max() <= 255 and ib.max() <= 255
    img = np.asarray(table, np.int8).reshape(-1)[ia * 256 + ib]
    return img, tiled_image_bytes(img, *img.shape), img.astype(np.int64).sum(axis=1).astype(np.int32)


# ----------------------------------------------------------------------------------------------
# a13 (training passes)  mq_fake_quant_backward, mq_lwc_fake_quant(_backward), mq_attention_probs_train(_backward)  (csrc/mq_fake_quant.hip)
# ----------------------------------------------------------------------------------------------
EXPF_ULP = 1          # ASSUMED error of the device expf, in ulp of its result: the vendor's math-API tables document 1 ulp; not measured, not
#                       fitted to any kernel output.  An ulp is charged at its largest relative size, 2^-23 = 2 u.
TRAIN_MUTATION = None  # tests only: "half_away" | "trunc" | "exclusive_mask" | "tie_one" | "mask_no_mod" make the functions below deliberately wrong
P_ABS = 2.0 ** -125   # absolute allowance on exp() for results below the normal range (flushed or denormal)


def _mutation(m):
    return TRAIN_MUTATION if m is None else m


def _rint_m(t, m):
    if m == "half_away":
        return (np.sign(t) * np.floor(np.abs(t) + 0.5)).astype(t.dtype)
    if m == "trunc":
        return np.trunc(t)
    return np.rint(t)


def fq_point(x, s, o, qmin, qmax, mutation=None):
    """The fake-quant expression tree at every element, fp32 op for op (fake_quant_bwd_kernel's names): t = x / s (IEEE), r = round_ste(t)
    = (rint(t) - t) + t, q = r + o, inside = qmin <= q <= qmax (inclusive: torch.clamp's backward mask), qc = clamp(q) with NaN kept,
    y = (qc - o) * s.  Returns (t, r, inside, qc, y)."""
    m = _mutation(mutation)
    x, s, o = np.asarray(x, F32), np.asarray(s, F32), np.asarray(o, F32)
    with np.errstate(all="ignore"):
        t = (x / s).astype(F32)
        r = ((_rint_m(t, m) - t).astype(F32) + t).astype(F32)
        q = (r + o).astype(F32)
        inside = ((q > F32(qmin)) & (q < F32(qmax))) if m == "exclusive_mask" else ((q >= F32(qmin)) & (q <= F32(qmax)))
        qc = np.clip(q, F32(qmin), F32(qmax)).astype(F32)
        y = ((qc - o).astype(F32) * s).astype(F32)
    return t, r, inside, qc, y


def fake_quant_backward_terms(x, grad_y, scale, offset, qmin, qmax, mutation=None):
    """fake_quant_backward with the sums left open: grad_x bit for bit (inside ? (g * s) / s : 0), and the fp32 TERMS of the two sums exactly
    as every kernel forms them -- ts = inside ? g * (r - t) : g * (qc - o), to = inside ? 0 : -g * s, one rounded product each (r - t and,
    for grids of at most 2^24 steps, qc - o are exact).  A kernel's grad_scale / grad_offset is some fp32 summation of these terms: within
    gamma_n * sum|term| of their float64 sum, n the adds on its longest path.  scale / offset: 0-d, or [rows, 1] against x [rows, cols]."""
    g, s, o = np.asarray(grad_y, F32), np.asarray(scale, F32), np.asarray(offset, F32)
    t, r, inside, qc, _ = fq_point(x, s, o, qmin, qmax, mutation)
    with np.errstate(all="ignore"):
        gx = np.where(inside, ((g * s).astype(F32) / s).astype(F32), F32(0)).astype(F32)
        ts = np.where(inside, (g * (r - t).astype(F32)).astype(F32), (g * (qc - o).astype(F32)).astype(F32)).astype(F32)
        to = np.where(inside, F32(0), (-g * s).astype(F32)).astype(F32)
    return dict(gx=gx, ts=ts, to=to, inside=inside, t=t, r=r)


def lwc_grid(mn, mx, sig_lo, sig_hi, qmax, is_symmetric):
    """lwc_grid of the fused pass, fp32 op for op: lo = sig_lo * mn, hi = sig_hi * mx (qmodule.py:271-273), alpha = max(|lo|, |hi|) (NaN
    kept) or hi - lo, scale = clamp(alpha / qmax) with the TRUE quotient and NaN kept, offset = -rint(beta / scale) (qmodule.py:40-61)."""
    with np.errstate(all="ignore"):
        lo, hi = (np.asarray(sig_lo, F32) * mn).astype(F32), (np.asarray(sig_hi, F32) * mx).astype(F32)
        if is_symmetric:
            alpha, beta = np.maximum(np.abs(lo), np.abs(hi)), np.zeros_like(lo)
        else:
            alpha, beta = (hi - lo).astype(F32), lo
        raw = (alpha / F32(qmax)).astype(F32)
        scale = np.clip(raw, CLIPMIN, CLIPMAX).astype(F32)
        offset = (-np.rint((beta / scale).astype(F32))).astype(F32)
    return dict(lo=lo, hi=hi, alpha=alpha, raw=raw, scale=scale, offset=offset)


def lwc_fused_forward(w, sig_lo, sig_hi, bitwidth, is_symmetric):
    """mq_lwc_fused's forward on its own interface (the sigmoids, not the factors; lwc_forward is the same expression behind sigmoid_f32):
    row amin / amax with NaN propagated, lwc_grid, the fake-quant.  Everything fp32 op for op -- every output is exact."""
    w = np.asarray(w, F32)
    qmin, qmax = qrange(bitwidth, is_symmetric)
    mn, mx = w.min(axis=1), w.max(axis=1)                                  # np.min / np.max propagate NaN, as amin / amax do
    g = lwc_grid(mn, mx, sig_lo, sig_hi, qmax, is_symmetric)
    y = fq_point(w, g["scale"][:, None], g["offset"][:, None], qmin, qmax)[4]
    return dict(y=y, row_min=mn, row_max=mx, scale=g["scale"], offset=g["offset"])


def lwc_fused_backward(w, grad_y, sig_lo, sig_hi, row_min, row_max, bitwidth, is_symmetric, mutation=None):
    """mq_lwc_fake_quant_backward.  Exact part: gx = inside ? (g * s) / s : 0 -- grad_w wherever the element is no row extreme.  Behind the
    row sum S = sum(ts) (terms as in fake_quant_backward_terms) everything is LINEAR in S: g_alpha = S / qmax where CLIPMIN <= alpha / qmax
    <= CLIPMAX (bounds included) and exactly 0 elsewhere; alpha = hi - lo gives (g_lo, g_hi) = (-g_alpha, g_alpha), alpha = max(|lo|, |hi|)
    gives the larger one g_alpha sign(.) and a tie half each; grad_sig_lo = g_lo mn, grad_sig_hi = g_hi mx; the extreme elements receive
    g_lo sig_lo / n_mn and g_hi sig_hi / n_mx, n the number of elements EQUAL to the extreme (ties share evenly, +0 == -0).  Returned in
    float64 with the factors c (value = c * S) so that a bound gamma_n * |c| * sum|ts| can be formed; NaN / inf follow IEEE through the
    same expression (0 * NaN = NaN: a NaN row has grad_sig NaN and grad_w exactly 0)."""
    m = _mutation(mutation)
    w, g = np.asarray(w, F32), np.asarray(grad_y, F32)
    qmin, qmax = qrange(bitwidth, is_symmetric)
    mn, mx = np.asarray(row_min, F32), np.asarray(row_max, F32)
    slo, shi = np.asarray(sig_lo, F32), np.asarray(sig_hi, F32)
    gd = lwc_grid(mn, mx, slo, shi, qmax, is_symmetric)
    b = fake_quant_backward_terms(w, g, gd["scale"][:, None], gd["offset"][:, None], qmin, qmax, m)
    ts = b["ts"].astype(np.float64)
    with np.errstate(all="ignore"):
        S, sumabs = ts.sum(axis=1), np.abs(ts).sum(axis=1)
        passes = (gd["raw"] >= CLIPMIN) & (gd["raw"] <= CLIPMAX)
        c_alpha = np.where(passes, 1.0 / qmax, 0.0)
        if is_symmetric:
            alo, ahi = np.abs(gd["lo"]).astype(np.float64), np.abs(gd["hi"]).astype(np.float64)
            c_lo = c_alpha * np.where(alo > ahi, 1.0, np.where(alo == ahi, 0.5, 0.0)) * np.sign(np.nan_to_num(gd["lo"], nan=0.0))
            c_hi = c_alpha * np.where(ahi > alo, 1.0, np.where(alo == ahi, 0.5, 0.0)) * np.sign(np.nan_to_num(gd["hi"], nan=0.0))
        else:
            c_lo, c_hi = -c_alpha, c_alpha
        Sz = np.where(passes, S, 0.0)                                        # the kernel selects 0 there, whatever S is
        is_mn, is_mx = w == mn[:, None], w == mx[:, None]
        if m == "tie_one":                                                   # wrong on purpose: the first of several tied elements takes it all
            is_mn = is_mn & (np.cumsum(is_mn, axis=1) == 1)
            is_mx = is_mx & (np.cumsum(is_mx, axis=1) == 1)
        n_mn, n_mx = is_mn.sum(axis=1).astype(np.float64), is_mx.sum(axis=1).astype(np.float64)
        c_add_mn, c_add_mx = c_lo * slo / n_mn, c_hi * shi / n_mx
        g_sig_lo, g_sig_hi = (c_lo * Sz) * mn, (c_hi * Sz) * mx
        c_sig_lo, c_sig_hi = np.abs(c_lo * mn.astype(np.float64)), np.abs(c_hi * mx.astype(np.float64))
        scat = np.where(is_mn, (c_add_mn * Sz)[:, None], 0.0) + np.where(is_mx, (c_add_mx * Sz)[:, None], 0.0)
        c_scat = np.where(is_mn, np.abs(c_add_mn)[:, None], 0.0) + np.where(is_mx, np.abs(c_add_mx)[:, None], 0.0)
    return dict(gx=b["gx"], ts=b["ts"], S=S, sumabs=sumabs, extreme=is_mn | is_mx, grad_w=b["gx"].astype(np.float64) + scat, c_scat=c_scat,
                grad_sig_lo=g_sig_lo, grad_sig_hi=g_sig_hi, c_sig_lo=c_sig_lo, c_sig_hi=c_sig_hi, passes=passes, scale=gd["scale"],
                offset=gd["offset"])


def train_attn_probs(raw, mask, grid1, grid2, sqrt_d, n_sum, mutation=None):
    """mq_attention_probs_train: Q2(softmax(Q1(raw) / sqrt_d + mask)), grid = (scale, offset, qmin, qmax), mask None or additive fp32
    [mask_rows, cols] (row r takes mask[r % mask_rows]).  x is fp32 op for op -- Q1's output has the same bits in the kernel's FAST and
    !FAST bodies (the fast quotient is the IEEE one from |t| = 1/4 up and r = 0 below either way), one rounded division by sqrt_d (an
    exact multiplication by its reciprocal when sqrt_d is a power of two), one rounded add of the mask.  The softmax of that x is float64,
    rows disposed of as in calib_probs.  t2 = p / s2 in float64 and the Q2 index from it.
    env: bound on the relative error of the kernel's fp32 p: fl(x - max) moves the exponent by u |x - max|, expf by EXPF_ULP ulp (2 u
    each), both again as the p-weighted row mean through the sum l, gamma_n_sum for l's summation path (n_sum adds: the caller counts them
    from the launch geometry), one division.  et: the absolute error of the kernel's t2 (its quotient: 2 u more).  An element is
    UNDECIDED when t2 lies within et of a half-integer: the kernel may return either neighbour (out / out_alt); edge: such an element
    straddles a Q2 clamp edge (cases are re-seeded until there is none)."""
    m = _mutation(mutation)
    raw = np.asarray(raw, F32)
    rows, cols = raw.shape
    s1, o1, qmin1, qmax1 = grid1
    s2, o2, qmin2, qmax2 = grid2
    s1, o1, s2, o2 = F32(s1), F32(o1), F32(s2), F32(o2)
    t1, r1, in1, qc1, y1 = fq_point(raw, s1, o1, qmin1, qmax1, m)
    with np.errstate(all="ignore"):
        x = (y1 / F32(sqrt_d)).astype(F32)
        if mask is not None:
            mk = np.asarray(mask, F32)
            ri = np.minimum(np.arange(rows), mk.shape[0] - 1) if m == "mask_no_mod" else np.arange(rows) % mk.shape[0]
            x = (x + mk[ri]).astype(F32)
        mx = x.max(axis=1)
        nan_row = np.isnan(mx) | np.isinf(mx)
        d = x.astype(np.float64) - np.where(nan_row, 0.0, mx.astype(np.float64))[:, None]
        e = np.exp(d)
        p = e / e.sum(axis=1, keepdims=True)
        p[nan_row] = np.nan
        a = np.where(np.isfinite(d), U32 * np.abs(d) + 2 * U32 * EXPF_ULP, 0.0)
        env = 1.001 * (a + np.nansum(p * a, axis=1)[:, None] + _gamma(n_sum) + U32)
        t2 = p / np.float64(s2)
        et = (env + 2 * U32) * t2 + P_ABS / np.float64(s2)
        r2 = _rint_m(t2, m)
        undecided = _tie_dist(t2) <= et
        r2_alt = np.where(t2 >= r2, r2 + 1.0, r2 - 1.0)

        def q2(r):
            q = r + np.float64(o2)
            ins = ((q > qmin2) & (q < qmax2)) if m == "exclusive_mask" else ((q >= qmin2) & (q <= qmax2))
            qc = np.clip(q, qmin2, qmax2)
            return ins, qc, ((qc.astype(F32) - o2).astype(F32) * s2).astype(F32)
        in2, qc2, out = q2(r2)
        in2_alt, _, out_alt = q2(r2_alt)
        edge = undecided & (in2 != in2_alt)
    return dict(x=x, p=p, env=env, et=et, t2=t2, r2=r2, in2=in2, qc2=qc2, out=out, out_alt=out_alt, undecided=undecided, edge=edge,
                nan_row=nan_row, masked=np.isneginf(x), t1=t1, r1=r1, in1=in1, qc1=qc1)


def train_attn_probs_backward(raw, grad_out, mask, grid1, grid2, sqrt_d, n_sum, mutation=None):
    """mq_attention_probs_train_backward in float64 on train_attn_probs' p, with first-order error envelopes (times 1.01 for the second
    order) of what the kernel's fp32 chain may return:
      Q2 backward  gp = inside2 ? (g s2) / s2 : 0 (3 u); d s2 terms g (r2 - t2) | g (qc2 - o2), error |g| et + u |term|, an undecided
                   element |g| more; d o2 terms -g s2 outside.
      softmax      dot = sum(gp p): sum |gp p| (env + 4 u) + gamma_n_sum sum |gp p|; ga = p (gp - dot).
      / sqrt_d     gs, one rounding.
      Q1 backward  grad_raw = inside1 ? (gs s1) / s1 : exactly 0; d s1 terms gs (r1 - t1) | gs (qc1 - o1) (the fast body's t1 is within an
                   ulp below 1/4: 3 u on the term), d o1 terms -gs s1 outside.
    Returns grad_raw, e_raw [rows, cols], terms / errs: the four [rows, cols] term arrays (d s1, d o1, d s2, d o2) and their error arrays,
    and prod = gp p with e_dot per row.  NaN rows carry NaN through the same expressions (inside is false for a NaN index)."""
    f = train_attn_probs(raw, mask, grid1, grid2, sqrt_d, n_sum, mutation)
    s1, o1 = np.float64(F32(grid1[0])), np.float64(F32(grid1[1]))
    s2, o2 = np.float64(F32(grid2[0])), np.float64(F32(grid2[1]))
    g = np.asarray(grad_out, F32).astype(np.float64)
    p, env, in1, in2 = f["p"], f["env"], f["in1"], f["in2"]
    sd = np.float64(F32(sqrt_d))
    with np.errstate(all="ignore"):
        ts2 = np.where(in2, g * (f["r2"] - f["t2"]), g * (f["qc2"] - o2))
        e_ts2 = np.where(in2, np.abs(g) * f["et"], 0.0) + U32 * np.abs(ts2) + np.where(f["undecided"], np.abs(g), 0.0)
        to2 = np.where(in2, 0.0, -g * s2)
        e_to2 = U32 * np.abs(to2)
        gp = np.where(in2, g, 0.0)
        prod = gp * p
        dot = prod.sum(axis=1)
        e_dot = (np.abs(prod) * (env + 4 * U32)).sum(axis=1) + _gamma(n_sum) * np.abs(prod).sum(axis=1)
        diff = gp - dot[:, None]
        e_diff = 3 * U32 * np.abs(gp) + e_dot[:, None] + U32 * np.abs(diff)
        ga = p * diff
        e_ga = p * e_diff + np.abs(ga) * (env + U32) + P_ABS * np.abs(diff)
        gs = ga / sd
        e_gs = e_ga / sd + U32 * np.abs(gs)
        graw = np.where(in1, gs, 0.0)
        e_raw = np.where(in1, e_gs + 3 * U32 * np.abs(gs), 0.0)
        w1 = np.where(in1, f["r1"].astype(np.float64) - f["t1"].astype(np.float64), f["qc1"].astype(np.float64) - o1)
        ts1 = gs * w1
        e_ts1 = e_gs * np.abs(w1) + 3 * U32 * np.abs(ts1)
        to1 = np.where(in1, 0.0, -gs * s1)
        e_to1 = np.where(in1, 0.0, e_gs * s1 + U32 * np.abs(to1))
    return dict(fwd=f, grad_raw=graw, e_raw=1.01 * e_raw, terms=(ts1, to1, ts2, to2), errs=tuple(1.01 * v for v in (e_ts1, e_to1, e_ts2, e_to2)),
                prod=prod, dot=dot, e_dot=1.01 * e_dot, p=p, gp=gp)


# ----------------------------------------------------------------------------------------------
# a10 / a8 (pins)  mq_qmatmul (csrc/mq_qmatmul.hip) and mq_w8a8_linear_grouped (csrc/mq_gemm_grouped.hip), op for op
# ----------------------------------------------------------------------------------------------
QMATMUL_MUTATIONS = ("scale64", "in_half_up", "out_half_up", "nan_qmax", "no_zero_row")
GROUPED_MUTATIONS = ("mul_add", "reverse", "bracket_f64")
QMATMUL_MUTATION = None   # tests only (like TRAIN_MUTATION): a name from the lists above makes every call without its own `mutation` wrong on purpose
GROUPED_MUTATION = None


def _rint_half_up(t):
    """floor(t + 1/2) for fp32 t, exact in float64 (wrong on purpose: ties go up instead of to even); NaN / inf pass."""
    t64 = np.asarray(t, F32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(t64) < 2.0 ** 52, np.floor(t64 + 0.5), t64).astype(F32)


def image_index(x, grid, mutation=None):
    """int64 indices of an integer IMAGE (csrc/mq_quant.h index_image_nan2qmin): clamp(rint(x / s) + o), the logic of quantize_storage
    with shift 0 -- where the reference's index is NaN (x NaN or +-inf: round_ste's inf - inf; an overflowing quotient) the index is
    qmin.  grid = (scale, offset, qmin, qmax) per tensor.  mutation "in_half_up": ties up; "nan_qmax": NaN becomes qmax."""
    s, o, qmin, qmax = grid
    x = np.asarray(x, F32)
    with np.errstate(all="ignore"):
        t = (x / F32(s)).astype(F32)
        rt = _rint_half_up(t) if mutation == "in_half_up" else np.rint(t)
        r = ((rt - t).astype(F32) + t).astype(F32)
        idx = np.clip((r + F32(o)).astype(F32), F32(qmin), F32(qmax))
    return np.where(np.isnan(idx), F32(qmax if mutation == "nan_qmax" else qmin), idx).astype(np.int64)


def qmatmul_launch(x1, x2, g1, g2, g_out, mutation=None):
    """What one mq_qmatmul launch stores, op for op, knowing nothing of kernels, routes or tiles.  x1 [batch, M, K], x2 [batch, K, N]
    fp32 (the LOGICAL operand, whichever memory order the call uses); g1 / g2 / g_out = (scale, offset, qmin, qmax), g_out None for no
    output quantizer.
      ia, ib   image_index: clamp(rint(x / s) + o), NaN -> qmin
      t        sum_k (ia - rint(o1))(ib - rint(o2)) in exact integers (a float64 contraction below 2^53, asserted)
      domain   |rint(o)| >= 2^20 for either operand: every output is NaN
      v        x1 of at most 8 bits (qmax - qmin <= 255): fl32(t), then ONE fp32 multiply by alpha = fl32(s1 s2);
               a wider x1: fl32(float64(t) * float64(alpha))
      out      the reference's output quantizer (qmodule.py:286-290) op for op: q = v / s (IEEE), r = (rint(q) - q) + q (round_ste:
               +-inf -> NaN), idx = clamp(r + o) with NaN kept, (idx - o) * s.
    Returns dict(out fp32 [batch, M, N], t int64, alpha, v fp32, q fp32 | None, tie float64 | None: the distance of q to a half step,
    idx fp32 | None, ia, ib).  mutation (tests only) makes it deliberately wrong: QMATMUL_MUTATIONS."""
    mutation = QMATMUL_MUTATION if mutation is None else mutation
    assert mutation is None or mutation in QMATMUL_MUTATIONS, mutation
    x1, x2 = np.asarray(x1, F32), np.asarray(x2, F32)
    assert x1.ndim == 3 and x2.ndim == 3 and x1.shape[0] == x2.shape[0] and x1.shape[2] == x2.shape[1]
    ia, ib = image_index(x1, g1, mutation), image_index(x2, g2, mutation)
    z1, z2 = np.rint(F32(g1[1])), np.rint(F32(g2[1]))
    sane = bool(abs(z1) < 2.0 ** 20 and abs(z2) < 2.0 ** 20)
    a1 = ia.astype(np.float64) - (np.float64(z1) if sane else 0.0)
    b1 = ib.astype(np.float64) - (np.float64(z2) if sane else 0.0)
    assert x1.shape[2] * np.abs(a1).max() * np.abs(b1).max() < 2.0 ** 53
    t = np.rint(np.matmul(a1, b1)).astype(np.int64)
    if mutation == "no_zero_row":                                # the term -z2 sum_k (ia - z1) is lost
        t = t + np.int64(z2) * np.rint(a1.sum(axis=2, keepdims=True)).astype(np.int64)
    alpha = F32(F32(g1[0]) * F32(g2[0]))
    wide = float(g1[3]) - float(g1[2]) > 255
    with np.errstate(all="ignore"):
        if wide or mutation == "scale64":
            v = (t.astype(np.float64) * np.float64(alpha)).astype(F32)
        else:
            v = (t.astype(F32) * alpha).astype(F32)
        if not sane:
            v = np.full(v.shape, np.nan, F32)
        if g_out is None:
            return dict(out=v, t=t, alpha=alpha, v=v, q=None, tie=None, idx=None, ia=ia, ib=ib)
        so, oo, qmin, qmax = g_out
        so, oo = F32(so), F32(oo)
        q = (v / so).astype(F32)
        rq = _rint_half_up(q) if mutation == "out_half_up" else np.rint(q)
        r = ((rq - q).astype(F32) + q).astype(F32)
        idx = np.clip((r + oo).astype(F32), F32(qmin), F32(qmax)).astype(F32)
        out = ((idx - oo).astype(F32) * so).astype(F32)
        q64 = q.astype(np.float64)
        tie = np.abs(q64 - np.floor(q64) - 0.5)
    return dict(out=out, t=t, alpha=alpha, v=v, q=q, tie=tie, idx=idx, ia=ia, ib=ib)


def grouped_linear(a, w, gs, a_gsum, alpha, cw, t, bias, mutation=None):
    """What mq_w8a8_linear_grouped stores: a [M, K], w [N, K] stored int8 values, group g = columns [g gs, (g + 1) gs); a_gsum int32
    [G, M], alpha fp32 [G, N], cw / t int32 [G, N], bias fp32 [N] or None.  Per output acc = 0, then for g = 0 .. G - 1:
        acc = fma_f32(fl32(P_g[m, n] + cw[g, n] a_gsum[g, m] + t[g, n]), alpha[g, n], acc)
    (one int32 -> fp32 conversion, one fused multiply-add), then one fp32 add of bias[n].  The brackets are formed in int64 and asserted
    to lie inside the kernel's domain: |cw|, |a_gsum| < 2^23 (a 24-bit multiply), the product and the bracket inside int32.
    Returns dict(out fp32 [M, N], bracket int64 [G, M, N]).  mutation (tests only): "mul_add" -- a rounded multiply and a rounded add
    for the fma; "reverse" -- the groups folded from the last to the first; "bracket_f64" -- the bracket enters the fma as a float64
    (its rounding to fp32 is lost)."""
    mutation = GROUPED_MUTATION if mutation is None else mutation
    assert mutation is None or mutation in GROUPED_MUTATIONS, mutation
    a, w = np.asarray(a), np.asarray(w)
    M, K = a.shape
    N = w.shape[0]
    assert K % gs == 0 and w.shape[1] == K
    G = K // gs
    ag, cw, t = (np.asarray(v, np.int64) for v in (a_gsum, cw, t))
    alpha = np.asarray(alpha, F32)
    assert ag.shape == (G, M) and cw.shape == (G, N) and t.shape == (G, N) and alpha.shape == (G, N)
    assert np.abs(cw).max() < 2 ** 23 and np.abs(ag).max() < 2 ** 23
    br = np.empty((G, M, N), np.int64)
    for g in range(G):
        P = np.rint(a[:, g * gs:(g + 1) * gs].astype(np.float64) @ w[:, g * gs:(g + 1) * gs].astype(np.float64).T).astype(np.int64)
        prod = cw[g][None, :] * ag[g][:, None]
        assert np.abs(prod).max() < 2 ** 31
        br[g] = P + prod + t[g][None, :]
    assert br.min() >= -2 ** 31 and br.max() < 2 ** 31
    acc = np.zeros((M, N), F32)
    for g in (range(G - 1, -1, -1) if mutation == "reverse" else range(G)):
        al = np.broadcast_to(alpha[g][None, :], (M, N))
        if mutation == "bracket_f64":
            acc = (br[g].astype(np.float64) * al.astype(np.float64) + acc.astype(np.float64)).astype(F32)
        elif mutation == "mul_add":
            acc = ((br[g].astype(F32) * al).astype(F32) + acc).astype(F32)
        else:
            acc = fma_f32(br[g].astype(F32), al, acc)
    if bias is not None:
        acc = (acc + np.asarray(bias, F32)[None, :]).astype(F32)
    return dict(out=acc, bracket=br)


# ----------------------------------------------------------------------------------------------
# a8 (pin)  the M <= 8 weight-streaming GEMV behind mq_w8a8_linear / mq_w4a8_linear and their _f32in forms (csrc/mq_gemv.hip)
# ----------------------------------------------------------------------------------------------
LINEAR_GEMV_MUTATIONS = ("fma", "divide", "half_up", "fold_offset", "gemm_form", "rowsum_recomputed")
LINEAR_GEMV_MUTATION = None   # tests only (like QMATMUL_MUTATION): makes every call without its own `mutation` wrong on purpose


def _contract_rows(image, w, w4=False, block=16384):
    """Exact int64 [M, N] of image [M, K] . w[N, K]^T, in blocks of weight rows (a float64 product of integers below 2^53); w4: w is
    pack_w4's image and is unpacked block by block."""
    a = np.asarray(image).astype(np.float64)
    assert a.shape[1] * 128 * 255 < 2 ** 53
    out = np.empty((a.shape[0], w.shape[0]), np.int64)
    for lo in range(0, w.shape[0], block):
        wi = unpack_w4(w[lo:lo + block], 0) if w4 else w[lo:lo + block]
        assert wi.shape[1] == a.shape[1]
        out[:, lo:lo + block] = np.rint(a @ wi.astype(np.float64).T).astype(np.int64)
    return out


def linear_gemv_launch(w, alpha, w_zp, col_term, bias=None, a=None, a_rowsum=None, x=None, a_grid=None, w4=False, out_grid=None,
                       out_dtype="f32", mutation=None):
    """What one launch of gemv_i8_fat_kernel stores, op for op, knowing nothing of workgroups, waves or passes.
      w         int8 [N, K] stored weights, or (w4) mq_pack_w4's image [N, K / 2]: the unsigned nibbles in pack_w4's layout
      a         int8 [M, K] stored activation image (index - shift) with a_rowsum int32 [M] or None -- the int8 entry points.  The
                kernel does NOT recompute the row sum: it takes the caller's word, and 0 when the pointer is NULL
      x, a_grid fp32 [M, K] and (scale, offset, qmin, qmax, shift) -- the _f32in entry points: the image is quantize_storage's (STORAGE
                form: IEEE x / s behind the guarded reciprocal, rint, + offset, fminf / fmaxf clamp, NaN and +-inf -> qmin) and the row
                sum is the sum of that image
      tt        wrap32(sum_k a[m, k] w[n, k] - w_zp[n] rs[m] + col_term[n]), the contraction exact
      f         fl(fl(float(tt) alpha[n]) + bias[n]): int32 -> fp32 to nearest even, a rounded multiply, a rounded add (bias 0.0f when absent)
      out_grid  None: f as f32, or rounded once more to f16.  (scale, offset, qmin, qmax): inv = fl(1 / scale), v = fl(f inv),
                q = fl(rint(v) + offset), q = fminf(fmaxf(q, qmin), qmax) (a NaN operand dropped); storage u8 (uint8)(int)q, i8
                (int)q - 128 on a grid that starts at 0 and (int)q otherwise (low byte), u16 / i16 the low 16 bits, f32 / f16
                fl(fl(q - offset) scale), f16 rounded once more.
    Returns dict(stored [M, N] in the storage type, tt int32, f fp32, v float64: the value in front of the rint (f without a grid), tie:
    its distance to the nearest half-integer, image int8 [M, K], rs int64 [M]).
    mutation (tests only, LINEAR_GEMV_MUTATIONS) makes it wrong on purpose: "fma" one fma for the multiply and the add; "divide" f / s
    for f inv; "half_up" ties rounded half up; "fold_offset" rint(v + offset); "gemm_form" the prefill GEMM's folded epilogue
    (prefill_gemm_epilogue on the same tt); "rowsum_recomputed" the image's true row sum for the caller's (or for 0 when it is NULL)."""
    mutation = LINEAR_GEMV_MUTATION if mutation is None else mutation
    assert mutation is None or mutation in LINEAR_GEMV_MUTATIONS, mutation
    w = np.asarray(w)
    assert w.ndim == 2 and w.dtype == (np.uint8 if w4 else np.int8)
    N = w.shape[0]
    if x is not None:
        assert a is None and a_rowsum is None and a_grid is not None
        s, o, qmin, qmax, shift = a_grid
        stored_a, rs32 = quantize_storage(np.asarray(x, F32), F32(s), F32(o), int(qmin), int(qmax), int(shift))
        assert stored_a.min() >= -128 and stored_a.max() <= 127, "index - shift has to fit int8"
        image, rs = stored_a.astype(np.int8), rs32.astype(np.int64)
    else:
        image = np.asarray(a)
        assert image.dtype == np.int8
        rs = np.zeros(image.shape[0], np.int64) if a_rowsum is None else np.asarray(a_rowsum, np.int64)
        if mutation == "rowsum_recomputed":
            rs = image.astype(np.int64).sum(axis=1)
    sums = _contract_rows(image, w, w4)
    tt = _wrap32(sums - np.asarray(w_zp, np.int64)[None, :] * rs[:, None] + np.asarray(col_term, np.int64)[None, :])
    tf = tt.astype(F32)                                            # int32 -> fp32, round to nearest even
    al = np.broadcast_to(np.asarray(alpha, F32).reshape(1, N), tf.shape)
    bs = np.broadcast_to((np.zeros(N, F32) if bias is None else np.asarray(bias, F32)).reshape(1, N), tf.shape)
    with np.errstate(over="ignore", invalid="ignore"):
        f = fma_f32(tf, al, bs) if mutation == "fma" else ((tf * al).astype(F32) + bs).astype(F32)
        st = PREFILL_GEMM_STORAGE[out_dtype]
        if out_grid is None:
            assert out_dtype in ("f32", "f16")
            v = f.astype(np.float64)
            return dict(stored=f.astype(st), tt=tt, f=f, v=v, tie=_tie_dist(v), image=image, rs=rs)
        so, oo, oqmin, oqmax = F32(out_grid[0]), F32(out_grid[1]), F32(out_grid[2]), F32(out_grid[3])
        if mutation == "gemm_form":
            stored, q, tie = prefill_gemm_epilogue(tt, alpha, bias, [(so, oo)], None, float(oqmin), float(oqmax), out_dtype)
            return dict(stored=stored, tt=tt, f=f, v=q, tie=tie, image=image, rs=rs)
        inv = (F32(1.0) / so).astype(F32)
        vf = (f / so).astype(F32) if mutation == "divide" else (f * inv).astype(F32)
        if mutation == "fold_offset":
            q = np.rint((vf + oo).astype(F32)).astype(F32)
        else:
            q = ((_rint_half_up(vf) if mutation == "half_up" else np.rint(vf)) + oo).astype(F32)
        q = np.fmin(np.fmax(q, oqmin), oqmax)
        qi = q.astype(np.int64)
        if out_dtype == "u8":
            stored = (qi & 0xFF).astype(np.uint8)
        elif out_dtype == "i8":
            stored = ((qi - (128 if float(oqmin) == 0.0 else 0)) & 0xFF).astype(np.uint8).view(np.int8)
        elif out_dtype in ("u16", "i16"):
            stored = (qi & 0xFFFF).astype(np.uint16).view(st)
        else:
            stored = ((q - oo).astype(F32) * so).astype(F32).astype(st)
    v = vf.astype(np.float64)
    return dict(stored=stored, tt=tt, f=f, v=v, tie=_tie_dist(v), image=image, rs=rs)
