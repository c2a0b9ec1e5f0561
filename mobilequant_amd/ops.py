"""Tensor-level wrappers over the C ABI (include/mobilequant_amd.h).

PyTorch is plumbing here: it owns device memory and the current HIP stream; every computation is a
hand-written HIP kernel in libmobilequant_amd.so.  All functions require ROCm device tensors and raise
otherwise -- there is no CPU or eager-PyTorch fallback.

Operands come in three kinds (tests/ops_contract_cases.py lists every one).  A *converted* operand (grids, bias, weights of the norms: `_f32`)
may be any floating dtype in any layout; it is read as contiguous float32, copied where it is not that already, and the copy lives until
the launch is queued.  An integer or bool tensor is refused there on purpose, not converted: a grid of integers is a caller's mistake
(an index tensor passed for a scale), and a silent conversion would hide it.  A *layout* operand (activations) keeps its dtype and is made
contiguous.  Every other pointer -- outputs, in-place statistics, integer images, epilogue vectors -- goes to the entry as it is: `_raw`
checks device, dtype, contiguity and element count and copies nothing.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import MQ_F16, MQ_F32, MQ_I8, MQ_I16, MQ_I32, MQ_U8, MQ_U16

_DT = {torch.float32: MQ_F32, torch.float16: MQ_F16}
_QDT = {MQ_I8: torch.int8, MQ_U8: torch.uint8, MQ_I16: torch.int16, MQ_U16: torch.uint16, MQ_I32: torch.int32}


def _dev(t: torch.Tensor, what: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"mobilequant_amd: {what} must be a ROCm device tensor (got "
                           f"{getattr(t, 'device', type(t))}); there is no CPU path")
    return t


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


class _on:
    """Device guard: every tensor handed to one C-ABI call must live on the same ROCm device, and the call is made with
    that device current (so the stream is that device's current stream and the kernel launches there) -- a model placed on
    cuda:1 while cuda:0 is current must not race or fault.  No-op when the device is already current."""

    __slots__ = ("idx", "prev")

    def __init__(self, first: torch.Tensor, *rest):
        dev = first.device
        for t in rest:
            if t is not None and t.device != dev:
                raise RuntimeError(f"mobilequant_amd: tensors on different devices in one call ({dev} vs {t.device}); move the "
                                   "quantizer grids / statistics to the activation's device")
        self.idx = dev.index if dev.type == "cuda" else None
        self.prev = None

    def __enter__(self):
        if self.idx is not None and torch.cuda.current_device() != self.idx:
            self.prev = torch.cuda.current_device()
            torch.cuda.set_device(self.idx)
        return self

    def __exit__(self, *exc):
        if self.prev is not None:
            torch.cuda.set_device(self.prev)
        return False


def _fdt(t: torch.Tensor, what: str = "x") -> int:
    try:
        return _DT[t.dtype]
    except KeyError:
        raise RuntimeError(f"mobilequant_amd: dtype {t.dtype} not supported (float32, float16) for {what}") from None


def _f32(t: torch.Tensor, what: str, align16: bool = False) -> torch.Tensor:
    """The contiguous float32 form of a converted operand: the tensor itself when it is that already, else a copy the CALLER keeps alive
    until its launch is queued.  align16: the entry takes a 16-byte aligned pointer, so a contiguous view off that boundary is copied too."""
    _dev(t, what)
    if t.dtype != torch.float32 or not t.is_contiguous():
        if not t.dtype.is_floating_point:
            raise RuntimeError(f"mobilequant_amd: {what} must be a floating-point tensor (got {t.dtype}); it is read as float32")
        t = t.to(torch.float32).contiguous()
    if align16 and t.data_ptr() % 16:
        t = t.clone()
    return t


def _raw(t: torch.Tensor, what: str, dtype, numel: Optional[int] = None, at_least: bool = False) -> torch.Tensor:
    """An operand whose pointer goes to the C entry as it is (outputs, in-place statistics, integer images and epilogue vectors): a
    contiguous device tensor of `dtype` (one dtype or a tuple) with `numel` elements (at_least: that many or more -- a read-only
    buffer may be longer than the launch reads).  Nothing is converted or copied; host attribute reads only."""
    _dev(t, what)
    dts = dtype if isinstance(dtype, tuple) else (dtype,)
    if t.dtype not in dts or not t.is_contiguous() or (numel is not None and (t.numel() < numel if at_least else t.numel() != numel)):
        raise RuntimeError(f"mobilequant_amd: {what} must be a contiguous {' / '.join(str(d) for d in dts)} device tensor"
                           + (f" of {'at least ' if at_least else ''}{numel} elements" if numel is not None else "")
                           + f" (got {t.dtype}, shape {tuple(t.shape)}, strides {tuple(t.stride())})")
    return t


def _same_len(a: torch.Tensor, b: torch.Tensor, what_a: str, what_b: str) -> None:
    if a.numel() != b.numel():
        raise RuntimeError(f"mobilequant_amd: {what_b} holds {b.numel()} elements, {what_a} {a.numel()}: one {what_b} entry per {what_a} entry")


def _stats(stats, n: int, who: str):
    """The n 1-element fp32 running statistics of a calibration pass, each handed over by pointer."""
    stats = list(stats)
    if len(stats) != n:
        raise RuntimeError(f"mobilequant_amd: {who} stats must hold {n} tensors (got {len(stats)})")
    return [_raw(t, f"{who} stats[{i}]", torch.float32, 1) for i, t in enumerate(stats)]


_I8 = (torch.int8, torch.uint8)


def _al16(t: torch.Tensor) -> torch.Tensor:
    """A contiguous input for an entry that takes 16-byte aligned pointers: a view off that boundary is copied, like any other layout."""
    return t.clone() if t.data_ptr() % 16 else t


# ---- a1 --------------------------------------------------------------------------------------------
def scale_offset_from_minmax(min_val: torch.Tensor, max_val: torch.Tensor, bitwidth: int, is_symmetric: bool):
    """Device version of compute_scale_offset_from_min_max (qmodule.py:40-61); shapes follow min_val."""
    mn, mx = _f32(min_val, "min_val"), _f32(max_val, "max_val")
    _same_len(mn, mx, "min_val", "max_val")
    scale, offset = torch.empty_like(mn), torch.empty_like(mn)
    with _on(mn, mx):
        _lib.call("mq_scale_offset_from_minmax", mn.data_ptr(), mx.data_ptr(), mn.numel(), int(bitwidth),
                  int(bool(is_symmetric)), scale.data_ptr(), offset.data_ptr(), _stream())
    return scale, offset


# ---- a3 / a12 --------------------------------------------------------------------------------------
def minmax_new(n: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """Fresh running statistics (min = +inf, max = -inf)."""
    if torch.device(device).type != "cuda":
        raise RuntimeError(f"mobilequant_amd: minmax_new needs a ROCm device (got {device}); there is no CPU path")
    mn = torch.empty(n, dtype=torch.float32, device=device)
    mx = torch.empty(n, dtype=torch.float32, device=device)
    with _on(mn, mx):
        _lib.call("mq_minmax_init", mn.data_ptr(), mx.data_ptr(), n, _stream())
    return mn, mx


def minmax_tensor_(x: torch.Tensor, mn: torch.Tensor, mx: torch.Tensor) -> None:
    """Running per-tensor update: mn[0] = min(mn[0], x.min()), mx[0] = max(mx[0], x.max())."""
    x = _dev(x, "x").contiguous()
    _raw(mn, "mn", torch.float32, 1), _raw(mx, "mx", torch.float32, 1)
    with _on(x, mn, mx):
        _lib.call("mq_minmax_tensor", x.data_ptr(), _fdt(x), x.numel(), mn.data_ptr(), mx.data_ptr(), _stream())


def hist_new(n_slots: int, mantissa_bits: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """Fresh running histograms of mq_hist_minmax_tensor: (counts int64 [n_slots, 2 * NB], nan int64 [n_slots]), NB = 256 << mantissa_bits.
    The kernel reads the int64 words as unsigned 64-bit counters (counts stay below 2^63)."""
    if not 0 <= int(mantissa_bits) <= 6:
        raise ValueError(f"mobilequant_amd: mantissa_bits={mantissa_bits} outside 0..6")
    return (torch.zeros((n_slots, 512 << int(mantissa_bits)), dtype=torch.int64, device=device),
            torch.zeros((n_slots,), dtype=torch.int64, device=device))


def hist_minmax_tensor_(t: torch.Tensor, counts_row: torch.Tensor, nan_row: torch.Tensor, mn: Optional[torch.Tensor], mx: Optional[torch.Tensor],
                        mantissa_bits: int) -> None:
    """ONE pass over t: its bit-pattern histogram is ADDED to counts_row [2 * NB] / nan_row [1] (int64, read as u64) and its min / max
    folded into the running mn / mx (1-element fp32, the bits of minmax_tensor_; None as a pair: histogram only)."""
    x = _dev(t, "x").contiguous()
    for c, what, n in ((counts_row, "counts_row", 512 << int(mantissa_bits)), (nan_row, "nan_row", 1)):
        if _dev(c, what).dtype != torch.int64 or not c.is_contiguous() or c.numel() != n:
            raise RuntimeError(f"mobilequant_amd: {what} must be a contiguous int64 tensor of {n} elements (got {c.dtype}, {tuple(c.shape)})")
    if (mn is None) != (mx is None):
        raise RuntimeError("mobilequant_amd: hist_minmax_tensor_ takes mn and mx as a pair")
    if mn is not None:
        _raw(mn, "mn", torch.float32, 1), _raw(mx, "mx", torch.float32, 1)
    with _on(x, counts_row, nan_row, mn, mx):
        _lib.call("mq_hist_minmax_tensor", x.data_ptr(), _fdt(x), x.numel(), int(mantissa_bits), counts_row.data_ptr(), nan_row.data_ptr(),
                  None if mn is None else mn.data_ptr(), None if mx is None else mx.data_ptr(), _stream())


def minmax_rows_(x2d: torch.Tensor, mn: torch.Tensor, mx: torch.Tensor) -> None:
    x2d = _dev(x2d, "x").contiguous()
    if x2d.dim() != 2:
        raise RuntimeError(f"mobilequant_amd: minmax_rows_ x must be [rows, cols] (got {tuple(x2d.shape)})")
    rows, cols = x2d.shape
    _raw(mn, "mn", torch.float32, rows), _raw(mx, "mx", torch.float32, rows)
    with _on(x2d, mn, mx):
        _lib.call("mq_minmax_rows", x2d.data_ptr(), _fdt(x2d), rows, cols, mn.data_ptr(), mx.data_ptr(), _stream())


def minmax_cols_(x2d: torch.Tensor, mn: torch.Tensor, mx: torch.Tensor) -> None:
    x2d = _dev(x2d, "x").contiguous()
    if x2d.dim() != 2:
        raise RuntimeError(f"mobilequant_amd: minmax_cols_ x must be [rows, cols] (got {tuple(x2d.shape)})")
    rows, cols = x2d.shape
    _raw(mn, "mn", torch.float32, cols), _raw(mx, "mx", torch.float32, cols)
    with _on(x2d, mn, mx):
        _lib.call("mq_minmax_cols", x2d.data_ptr(), _fdt(x2d), rows, cols, mn.data_ptr(), mx.data_ptr(), _stream())


def calib_attention_probs_(raw: torch.Tensor, mask: Optional[torch.Tensor], sqrt_d: float, raw_min: torch.Tensor, raw_max: torch.Tensor,
                           probs_min: torch.Tensor, probs_max: torch.Tensor) -> torch.Tensor:
    """Calibration-mode score chain (mq_calib_attention_probs): raw [..., S, T] fp32 scores are replaced IN PLACE by
    softmax(raw / sqrt_d + mask, -1) while the running [min, max] of the raw scores and of the probabilities (1-element fp32 device
    tensors, ActRangeCollector's slots) are updated -- hf_model.py:513-530 between generate_act_range.py's two hooks.  mask: None or an
    additive fp32 [S, T] tensor.  Returns `raw` (now the probabilities)."""
    raw = _dev(raw, "raw")
    if raw.dtype != torch.float32 or not raw.is_contiguous():
        raise RuntimeError("mobilequant_amd: calib_attention_probs_ takes a contiguous float32 score tensor")
    cols = raw.shape[-1]
    rows = raw.numel() // max(cols, 1)
    mrows = 0
    if mask is not None:
        mask = _dev(mask, "mask")
        if mask.dtype != torch.float32 or not mask.is_contiguous() or mask.dim() != 2 or mask.shape[1] != cols or raw.shape[-2] != mask.shape[0]:
            raise RuntimeError("mobilequant_amd: calib_attention_probs_ mask must be a contiguous float32 [S, T] tensor")
        mrows = mask.shape[0]
    for t, what in ((raw_min, "raw_min"), (raw_max, "raw_max"), (probs_min, "probs_min"), (probs_max, "probs_max")):
        _raw(t, what, torch.float32, 1)
    with _on(raw, mask, raw_min, raw_max, probs_min, probs_max):
        _lib.call("mq_calib_attention_probs", raw.data_ptr(), raw.data_ptr(), rows, cols, mask.data_ptr() if mask is not None else None, mrows,
                  float(sqrt_d), raw_min.data_ptr(), raw_max.data_ptr(), probs_min.data_ptr(), probs_max.data_ptr(), _stream())
    return raw


def calib_norm_(x: torch.Tensor, delta: Optional[torch.Tensor], weight: torch.Tensor, bias: Optional[torch.Tensor], eps: float, layernorm: bool,
                in_min: torch.Tensor, in_max: torch.Tensor, out_min: torch.Tensor, out_max: torch.Tensor,
                delta_min: Optional[torch.Tensor] = None, delta_max: Optional[torch.Tensor] = None):
    """Calibration-mode norm (mq_calib_norm): h = x (+ delta), y = RMSNorm / LayerNorm(h) with the running [min, max] of h (the module's
    input hook) and of y (its output hook) taken in the same pass; delta_min / delta_max: also that of delta itself.  Returns (h, y); h is x
    itself without a delta."""
    x = _dev(x, "x")
    if delta is not None:
        _dev(delta, "delta")
    if x.dtype != torch.float32 or not x.is_contiguous() or (delta is not None and (delta.dtype != torch.float32 or not delta.is_contiguous()
                                                                                        or delta.shape != x.shape)):
        raise RuntimeError("mobilequant_amd: calib_norm_ takes contiguous float32 tensors of one shape")
    cols = x.shape[-1]
    rows = x.numel() // max(cols, 1)
    y = torch.empty_like(x)
    h = torch.empty_like(x) if delta is not None else None
    w = _f32(weight, "weight", True)
    b = _f32(bias, "bias", True) if bias is not None else None
    if w.numel() != cols or (b is not None and b.numel() != cols):
        raise RuntimeError(f"mobilequant_amd: calib_norm_ weight / bias must hold {cols} elements (got {w.numel()}"
                           + (f", {b.numel()}" if b is not None else "") + ")")
    if (delta_min is None) != (delta_max is None):
        raise RuntimeError("mobilequant_amd: calib_norm_ takes delta_min and delta_max as a pair")
    for t, what in ((in_min, "in_min"), (in_max, "in_max"), (out_min, "out_min"), (out_max, "out_max"), (delta_min, "delta_min"),
                    (delta_max, "delta_max")):
        if t is not None:
            _raw(t, what, torch.float32, 1)
    with _on(x, delta, w, b, y, h, in_min, in_max, out_min, out_max, delta_min, delta_max):
        _lib.call("mq_calib_norm", x.data_ptr(), delta.data_ptr() if delta is not None else None, h.data_ptr() if h is not None else None,
                  y.data_ptr(), rows, cols, w.data_ptr(), b.data_ptr() if b is not None else None, float(eps), int(bool(layernorm)),
                  in_min.data_ptr(), in_max.data_ptr(), out_min.data_ptr(), out_max.data_ptr(),
                  delta_min.data_ptr() if delta_min is not None else None, delta_max.data_ptr() if delta_max is not None else None, _stream())
    return (h if h is not None else x), y


def calib_gated_(a: torch.Tensor, b: torch.Tensor, act: str, stats) -> torch.Tensor:
    """Calibration-mode act(a) * b (mq_calib_gated) with the running [min, max] of a, act(a), b and the product: stats = eight 1-element
    fp32 device tensors (min, max) x 4 in that order.  act: "silu" | "gelu" (erf).  Returns the product."""
    a, b = _dev(a, "a"), _dev(b, "b")
    if a.dtype != torch.float32 or b.dtype != torch.float32 or a.shape != b.shape or not a.is_contiguous() or not b.is_contiguous():
        raise RuntimeError("mobilequant_amd: calib_gated_ takes two contiguous float32 tensors of one shape")
    stats = _stats(stats, 8, "calib_gated_")
    out = torch.empty_like(a)
    ptrs = (ctypes.c_void_p * 8)(*[t.data_ptr() for t in stats])
    with _on(a, b, out, *stats):
        _lib.call("mq_calib_gated", a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), {"silu": 0, "gelu": 1}[act], ptrs, _stream())
    return out


def calib_rope_(q_lin: torch.Tensor, k_lin: torch.Tensor, heads: int, kv_heads: int, head_dim: int, cos: torch.Tensor, sin: torch.Tensor, stats):
    """Calibration-mode RoPE (mq_calib_rope): q_lin [B, S, heads * D], k_lin [B, S, kv_heads * D] (the projections' outputs) -> q [B, heads,
    S, D], k [B, kv_heads, S, D] contiguous, rotated with cos / sin [S, rot]; stats = eight 1-element fp32 device tensors: (min, max) of
    q_lin, q, k_lin, k.  The bits of llama.apply_rope."""
    q_lin, k_lin = _dev(q_lin, "q"), _dev(k_lin, "k")
    if q_lin.dim() != 3 or k_lin.dim() != 3 or k_lin.shape[:2] != q_lin.shape[:2]:
        raise RuntimeError("mobilequant_amd: calib_rope_ takes the contiguous float32 outputs of q_proj / k_proj [B, S, heads * D] and cos / sin [S, rot]")
    B, S = q_lin.shape[0], q_lin.shape[1]
    cos, sin = _f32(cos, "cos", True), _f32(sin, "sin", True)
    if (q_lin.dtype != torch.float32 or k_lin.dtype != torch.float32 or not q_lin.is_contiguous() or not k_lin.is_contiguous()
            or q_lin.shape[-1] != heads * head_dim or k_lin.shape[-1] != kv_heads * head_dim or cos.shape != sin.shape or cos.shape[0] != S):
        raise RuntimeError("mobilequant_amd: calib_rope_ takes the contiguous float32 outputs of q_proj / k_proj and cos / sin [S, rot]")
    stats = _stats(stats, 8, "calib_rope_")
    q = torch.empty((B, heads, S, head_dim), dtype=torch.float32, device=q_lin.device)
    k = torch.empty((B, kv_heads, S, head_dim), dtype=torch.float32, device=q_lin.device)
    ptrs = (ctypes.c_void_p * 8)(*[t.data_ptr() for t in stats])
    with _on(q_lin, k_lin, q, k, cos, sin, *stats):
        _lib.call("mq_calib_rope", q_lin.data_ptr(), k_lin.data_ptr(), q.data_ptr(), k.data_ptr(), B, S, heads, kv_heads, head_dim, cos.shape[1],
                  cos.data_ptr(), sin.data_ptr(), ptrs, _stream())
    return q, k


def calib_rope_qkv_(q_lin: torch.Tensor, k_lin: torch.Tensor, v_lin: torch.Tensor, heads: int, kv_heads: int, head_dim: int, cos: torch.Tensor,
                    sin: torch.Tensor, stats):
    """calib_rope_ with v carried along and repeat_kv inside (mq_calib_rope_qkv): returns q [B, heads, S, D] and k, v [B, heads, S, D]
    with every kv head repeated heads / kv_heads times; stats = ten 1-element fp32 device tensors: (min, max) of q_lin, q, k_lin, k, v_lin."""
    q_lin, k_lin, v_lin = _dev(q_lin, "q"), _dev(k_lin, "k"), _dev(v_lin, "v")
    if q_lin.dim() != 3 or k_lin.dim() != 3 or k_lin.shape[:2] != q_lin.shape[:2] or v_lin.shape != k_lin.shape:
        raise RuntimeError("mobilequant_amd: calib_rope_qkv_ takes the contiguous float32 outputs of q_proj / k_proj / v_proj [B, S, heads * D] "
                           "and cos / sin [S, rot]")
    B, S = q_lin.shape[0], q_lin.shape[1]
    cos, sin = _f32(cos, "cos", True), _f32(sin, "sin", True)
    if (any(t.dtype != torch.float32 or not t.is_contiguous() for t in (q_lin, k_lin, v_lin)) or q_lin.shape[-1] != heads * head_dim
            or k_lin.shape[-1] != kv_heads * head_dim or v_lin.shape != k_lin.shape or cos.shape != sin.shape or cos.shape[0] != S):
        raise RuntimeError("mobilequant_amd: calib_rope_qkv_ takes the contiguous float32 outputs of q_proj / k_proj / v_proj and cos / sin [S, rot]")
    stats = _stats(stats, 10, "calib_rope_qkv_")
    q, k, v = (torch.empty((B, heads, S, head_dim), dtype=torch.float32, device=q_lin.device) for _ in range(3))
    ptrs = (ctypes.c_void_p * 12)(*([t.data_ptr() for t in stats] + [None, None]))
    with _on(q_lin, k_lin, v_lin, q, k, v, cos, sin, *stats):
        _lib.call("mq_calib_rope_qkv", q_lin.data_ptr(), k_lin.data_ptr(), v_lin.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(), B, S, heads,
                  kv_heads, head_dim, cos.shape[1], cos.data_ptr(), sin.data_ptr(), ptrs, _stream())
    return q, k, v


def calib_attention_probs_causal_(raw: torch.Tensor, out: torch.Tensor, sqrt_d: float, store_masked: bool, raw_min: torch.Tensor, raw_max: torch.Tensor,
                                  probs_min: torch.Tensor, probs_max: torch.Tensor) -> torch.Tensor:
    """calib_attention_probs_ under the causal mask of square [S, S] blocks (mq_calib_attention_probs_causal): no mask tensor is read;
    store_masked = False leaves the quads above the diagonal of `out` (a buffer of raw's shape, not raw itself) untouched -- it must
    already hold zeros there.  Returns `out`."""
    raw, out = _dev(raw, "raw"), _dev(out, "out")
    S = raw.shape[-1]
    if (raw.dtype != torch.float32 or out.dtype != torch.float32 or not raw.is_contiguous() or not out.is_contiguous() or raw.shape != out.shape
            or raw.dim() < 2 or raw.shape[-2] != S):
        raise RuntimeError("mobilequant_amd: calib_attention_probs_causal_ takes contiguous float32 [..., S, S] tensors")
    if out.data_ptr() == raw.data_ptr():
        raise RuntimeError("mobilequant_amd: calib_attention_probs_causal_ out must not be raw itself")
    for t, what in ((raw_min, "raw_min"), (raw_max, "raw_max"), (probs_min, "probs_min"), (probs_max, "probs_max")):
        _raw(t, what, torch.float32, 1)
    with _on(raw, out, raw_min, raw_max, probs_min, probs_max):
        _lib.call("mq_calib_attention_probs_causal", raw.data_ptr(), out.data_ptr(), raw.numel() // max(S, 1), S, float(sqrt_d), int(bool(store_masked)),
                  raw_min.data_ptr(), raw_max.data_ptr(), probs_min.data_ptr(), probs_max.data_ptr(), _stream())
    return out


def minmax_tensor(x: torch.Tensor):
    """(min, max) of one tensor as 1-element device tensors: partials + fold, no atomics, no init launch."""
    x = _dev(x, "x").contiguous()
    buf = torch.empty(2 + 1024, dtype=torch.float32, device=x.device)     # [min | max | scratch]
    mn, mx, scratch = buf[0:1], buf[1:2], buf[2:]
    with _on(x):
        _lib.call("mq_minmax_tensor_fresh", x.data_ptr(), _fdt(x), x.numel(), mn.data_ptr(), mx.data_ptr(), scratch.data_ptr(),
                  scratch.numel(), _stream())
    return mn, mx


def _x2d(x2d: torch.Tensor, who: str) -> torch.Tensor:
    """The checks of minmax_rows_ / minmax_cols_ on x, made before the fresh statistics are initialised (a launch of its own)."""
    _fdt(_dev(x2d, "x"))
    if x2d.dim() != 2:
        raise RuntimeError(f"mobilequant_amd: {who} x must be [rows, cols] (got {tuple(x2d.shape)})")
    return x2d


def minmax_rows(x2d: torch.Tensor):
    _x2d(x2d, "minmax_rows")
    mn, mx = minmax_new(x2d.shape[0], x2d.device)
    minmax_rows_(x2d, mn, mx)
    return mn, mx


def minmax_cols(x2d: torch.Tensor):
    _x2d(x2d, "minmax_cols")
    mn, mx = minmax_new(x2d.shape[1], x2d.device)
    minmax_cols_(x2d, mn, mx)
    return mn, mx


# ---- a5 --------------------------------------------------------------------------------------------
def _rows_cols(x: torch.Tensor, n_scale: int) -> Tuple[int, int]:
    if n_scale == 1:
        return 1, x.numel()
    if x.numel() % n_scale:
        raise RuntimeError(f"mobilequant_amd: {n_scale} scales do not divide a tensor of {x.numel()} elements")
    return n_scale, x.numel() // n_scale


def fake_quant(x: torch.Tensor, scale: torch.Tensor, offset: torch.Tensor, qmin: float, qmax: float,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Quantizer.forward arithmetic (qmodule.py:286-295).  `scale`/`offset` hold 1 element (per-tensor)
    or one per row of x viewed as [n_scale, -1] (per-channel / per-group)."""
    x = _dev(x, "x").contiguous()
    s, o = _f32(scale, "scale"), _f32(offset, "offset")
    _same_len(s, o, "scale", "offset")
    rows, cols = _rows_cols(x, s.numel())
    if out is None:
        y = torch.empty_like(x)
    else:
        y = _raw(out, "out", x.dtype, x.numel())
        if y.shape != x.shape:
            raise RuntimeError(f"mobilequant_amd: out must have x's shape {tuple(x.shape)} (got {tuple(y.shape)})")
    with _on(x, s, o, y):
        _lib.call("mq_fake_quant", x.data_ptr(), y.data_ptr(), _fdt(x), rows, cols, s.data_ptr(), o.data_ptr(),
                  s.numel(), float(qmin), float(qmax), _stream())
    return y


def fake_quant_backward(x: torch.Tensor, grad_y: torch.Tensor, scale: torch.Tensor, offset: torch.Tensor, qmin: float,
                        qmax: float):
    """Straight-through gradients of fake_quant: (grad_x, grad_scale, grad_offset), fp32."""
    x = _f32(x, "x")
    g = _f32(grad_y, "grad_y")
    s, o = _f32(scale, "scale"), _f32(offset, "offset")
    _same_len(s, o, "scale", "offset")
    if g.shape != x.shape:
        raise RuntimeError(f"mobilequant_amd: grad_y must have x's shape {tuple(x.shape)} (got {tuple(g.shape)})")
    rows, cols = _rows_cols(x, s.numel())
    gx = torch.empty_like(x)
    acc = torch.zeros(2 * s.numel(), dtype=torch.float32, device=x.device)      # one fill for both accumulators
    gs, go = acc[:s.numel()].view(s.shape), acc[s.numel():].view(o.shape)
    with _on(x, g, s, o):
        _lib.call("mq_fake_quant_backward", x.data_ptr(), g.data_ptr(), rows, cols, s.data_ptr(), o.data_ptr(), s.numel(),
                  float(qmin), float(qmax), gx.data_ptr(), gs.data_ptr(), go.data_ptr(), _stream())
    return gx, gs, go


def _chan(chan_scale, cols: int, x: torch.Tensor):
    if chan_scale is None:
        return None
    cs = _f32(chan_scale, "chan_scale").reshape(-1)
    if cs.numel() != cols or x.dtype != torch.float32:
        raise RuntimeError(f"mobilequant_amd: chan_scale needs {cols} fp32 entries (got {cs.numel()}) and float32 activations")
    return cs


def lwc_fake_quant_supported(w: torch.Tensor) -> bool:
    return (w.is_cuda and w.dtype == torch.float32 and w.dim() == 2 and w.shape[1] % 4 == 0 and 0 < w.shape[1] <= 16384
            and w.is_contiguous() and w.data_ptr() % 16 == 0)


def lwc_fake_quant(w: torch.Tensor, sig_lo: torch.Tensor, sig_hi: torch.Tensor, bitwidth: int, is_symmetric: bool):
    """Per-row range -> sigmoid(bound) * range -> grid -> fake-quant of a weight [N, K] in one pass (mq_lwc_fake_quant).
    Returns (w_q, row_min, row_max, scale, offset), the last four [N]."""
    w = _f32(_dev(w, "w"), "w", True)
    N, K = w.shape
    lo, hi = _f32(sig_lo, "sig_lo").reshape(-1), _f32(sig_hi, "sig_hi").reshape(-1)
    if lo.numel() != N or hi.numel() != N:
        raise RuntimeError("mobilequant_amd: lwc_fake_quant needs one bound factor per output row")
    out = torch.empty_like(w)
    mn, mx, sc, of = (torch.empty(N, dtype=torch.float32, device=w.device) for _ in range(4))
    with _on(w, lo, hi):
        _lib.call("mq_lwc_fake_quant", w.data_ptr(), N, K, lo.data_ptr(), hi.data_ptr(), int(bitwidth), int(bool(is_symmetric)),
                  out.data_ptr(), mn.data_ptr(), mx.data_ptr(), sc.data_ptr(), of.data_ptr(), _stream())
    return out, mn, mx, sc, of


def lwc_fake_quant_backward(w, grad_out, sig_lo, sig_hi, row_min, row_max, bitwidth: int, is_symmetric: bool):
    """(grad_w, grad_sig_lo, grad_sig_hi) of lwc_fake_quant (mq_lwc_fake_quant_backward)."""
    w, g = _f32(_dev(w, "w"), "w", True), _f32(_dev(grad_out, "grad_out"), "grad_out", True)
    N, K = w.shape
    lo, hi = _f32(sig_lo, "sig_lo").reshape(-1), _f32(sig_hi, "sig_hi").reshape(-1)
    if lo.numel() != N or hi.numel() != N:
        raise RuntimeError("mobilequant_amd: lwc_fake_quant_backward needs one bound factor (sig_lo, sig_hi) per output row")
    if g.shape != w.shape:
        raise RuntimeError(f"mobilequant_amd: grad_out must have w's shape {tuple(w.shape)} (got {tuple(g.shape)})")
    _raw(row_min, "row_min", torch.float32, N), _raw(row_max, "row_max", torch.float32, N)
    gw = torch.empty_like(w)
    glo, ghi = torch.empty(N, dtype=torch.float32, device=w.device), torch.empty(N, dtype=torch.float32, device=w.device)
    with _on(w, g, lo, hi, row_min, row_max):
        _lib.call("mq_lwc_fake_quant_backward", w.data_ptr(), g.data_ptr(), N, K, lo.data_ptr(), hi.data_ptr(), row_min.data_ptr(),
                  row_max.data_ptr(), int(bitwidth), int(bool(is_symmetric)), gw.data_ptr(), glo.data_ptr(), ghi.data_ptr(), _stream())
    return gw, glo, ghi


LWC_SEARCH_MAX_CANDIDATES = 1024


def lwc_search(w2d: torch.Tensor, sig_lo: torch.Tensor, sig_hi: torch.Tensor, bitwidth: int, is_symmetric: bool,
               col_weight: Optional[torch.Tensor] = None, return_costs: bool = False):
    """Clip search over a weight viewed [rows, cols] (mq_lwc_search): every row is scored under the C candidate pairs sig_lo[c], sig_hi[c]
    (fp32 [C], sigmoid(bound factor) already evaluated) by the fp64 sum of (Q(w) - w)^2 (* col_weight), Q the LWC fake-quant of
    lwc_fake_quant at that pair.  col_weight: fp32, a multiple of cols long; row r uses elements (r % (len / cols)) * cols + i.
    Returns (best_idx int32 [rows], best_cost fp64 [rows], base_cost fp64 [rows] = the cost of candidate 0) and, with return_costs, the
    table costs fp64 [rows, C].  Candidate 0 is the incumbent, a later one wins only with a strictly smaller cost.
    The arguments' dtypes and shapes are checked first (nothing is converted: what was scored is what the caller holds), the device last."""
    for t, what in ((w2d, "w2d"), (sig_lo, "sig_lo"), (sig_hi, "sig_hi"), (col_weight, "col_weight")):
        if t is None and what == "col_weight":
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise RuntimeError(f"mobilequant_amd: lwc_search takes float32 tensors ({what}: {getattr(t, 'dtype', type(t))})")
        if not t.is_contiguous():
            raise RuntimeError(f"mobilequant_amd: lwc_search takes contiguous tensors ({what})")
    if w2d.dim() != 2:
        raise RuntimeError(f"mobilequant_amd: lwc_search takes the weight viewed [rows, cols] (got {tuple(w2d.shape)})")
    rows, cols = w2d.shape
    if cols % 4 != 0 or not 16 <= cols <= 16384:
        raise RuntimeError(f"mobilequant_amd: lwc_search takes rows of 16 to 16384 columns, a multiple of 4 (cols={cols})")
    if sig_lo.dim() != 1 or sig_lo.shape != sig_hi.shape:
        raise RuntimeError(f"mobilequant_amd: lwc_search takes two candidate tables [C] of one length (got {tuple(sig_lo.shape)}, {tuple(sig_hi.shape)})")
    C = sig_lo.numel()
    if not 1 <= C <= LWC_SEARCH_MAX_CANDIDATES:
        raise RuntimeError(f"mobilequant_amd: lwc_search takes 1 to {LWC_SEARCH_MAX_CANDIDATES} candidates (got {C})")
    if not 2 <= int(bitwidth) <= 16:
        raise RuntimeError(f"mobilequant_amd: lwc_search bitwidth={bitwidth} outside 2..16")
    if col_weight is not None and (col_weight.dim() != 1 or col_weight.numel() < cols or col_weight.numel() % cols != 0):
        raise RuntimeError(f"mobilequant_amd: lwc_search col_weight holds a multiple of cols={cols} entries (got {tuple(col_weight.shape)})")
    for t, what in ((w2d, "w2d"), (sig_lo, "sig_lo"), (sig_hi, "sig_hi"), (col_weight, "col_weight")):
        if t is not None:
            _dev(t, what)
    dev = w2d.device
    idx = torch.empty(rows, dtype=torch.int32, device=dev)
    best, base = torch.empty(rows, dtype=torch.float64, device=dev), torch.empty(rows, dtype=torch.float64, device=dev)
    costs = torch.empty((rows, C), dtype=torch.float64, device=dev) if return_costs else None
    with _on(w2d, sig_lo, sig_hi, col_weight):
        _lib.call("mq_lwc_search", w2d.data_ptr(), rows, cols, sig_lo.data_ptr(), sig_hi.data_ptr(), C, int(bitwidth), int(bool(is_symmetric)),
                  col_weight.data_ptr() if col_weight is not None else None, col_weight.numel() if col_weight is not None else 0,
                  idx.data_ptr(), best.data_ptr(), base.data_ptr(), costs.data_ptr() if return_costs else None, _stream())
    return (idx, best, base, costs) if return_costs else (idx, best, base)


def attention_probs_train_supported(raw: torch.Tensor, mask: Optional[torch.Tensor]) -> bool:
    if not (raw.is_cuda and raw.dtype == torch.float32 and raw.dim() >= 2 and raw.is_contiguous() and raw.shape[-1] % 4 == 0
            and 0 < raw.shape[-1] <= 4096 and raw.data_ptr() % 16 == 0):
        return False
    if mask is None:
        return True
    return (mask.is_cuda and mask.dtype == torch.float32 and mask.dim() >= 2 and all(d == 1 for d in mask.shape[:-2])
            and mask.shape[-1] == raw.shape[-1] and mask.shape[-2] == raw.shape[-2])


def _attn_probs_args(raw, mask, g1, g2):
    cols = raw.shape[-1]
    rows = raw.numel() // cols
    m = None if mask is None else _f32(mask, "mask", True).reshape(-1, cols)
    s1, o1, s2, o2 = (_f32(t, "grid") for t in (g1[0], g1[1], g2[0], g2[1]))
    if any(t.numel() != 1 for t in (s1, o1, s2, o2)):
        raise RuntimeError("mobilequant_amd: attention_probs_train takes per-tensor grids: every grid scale and offset holds one element")
    return rows, cols, m, (s1, o1, s2, o2)


def attention_probs_train(raw, mask, grid1, grid2, sqrt_d: float):
    """Q2(softmax(Q1(raw) / sqrt_d + mask)) over the last dimension (mq_attention_probs_train); grid = (scale, offset, qmin, qmax)."""
    raw = _f32(_dev(raw, "raw"), "raw", True)
    rows, cols, m, (s1, o1, s2, o2) = _attn_probs_args(raw, mask, grid1, grid2)
    out = torch.empty_like(raw)
    with _on(raw, m, s1, o1, s2, o2):
        _lib.call("mq_attention_probs_train", raw.data_ptr(), rows, cols, m.data_ptr() if m is not None else None, m.shape[0] if m is not None else 1,
                  s1.data_ptr(), o1.data_ptr(), float(grid1[2]), float(grid1[3]), s2.data_ptr(), o2.data_ptr(), float(grid2[2]), float(grid2[3]),
                  float(sqrt_d), out.data_ptr(), _stream())
    return out


def attention_probs_train_backward(raw, grad_out, mask, grid1, grid2, sqrt_d: float):
    """(grad_raw, [d s1, d o1, d s2, d o2]) of attention_probs_train."""
    raw, g = _f32(_dev(raw, "raw"), "raw", True), _f32(_dev(grad_out, "grad_out"), "grad_out", True)
    if g.shape != raw.shape:
        raise RuntimeError(f"mobilequant_amd: grad_out must have raw's shape {tuple(raw.shape)} (got {tuple(g.shape)})")
    rows, cols, m, (s1, o1, s2, o2) = _attn_probs_args(raw, mask, grid1, grid2)
    graw = torch.empty_like(raw)
    gg = torch.zeros(4, dtype=torch.float32, device=raw.device)
    with _on(raw, g, m, s1, o1, s2, o2):
        _lib.call("mq_attention_probs_train_backward", raw.data_ptr(), g.data_ptr(), rows, cols, m.data_ptr() if m is not None else None,
                  m.shape[0] if m is not None else 1, s1.data_ptr(), o1.data_ptr(), float(grid1[2]), float(grid1[3]), s2.data_ptr(), o2.data_ptr(),
                  float(grid2[2]), float(grid2[3]), float(sqrt_d), graw.data_ptr(), gg.data_ptr(), _stream())
    return graw, gg


def quantize(x: torch.Tensor, scale: torch.Tensor, offset: torch.Tensor, qmin: float, qmax: float, *,
             q_dtype: int = MQ_I8, shift: int = 0, rows: Optional[int] = None, want_row_sum: bool = False,
             chan_scale: Optional[torch.Tensor] = None):
    """Integer indices (qmodule.py:286-287) as integers; optional per-row sums of the stored values.
    x is viewed as [rows, -1]; rows defaults to the number of scales (per-row) or all leading dims.
    chan_scale [cols]: SmoothQuant per-channel scale fused in front (index of x / chan_scale; per-tensor grids, fp32)."""
    x = _dev(x, "x").contiguous()
    s, o = _f32(scale, "scale"), _f32(offset, "offset")
    _same_len(s, o, "scale", "offset")
    if rows is None:
        rows = s.numel() if s.numel() > 1 else (x.numel() // x.shape[-1] if x.dim() > 0 else 1)
    rows = int(rows)
    if rows < 1 or x.numel() % rows or s.numel() not in (1, rows):
        raise RuntimeError(f"mobilequant_amd: quantize rows={rows} must divide x's {x.numel()} elements and take 1 or {rows} scales "
                           f"(got {s.numel()})")
    cols = x.numel() // max(rows, 1)
    q = torch.empty(x.shape, dtype=_QDT[q_dtype], device=x.device)
    rs = torch.empty(rows, dtype=torch.int32, device=x.device) if want_row_sum else None
    cs = _chan(chan_scale, cols, x)
    with _on(x, s, o, cs):
        _lib.call("mq_quantize", x.data_ptr(), _fdt(x), rows, cols, s.data_ptr(), o.data_ptr(), s.numel(), float(qmin),
                  float(qmax), int(shift), cs.data_ptr() if cs is not None else None, q.data_ptr(), q_dtype,
                  rs.data_ptr() if rs is not None else None, _stream())
    return (q, rs) if want_row_sum else q


# ---- a8 --------------------------------------------------------------------------------------------
def linear_epilogue_prepare(a_scale, a_offset, a_shift: int, w_scale, w_offset, w_shift: int, w_colsum, K: int):
    sa, oa = _f32(a_scale, "a_scale"), _f32(a_offset, "a_offset")
    sw, ow = _f32(w_scale, "w_scale"), _f32(w_offset, "w_offset")
    _same_len(sa, oa, "a_scale", "a_offset"), _same_len(sw, ow, "w_scale", "w_offset")
    _raw(w_colsum, "w_colsum", torch.int32)
    N = w_colsum.numel()
    if sa.numel() != 1 or sw.numel() not in (1, N):
        raise RuntimeError(f"mobilequant_amd: linear_epilogue_prepare takes a per-tensor activation grid (a_scale, a_offset of one element) "
                           f"and 1 or {N} weight scales (w_scale, w_offset) (got {sa.numel()}, {sw.numel()})")
    dev = w_colsum.device
    alpha = torch.empty(N, dtype=torch.float32, device=dev)
    w_zp = torch.empty(N, dtype=torch.int32, device=dev)
    col_term = torch.empty(N, dtype=torch.int32, device=dev)
    with _on(w_colsum, sa, oa, sw, ow):
        _lib.call("mq_linear_epilogue_prepare", sa.data_ptr(), oa.data_ptr(), int(a_shift), sw.data_ptr(), ow.data_ptr(),
                  sw.numel(), int(w_shift), w_colsum.data_ptr(), N, int(K), alpha.data_ptr(), w_zp.data_ptr(),
                  col_term.data_ptr(), _stream())
    return alpha, w_zp, col_term


_OUT_TORCH = {MQ_F32: torch.float32, MQ_F16: torch.float16, MQ_U8: torch.uint8, MQ_I8: torch.int8,
              MQ_U16: torch.uint16, MQ_I16: torch.int16}


def _gemm_images(a_q: torch.Tensor, w_q: torch.Tensor, w4: bool, a_tiled_rows: Optional[int], what_a: str = "a_q", what_w: str = "w_q"):
    """(M, N, K) of an integer GEMM whose two byte images go to the entry by pointer: a_q [M, K] (a_tiled_rows = M: the fragment-blocked
    [>= ceil16(M), K] buffer), w_q [N, K] or, packed, [N, K / 2]."""
    _raw(a_q, what_a, _I8), _raw(w_q, what_w, _I8)
    if a_q.dim() != 2 or w_q.dim() != 2:
        raise RuntimeError(f"mobilequant_amd: {what_a} and {what_w} must be 2-D byte images (got {tuple(a_q.shape)}, {tuple(w_q.shape)})")
    M, K = a_q.shape
    if a_tiled_rows is not None:
        M = int(a_tiled_rows)
        if M < 1 or (M + 15) // 16 * 16 > a_q.shape[0]:
            raise RuntimeError(f"mobilequant_amd: {what_a} holds {a_q.shape[0]} rows, the fragment-blocked image of {M} rows needs "
                               f"{(M + 15) // 16 * 16}")
    if w_q.shape[1] * (2 if w4 else 1) != K:
        raise RuntimeError(f"mobilequant_amd: {what_w} {tuple(w_q.shape)} does not match {what_a}'s K = {K}"
                           + (" (packed nibbles: [N, K / 2])" if w4 else ""))
    return M, w_q.shape[0], K


def _gemm_vectors(M: int, N: int, a_rowsum, alpha, w_zp, col_term, sfx: str = "") -> None:
    """The epilogue vectors of an integer GEMM, read by pointer: a_rowsum int32 [>= M] or None, alpha fp32, w_zp / col_term int32 [>= N]."""
    if a_rowsum is not None:
        _raw(a_rowsum, "a_rowsum", torch.int32, M, at_least=True)
    _raw(alpha, "alpha" + sfx, torch.float32, N, at_least=True)
    _raw(w_zp, "w_zp" + sfx, torch.int32, N, at_least=True)
    _raw(col_term, "col_term" + sfx, torch.int32, N, at_least=True)


def _gemm_bias(bias, N: int):
    """The bias of an integer GEMM as contiguous, 16-byte aligned float32 with one entry per output column (None stays None)."""
    if bias is None:
        return None
    b = _f32(bias, "bias", True)
    if b.numel() != N:
        raise RuntimeError(f"mobilequant_amd: bias must hold {N} elements, one per output column (got {b.numel()})")
    return b


def _gemm_out(out: Optional[torch.Tensor], M: int, N: int, out_dtype: int, like: torch.Tensor) -> torch.Tensor:
    if out is None:
        return torch.empty((M, N), dtype=_OUT_TORCH[out_dtype], device=like.device)
    return _raw(out, "out", _OUT_TORCH[out_dtype], M * N)


def int8_linear(a_q: torch.Tensor, w_q: torch.Tensor, a_rowsum: Optional[torch.Tensor], alpha: torch.Tensor,
                w_zp: torch.Tensor, col_term: torch.Tensor, bias: Optional[torch.Tensor] = None, *,
                out_scale: Optional[torch.Tensor] = None, out_offset: Optional[torch.Tensor] = None,
                out_qmin: float = 0.0, out_qmax: float = 255.0, out_dtype: int = MQ_F32, w4: bool = False,
                out: Optional[torch.Tensor] = None, a_tiled_rows: Optional[int] = None,
                resid: Optional[torch.Tensor] = None) -> torch.Tensor:
    """QLinear as an int8 MFMA GEMM with fused dequant (+ output quantizer).  a_q [M,K] int8, w_q [N,K]
    int8 (or [N,K/2] packed nibbles when w4).  a_tiled_rows = M: a_q is the fragment-blocked buffer of
    quantize_tiled ([ceil16(M), K] bytes) and the generated-ISA GEMM path runs (gemm_tiled_supported shapes).
    resid [M, N] fp32 (row-major int8 weights and activations, fp32 output, M > 8): out = resid + Qout(linear), the add fused into
    the GEMM's store (residual_supported())."""
    M, N, K = _gemm_images(a_q, w_q, w4 and not (a_tiled_rows is not None and resid is None), a_tiled_rows)
    _gemm_vectors(M, N, a_rowsum, alpha, w_zp, col_term)
    out = _gemm_out(out, M, N, out_dtype, a_q)
    b = _gemm_bias(bias, N)
    os_ = _f32(out_scale, "out_scale") if out_scale is not None else None
    oo_ = _f32(out_offset, "out_offset") if out_offset is not None else None
    if resid is not None:
        if w4 and a_tiled_rows is None:
            raise RuntimeError("mobilequant_amd: int8_linear(resid=..., w4=True) needs the fragment-blocked activation image (a_tiled_rows)")
        if out_dtype != MQ_F32 or M <= 8:
            raise RuntimeError("mobilequant_amd: int8_linear(resid=...) needs fp32 output and M > 8")
        if a_tiled_rows is not None and not (os_ is not None and out_qmax - out_qmin > 255.0 and gemm_tiled128_supported(M, N, K)):
            raise RuntimeError("mobilequant_amd: int8_linear(resid=..., a_tiled_rows=...) needs a 16-bit output grid and a "
                               "gemm_tiled128_supported shape")
        resid = _f32(_dev(resid, "resid"), "resid", True)
        if resid.numel() != M * N or resid.data_ptr() == out.data_ptr():
            raise RuntimeError("mobilequant_amd: resid must be [M, N] and must not alias the output")
        with _on(a_q, w_q, a_rowsum, alpha, w_zp, col_term, b, os_, oo_, out, resid):
            _lib.call(("mq_w4a8_linear_tiled_residual" if w4 else "mq_w8a8_linear_tiled_residual") if a_tiled_rows is not None else "mq_w8a8_linear_residual",
                      a_q.data_ptr(), w_q.data_ptr(), M, N, K,
                      a_rowsum.data_ptr() if a_rowsum is not None else None, alpha.data_ptr(), w_zp.data_ptr(), col_term.data_ptr(),
                      b.data_ptr() if b is not None else None, os_.data_ptr() if os_ is not None else None,
                      oo_.data_ptr() if oo_ is not None else None, float(out_qmin), float(out_qmax), resid.data_ptr(), out.data_ptr(),
                      _stream())
        return out
    fn = "mq_w8a8_linear_tiled" if a_tiled_rows is not None else ("mq_w4a8_linear" if w4 else "mq_w8a8_linear")
    with _on(a_q, w_q, a_rowsum, alpha, w_zp, col_term, b, os_, oo_, out):
        _lib.call(fn, a_q.data_ptr(), w_q.data_ptr(), M, N, K,
                  a_rowsum.data_ptr() if a_rowsum is not None else None, alpha.data_ptr(), w_zp.data_ptr(),
                  col_term.data_ptr(), b.data_ptr() if b is not None else None,
                  os_.data_ptr() if os_ is not None else None, oo_.data_ptr() if oo_ is not None else None,
                  float(out_qmin), float(out_qmax), out.data_ptr(), out_dtype, _stream())
    return out


def int8_linear_grouped(a_q: torch.Tensor, w_q: torch.Tensor, group_size: int, a_gsum: torch.Tensor, alpha: torch.Tensor, cw: torch.Tensor,
                        t: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """QLinear with per-group weight grids as an int8 MFMA GEMM (mq_w8a8_linear_grouped): a_q [M, K] / w_q [N, K] stored int8 values,
    a_gsum [G, M] int32, alpha [G, N] fp32, cw / t [G, N] int32 (include/mobilequant_amd.h); fp32 [M, N] out."""
    M, N, K = _gemm_images(a_q, w_q, False, None)
    gs_ = int(group_size)
    if gs_ < 1 or K % gs_:
        raise RuntimeError(f"mobilequant_amd: int8_linear_grouped group_size={group_size} must divide K = {K}")
    G = K // gs_
    out = torch.empty((M, N), dtype=torch.float32, device=a_q.device)
    b = _gemm_bias(bias, N)
    al = _f32(alpha, "alpha", True)
    _raw(a_gsum, "a_gsum", torch.int32, G * M, at_least=True), _raw(cw, "cw", torch.int32, G * N, at_least=True)
    _raw(t, "t", torch.int32, G * N, at_least=True)
    if al.numel() < G * N:
        raise RuntimeError(f"mobilequant_amd: alpha must hold {G * N} elements (got {al.numel()})")
    with _on(a_q, w_q, a_gsum, al, cw, t, b):
        _lib.call("mq_w8a8_linear_grouped", a_q.data_ptr(), w_q.data_ptr(), M, N, K, int(group_size), a_gsum.data_ptr(), al.data_ptr(),
                  cw.data_ptr(), t.data_ptr(), b.data_ptr() if b is not None else None, out.data_ptr(), _stream())
    return out


def decode_gemv_grouped(args: "_lib.MqDecodeGemvGroupedArgs") -> None:
    """mq_decode_gemv_grouped on the current stream: the five-launch decode GEMV with per-group weight grids for 1 .. 8 activation rows.
    args is a filled _lib.MqDecodeGemvGroupedArgs (include/mobilequant_amd.h); the tensors it points into stay alive until it has run."""
    _lib.call("mq_decode_gemv_grouped", ctypes.byref(args), _stream())


def decode_attention_multi(args: "_lib.MqDecodeAttentionMultiArgs") -> None:
    """mq_decode_attention_multi on the current stream: the decode attention of args.rows consecutive positions of one sequence (from
    *args.a.pos on) in one launch, appending them to its caches.  args is a filled _lib.MqDecodeAttentionMultiArgs
    (include/mobilequant_amd.h); the tensors it points into stay alive until it has run."""
    _lib.call("mq_decode_attention_multi", ctypes.byref(args), _stream())


def decode_attention_ragged(args: "_lib.MqDecodeAttentionRaggedArgs") -> None:
    """mq_decode_attention_ragged on the current stream: the decode attention of args.rows table rows -- row r the position
    row_pos[r] of sequence row_seq[r] (device arrays), consecutive rows of one sequence at consecutive positions seeing each other --
    over args.batch caches in one launch, appending the named positions.  A sequence may appear in at most one run per launch.  args is
    a filled _lib.MqDecodeAttentionRaggedArgs (include/mobilequant_amd.h); the tensors it points into stay alive until it has run."""
    _lib.call("mq_decode_attention_ragged", ctypes.byref(args), _stream())


def decode_cache_table(caches) -> torch.Tensor:
    """The int64 device table of the caches' base pointers that decode_cache_fork takes as table=: built once for caches that are
    never reallocated (the tensors must outlive it)."""
    return torch.tensor([c.data_ptr() for c in caches], dtype=torch.int64).to(caches[0].device)


def _cache_slots_call(who: str, caches, pos: torch.Tensor, parent: torch.Tensor, table: Optional[torch.Tensor]) -> None:
    """The argument checks and the call of decode_cache_fork / decode_cache_reorder (who: the operation's name; one argument block)."""
    caches = list(caches)
    if not caches:
        raise ValueError(f"mobilequant_amd: {who} needs at least one cache")
    c0 = caches[0]
    if not isinstance(c0, torch.Tensor) or c0.dim() != 4:
        raise ValueError(f"mobilequant_amd: {who}: a cache is a tensor [batch, kv_heads, cache_len, head_dim], got {getattr(c0, 'shape', type(c0))}")
    for t in caches:                                               # (what a cache is, then where it lives: a CPU tensor is refused last)
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int8:
            raise RuntimeError(f"mobilequant_amd: {who}: caches are int8 tensors, got {getattr(t, 'dtype', type(t))}")
        if t.shape != c0.shape:
            raise ValueError(f"mobilequant_amd: {who}: caches of different shapes ({tuple(c0.shape)} vs {tuple(t.shape)})")
        if not t.is_contiguous():
            raise RuntimeError(f"mobilequant_amd: {who}: a cache is not contiguous")
    B, H, L, D = (int(v) for v in c0.shape)
    for t, what in ((pos, "pos"), (parent, "parent")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or tuple(t.shape) != (B,) or not t.is_contiguous():
            raise RuntimeError(f"mobilequant_amd: {who}: {what} must be a contiguous int32 [{B}] tensor, got "
                               f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
    if D % 16 or not 16 <= D <= 256:
        raise ValueError(f"mobilequant_amd: {who}: head_dim={D} must be a multiple of 16 in [16, 256]")
    if not 1 <= B <= 8 or not 1 <= len(caches) <= 1024 or H < 1 or L < 1:
        raise ValueError(f"mobilequant_amd: {who}: {len(caches)} caches of shape {tuple(c0.shape)} outside the launch's limits "
                         "(1 .. 1024 caches, batch 1 .. 8, no empty dimension)")
    for t in caches + [pos, parent]:
        _dev(t, f"{who}: every cache, pos and parent")
    if any(t.data_ptr() % 16 for t in caches):
        raise RuntimeError(f"mobilequant_amd: {who}: a cache is not 16-byte aligned")
    if table is None:
        table = decode_cache_table(caches)
    else:
        _dev(table, f"{who}: table")
        if table.dtype != torch.int64 or tuple(table.shape) != (len(caches),) or not table.is_contiguous():
            raise RuntimeError(f"mobilequant_amd: {who}: table must be a contiguous int64 [{len(caches)}] tensor of the caches' base pointers")
    a = _lib.MqDecodeCacheForkArgs(table.data_ptr(), len(caches), B, H, L, D, pos.data_ptr(), parent.data_ptr())
    with _on(c0, *caches[1:], pos, parent, table):
        _lib.call("mq_" + who, ctypes.byref(a), _stream())


def decode_cache_fork(caches, pos: torch.Tensor, parent: torch.Tensor, table: Optional[torch.Tensor] = None) -> None:
    """mq_decode_cache_fork on the current stream (csrc/mq_decode_fork.hip): ONE launch copies the live part of every
    source slot of `caches` -- a list of int8 device tensors [batch, kv_heads, cache_len, head_dim], all of one shape, contiguous, on one
    device -- into its destination slots, in place.  pos / parent: int32 [batch] device tensors, read on the device: slot s is a source
    iff parent[s] == s; slot d with p = parent[d] != d takes bytes [0, pos[p] * head_dim) of every head of every cache from slot p iff
    p is in range, parent[p] == p and 0 <= pos[p] < cache_len; nothing else is written.  table: decode_cache_table(caches), prebuilt
    (otherwise it is built here: one host -> device copy).  RuntimeError / ValueError on any violation, before the C call."""
    _cache_slots_call("decode_cache_fork", caches, pos, parent, table)


def decode_cache_reorder(caches, pos: torch.Tensor, parent: torch.Tensor, table: Optional[torch.Tensor] = None) -> None:
    """mq_decode_cache_reorder on the current stream (csrc/mq_decode_reorder.hip): ONE launch assigns "slot d continues
    old slot parent[d]" for all slots of `caches` AT ONCE, in place -- decode_cache_fork's arguments (caches, pos, parent, table), but a
    source may itself be a destination: swaps, cycles, chains and fan-out from an overwritten slot.  Slot d with p = parent[d] takes
    bytes [0, pos[p] * head_dim) of every head of every cache from slot p, as they were before the call, iff p is in range, p != d and
    0 < pos[p] < cache_len; nothing else is written (the identity writes nothing).  RuntimeError / ValueError on any violation, before
    the C call."""
    _cache_slots_call("decode_cache_reorder", caches, pos, parent, table)


def beam_select(logits: torch.Tensor, cum: torch.Tensor, group: torch.Tensor, n_groups: int, n_cand: int, out=None, scratch: Optional[torch.Tensor] = None):
    """mq_beam_select on the current stream (csrc/mq_beam.hip): logits [rows, V] fp32 (row stride >= V; the RAW rows),
    cum [rows] fp32 and group [rows] int32 device tensors, n_groups in 1 .. 8, n_cand in 1 .. 20.  Returns device tensors (cand_score
    [n_groups, n_cand] fp32, cand_row int32, cand_token int32, cand_logprob fp32, row_lse [rows] fp32): per group the first n_cand
    (row, token) pairs by cum[row] + log-softmax(row)[token] descending, ties by row, then by the row's own order; -inf / -1 / -1 /
    -inf where a group has fewer.  A row whose group entry is outside [0, n_groups) is a member of nothing and is never read; row_lse
    is written for member rows only.  out: the five tensors of an earlier call, written in place (a captured launch); scratch: uint8
    [>= MQ_BEAM_SCRATCH_BYTES], owned by the call."""
    _dev(logits, "beam_select logits")
    if logits.dim() == 1:
        logits = logits.view(1, -1)
    if logits.dim() != 2 or logits.dtype != torch.float32 or logits.stride(1) != 1:
        raise RuntimeError("mobilequant_amd: beam_select logits must be fp32 [rows, V] with unit column stride")
    rows, V = logits.shape
    if not 1 <= rows <= 8:
        raise RuntimeError(f"mobilequant_amd: beam_select rows={rows} outside 1..8")
    for v, hi, what in ((n_groups, 8, "n_groups"), (n_cand, _lib.MQ_LOGPROB_MAX_TOP, "n_cand")):
        if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= hi:
            raise ValueError(f"mobilequant_amd: beam_select {what}={v!r} must be an int in 1..{hi}")
    for t, dt, what in ((cum, torch.float32, "cum"), (group, torch.int32, "group")):
        if not isinstance(t, torch.Tensor) or t.dtype != dt or tuple(t.shape) != (rows,) or not t.is_contiguous():
            raise RuntimeError(f"mobilequant_amd: beam_select {what} must be a contiguous {dt} [{rows}] tensor")
        _dev(t, "beam_select " + what)
    dev = logits.device
    if out is None:
        out = (torch.empty(n_groups, n_cand, dtype=torch.float32, device=dev), torch.empty(n_groups, n_cand, dtype=torch.int32, device=dev),
               torch.empty(n_groups, n_cand, dtype=torch.int32, device=dev), torch.empty(n_groups, n_cand, dtype=torch.float32, device=dev),
               torch.empty(rows, dtype=torch.float32, device=dev))
    else:
        out = tuple(out)
        want = [(torch.float32, (n_groups, n_cand)), (torch.int32, (n_groups, n_cand)), (torch.int32, (n_groups, n_cand)),
                (torch.float32, (n_groups, n_cand)), (torch.float32, (rows,))]
        if len(out) != 5 or any(not isinstance(t, torch.Tensor) or t.dtype != dt or tuple(t.shape) != sh or not t.is_contiguous() or t.device != dev
                                for t, (dt, sh) in zip(out, want)):
            raise RuntimeError(f"mobilequant_amd: beam_select out must be the five contiguous tensors of a call with n_groups={n_groups}, n_cand={n_cand}, rows={rows}")
    if scratch is None:
        scratch = torch.empty(_lib.MQ_BEAM_SCRATCH_BYTES, dtype=torch.uint8, device=dev)
    elif not isinstance(scratch, torch.Tensor) or scratch.dtype != torch.uint8 or scratch.numel() < _lib.MQ_BEAM_SCRATCH_BYTES or not scratch.is_contiguous() \
            or scratch.device != dev:
        raise RuntimeError(f"mobilequant_amd: beam_select scratch must be a contiguous uint8 device tensor of >= {_lib.MQ_BEAM_SCRATCH_BYTES} bytes")
    a = _lib.MqBeamSelectArgs()
    a.logits, a.logits_stride, a.V = logits.data_ptr(), logits.stride(0) if rows > 1 else max(V, logits.stride(0)), V
    a.rows, a.n_groups, a.n_cand = rows, n_groups, n_cand
    a.cum, a.group = cum.data_ptr(), group.data_ptr()
    a.cand_score, a.cand_row, a.cand_token, a.cand_logprob, a.row_lse = (t.data_ptr() for t in out)
    a.scratch, a.scratch_bytes = scratch.data_ptr(), scratch.numel()
    with _on(logits, cum, group, *out):
        _lib.call("mq_beam_select", ctypes.byref(a), _stream())
    return out


def int8_linear_segmented(a_q: torch.Tensor, w_q: torch.Tensor, a_rowsum: torch.Tensor, alpha: torch.Tensor, w_zp: torch.Tensor,
                          col_term: torch.Tensor, bias: Optional[torch.Tensor], seg_ends, grids, w4: bool = False,
                          a_tiled_rows: Optional[int] = None) -> torch.Tensor:
    """1..3 linears reading one row-major int8 activation as ONE GEMM (mq_w8a8_linear_segmented): w_q / alpha / w_zp / col_term /
    bias concatenated along N, seg_ends = cumulative column ends, grids[i] = (scale, offset) of segment i's 8-bit unsigned output
    grid.  Returns the uint8 output indices [M, N].  w4: w_q holds packed nibbles [N, K/2] (pack_w4).  a_tiled_rows = M: a_q is the
    fragment-blocked image (gemm_tiled128_supported shapes, int8 weights)."""
    fn = "mq_w4a8_linear_segmented" if w4 else "mq_w8a8_linear_segmented"
    if a_tiled_rows is not None:
        if w4:
            raise RuntimeError("mobilequant_amd: the fragment-blocked segmented GEMM takes int8 weights")
        fn = "mq_w8a8_linear_tiled_segmented"
    M, N, K = _gemm_images(a_q, w_q, w4, a_tiled_rows)
    _gemm_vectors(M, N, a_rowsum, alpha, w_zp, col_term)
    n = len(seg_ends)
    if len(grids) != n:
        raise RuntimeError(f"mobilequant_amd: int8_linear_segmented takes one grid per segment ({len(grids)} grids, {n} seg_ends)")
    out = torch.empty((M, N), dtype=torch.uint8, device=a_q.device)
    b = _gemm_bias(bias, N)
    ends = (ctypes.c_int64 * n)(*[int(e) for e in seg_ends])
    keep, gs = [], (_lib.MqGrid * n)()
    for i, g in enumerate(grids):
        sc, of = _f32(g[0], "scale"), _f32(g[1], "offset")
        if sc.numel() != 1 or of.numel() != 1:
            raise RuntimeError(f"mobilequant_amd: segment {i} takes a per-tensor grid: scale and offset of one element (got {sc.numel()}, {of.numel()})")
        keep += [sc, of]
        gs[i] = _lib.MqGrid(sc.data_ptr(), of.data_ptr(), 0.0, 255.0)
    with _on(a_q, w_q, a_rowsum, alpha, w_zp, col_term, b, out, *keep):
        _lib.call(fn, a_q.data_ptr(), w_q.data_ptr(), M, N, K, a_rowsum.data_ptr() if a_rowsum is not None else None,
                  alpha.data_ptr(), w_zp.data_ptr(), col_term.data_ptr(), b.data_ptr() if b is not None else None, n, ends, gs,
                  out.data_ptr(), _stream())
    return out


def gemm_tiled_w4_supported(M: int, N: int, K: int) -> bool:
    """Shapes served by the packed-4-bit generated kernels on fragment-blocked activations (mq_w4a8_linear_tiled)."""
    return bool(_lib.load().mq_gemm_tiled_w4_supported(int(M), int(N), int(K)))


def w4a8_linear_tiled(a_tiled: torch.Tensor, M: int, w_packed: torch.Tensor, a_rowsum: Optional[torch.Tensor], alpha: torch.Tensor,
                      w_zp: torch.Tensor, col_term: torch.Tensor, bias: Optional[torch.Tensor], grids, seg_ends=None,
                      out_dtype: int = MQ_U8, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Packed 4-bit weights [N, K/2] (pack_w4) x fragment-blocked int8 activations (quantize_tiled, M rows) on the generated-ISA kernels
    (mq_w4a8_linear_tiled): 8-bit unsigned output grid(s) -> uint8 indices (or int8 = index - 128) [M, N].  grids: [(scale, offset)] per
    column segment; seg_ends: cumulative column ends when there is more than one."""
    M, N, K = _gemm_images(a_tiled, w_packed, True, M, "a_tiled", "w_packed")
    _gemm_vectors(M, N, a_rowsum, alpha, w_zp, col_term)
    n = len(grids)
    if len(seg_ends if seg_ends is not None else [N]) != n:
        raise RuntimeError(f"mobilequant_amd: w4a8_linear_tiled takes one grid per segment ({n} grids)")
    out = _gemm_out(out, M, N, out_dtype, a_tiled)
    b = _gemm_bias(bias, N)
    ends = (ctypes.c_int64 * n)(*[int(e) for e in (seg_ends if seg_ends is not None else [N])])
    keep, gs = [], (_lib.MqGrid * n)()
    for i, g in enumerate(grids):
        sc, of = _f32(g[0], "scale"), _f32(g[1], "offset")
        if sc.numel() != 1 or of.numel() != 1:
            raise RuntimeError(f"mobilequant_amd: segment {i} takes a per-tensor grid: scale and offset of one element (got {sc.numel()}, {of.numel()})")
        keep += [sc, of]
        gs[i] = _lib.MqGrid(sc.data_ptr(), of.data_ptr(), 0.0, 255.0)
    with _on(a_tiled, w_packed, a_rowsum, alpha, w_zp, col_term, b, out, *keep):
        _lib.call("mq_w4a8_linear_tiled", a_tiled.data_ptr(), w_packed.data_ptr(), int(M), N, K,
                  a_rowsum.data_ptr() if a_rowsum is not None else None, alpha.data_ptr(), w_zp.data_ptr(), col_term.data_ptr(),
                  b.data_ptr() if b is not None else None, n, ends, gs, out.data_ptr(), out_dtype, _stream())
    return out


def gemm_tiled128_supported(M: int, N: int, K: int) -> bool:
    """Shapes served by the 128-column generated kernels on fragment-blocked activations (o_proj / w2 with the residual, q | k | v)."""
    return bool(_lib.load().mq_gemm_tiled128_supported(int(M), int(N), int(K)))


def gemm_tiled_supported(M: int, N: int, K: int) -> bool:
    """Shapes served by the fragment-blocked activation layout + generated-ISA GEMM loop (TinyLlama / StableLM FFN)."""
    return bool(_lib.load().mq_gemm_tiled_supported(int(M), int(N), int(K)))


def quantize_tiled(x2d: torch.Tensor, scale: torch.Tensor, offset: torch.Tensor, qmin: float, qmax: float, shift: int,
                   want_row_sum: bool = True, chan_scale: Optional[torch.Tensor] = None):
    """[M,K] activations -> fragment-blocked int8 ([ceil16(M), K] buffer, layout: include/mobilequant_amd.h) + row sums."""
    x2d = _dev(x2d, "x").contiguous()
    if x2d.dim() != 2:
        raise RuntimeError(f"mobilequant_amd: quantize_tiled x must be [M, K] (got {tuple(x2d.shape)})")
    if x2d.data_ptr() % 16:              # the entry takes 16-byte aligned activations and channel scales: a view off that boundary is copied
        x2d = x2d.clone()
    M, K = x2d.shape
    q = torch.empty(((M + 15) // 16 * 16, K), dtype=torch.int8, device=x2d.device)
    rs = torch.empty(M, dtype=torch.int32, device=x2d.device) if want_row_sum else None
    s, o = _f32(scale, "scale"), _f32(offset, "offset")
    _same_len(s, o, "scale", "offset")
    if s.numel() != 1:
        raise RuntimeError(f"mobilequant_amd: quantize_tiled takes a per-tensor grid: scale and offset of one element (got {s.numel()})")
    cs = _chan(chan_scale, K, x2d)
    if cs is not None and cs.data_ptr() % 16:
        cs = cs.clone()
    with _on(x2d, s, o, cs):
        _lib.call("mq_quantize_tiled", x2d.data_ptr(), _fdt(x2d), M, K, s.data_ptr(), o.data_ptr(), float(qmin), float(qmax),
                  int(shift), cs.data_ptr() if cs is not None else None, q.data_ptr(), rs.data_ptr() if rs is not None else None,
                  _stream())
    return (q, rs) if want_row_sum else q


def decode_shape(M: int, K: int) -> bool:
    """Shapes mq_w8a8_linear_f32in accepts (activation quantize fused into the weight-streaming GEMV)."""
    return M <= 8 and M * K <= 64 * 1024 - 64 and K % 256 == 0


def int8_linear_f32in(x2d: torch.Tensor, a_scale, a_offset, a_qmin: float, a_qmax: float, a_shift: int, w_q: torch.Tensor,
                      alpha, w_zp, col_term, bias=None, *, out_scale=None, out_offset=None, out_qmin: float = 0.0,
                      out_qmax: float = 255.0, out_dtype: int = MQ_F32, out: Optional[torch.Tensor] = None, w4: bool = False):
    """Decode-shape QLinear in ONE kernel: fp32 activations are quantised inside the GEMV (M <= 8).
    w4: w_q holds packed nibbles ([N, K/2], pack_w4)."""
    x2d = _f32(_dev(x2d, "x"), "x", True)
    if x2d.dim() != 2:
        raise RuntimeError(f"mobilequant_amd: int8_linear_f32in x must be [M, K] (got {tuple(x2d.shape)})")
    M, K = x2d.shape
    _raw(w_q, "w_q", _I8)
    if w_q.dim() != 2 or w_q.shape[1] * (2 if w4 else 1) != K:
        raise RuntimeError(f"mobilequant_amd: w_q {tuple(w_q.shape)} does not match x's K = {K}" + (" (packed nibbles: [N, K / 2])" if w4 else ""))
    N = w_q.shape[0]
    _gemm_vectors(M, N, None, alpha, w_zp, col_term)
    out = _gemm_out(out, M, N, out_dtype, x2d)
    sa, oa = _f32(a_scale, "a_scale"), _f32(a_offset, "a_offset")
    b = _gemm_bias(bias, N)
    os_ = _f32(out_scale, "out_scale") if out_scale is not None else None
    oo_ = _f32(out_offset, "out_offset") if out_offset is not None else None
    with _on(x2d, sa, oa, w_q, alpha, w_zp, col_term, b, os_, oo_, out):
        _lib.call("mq_w4a8_linear_f32in" if w4 else "mq_w8a8_linear_f32in", x2d.data_ptr(), sa.data_ptr(), oa.data_ptr(), float(a_qmin), float(a_qmax), int(a_shift),
                  w_q.data_ptr(), M, N, K, alpha.data_ptr(), w_zp.data_ptr(), col_term.data_ptr(),
                  b.data_ptr() if b is not None else None, os_.data_ptr() if os_ is not None else None,
                  oo_.data_ptr() if oo_ is not None else None, float(out_qmin), float(out_qmax), out.data_ptr(), out_dtype,
                  _stream())
    return out


def rmsnorm_quant(x: torch.Tensor, weight: torch.Tensor, bias, eps: float, in_grid=None, out_grid=None, emit_int8: bool = False,
                  layernorm: bool = False, emit_tiled: bool = False, want_y: bool = True, emit_rowmajor: bool = True):
    """QRMSNorm.forward (layernorm=True: QLayerNorm.forward) in one launch.  in_grid / out_grid: None or
    (scale, offset, qmin, qmax) per-tensor.  Returns y, or (y, q_int8, row_sum, shift, q_tiled) with emit_int8
    (8-bit output grids only; q_tiled = the fragment-blocked copy when emit_tiled, else None).  want_y=False (emit_int8 only): the
    fp32 result is not written (y = None); emit_rowmajor=False: only the fragment-blocked image (q_int8 = None)."""
    x = _f32(_dev(x, "x"), "x", True)
    cols = x.shape[-1]
    rows = x.numel() // cols
    w = _f32(weight, "weight", True)
    b = _f32(bias, "bias", True) if bias is not None else None
    if w.numel() != cols or (b is not None and b.numel() != cols):
        raise RuntimeError(f"mobilequant_amd: rmsnorm_quant weight / bias must hold {cols} elements (got {w.numel()}"
                           + (f", {b.numel()}" if b is not None else "") + ")")
    if not want_y and not emit_int8:
        raise RuntimeError("mobilequant_amd: rmsnorm_quant(want_y=False) needs emit_int8")
    y = torch.empty_like(x) if want_y else None
    si = oi = so = oo = None
    iqmin = iqmax = oqmin = oqmax = 0.0
    if in_grid is not None:
        si, oi, iqmin, iqmax = _f32(in_grid[0], "in_scale"), _f32(in_grid[1], "in_offset"), float(in_grid[2]), float(in_grid[3])
    if out_grid is not None:
        so, oo, oqmin, oqmax = _f32(out_grid[0], "out_scale"), _f32(out_grid[1], "out_offset"), float(out_grid[2]), float(out_grid[3])
    for sg, og in ((si, oi), (so, oo)):
        if sg is not None and (sg.numel() != 1 or og.numel() != 1):
            raise RuntimeError(f"mobilequant_amd: rmsnorm_quant takes per-tensor grids: in_scale / in_offset / out_scale / out_offset of one "
                               f"element (got {sg.numel()}, {og.numel()})")
    q = rs = qt = None
    shift = 0
    if emit_int8:
        shift = 128 if oqmax > 127 else 0
        if emit_rowmajor or not emit_tiled:
            q = torch.empty((rows, cols), dtype=torch.int8, device=x.device)
        rs = torch.empty(rows, dtype=torch.int32, device=x.device)
        if emit_tiled:
            qt = torch.empty(((rows + 15) // 16 * 16, cols), dtype=torch.int8, device=x.device)
    with _on(x, w, b, si, oi, so, oo):
        _lib.call("mq_layernorm_quant" if layernorm else "mq_rmsnorm_quant", x.data_ptr(), rows, cols, w.data_ptr(),
                  b.data_ptr() if b is not None else None, float(eps),
                  si.data_ptr() if si is not None else None, oi.data_ptr() if oi is not None else None, iqmin, iqmax,
                  so.data_ptr() if so is not None else None, oo.data_ptr() if oo is not None else None, oqmin, oqmax,
                  y.data_ptr() if y is not None else None, q.data_ptr() if q is not None else None,
                  qt.data_ptr() if qt is not None else None, shift,
                  rs.data_ptr() if rs is not None else None, _stream())
    return (y, q, rs, shift, qt) if emit_int8 else y


def act_quant(x: torch.Tensor, act: str, in_grid=None, mid_grid=None, out_grid=None):
    """QSiLU ("silu") / QGELU ("gelu") forward in one launch; grids: None or (scale, offset, qmin, qmax) per-tensor."""
    x = _f32(_dev(x, "x"), "x", True)
    y = torch.empty_like(x)
    ptrs, keep = [], []
    for g in (in_grid, mid_grid, out_grid):
        if g is None:
            ptrs += [None, None, 0.0, 0.0]
        else:
            s, o = _f32(g[0], "scale"), _f32(g[1], "offset")        # a converted copy lives in `keep` until the launch is queued
            if s.numel() != 1 or o.numel() != 1:
                raise RuntimeError(f"mobilequant_amd: act_quant takes per-tensor grids: scale and offset of one element (got {s.numel()}, {o.numel()})")
            keep += [s, o]
            ptrs += [s.data_ptr(), o.data_ptr(), float(g[2]), float(g[3])]
    with _on(x, *keep):
        _lib.call("mq_act_quant", x.data_ptr(), x.numel(), {"silu": 0, "gelu": 1}[act], *ptrs, y.data_ptr(), _stream())
    return y


def pack_w4(nibbles: torch.Tensor) -> torch.Tensor:
    """[N,K] uint8 nibbles (0..15) -> [N,K/2] packed (layout: include/mobilequant_amd.h, mq_pack_w4)."""
    nibbles = _dev(nibbles, "nibbles")
    if nibbles.dtype != torch.uint8 or nibbles.dim() != 2 or nibbles.shape[1] % 2:
        raise RuntimeError(f"mobilequant_amd: nibbles must be a uint8 [N, K] tensor with K even (got {nibbles.dtype}, {tuple(nibbles.shape)})")
    nibbles = nibbles.contiguous()
    N, K = nibbles.shape
    packed = torch.empty((N, K // 2), dtype=torch.uint8, device=nibbles.device)
    with _on(nibbles):
        _lib.call("mq_pack_w4", nibbles.data_ptr(), N, K, packed.data_ptr(), _stream())
    return packed


# ---- f1: integer chaining inside the gated FFN ---------------------------------------------------------------------------------
def _pair_halves(M: int, N: int, a_rowsum, first: dict, second: dict) -> None:
    """Both halves of a two-linear launch: the second's weight image has the first's shape and dtype, each half's vectors hold N entries."""
    _raw(second["w"], "second['w']", _I8)
    if second["w"].shape != first["w"].shape or second["w"].dtype != first["w"].dtype:
        raise RuntimeError(f"mobilequant_amd: second['w'] {tuple(second['w'].shape)} {second['w'].dtype} must match first['w'] "
                           f"{tuple(first['w'].shape)} {first['w'].dtype}")
    for p, sfx in ((first, " (first)"), (second, " (second)")):
        _gemm_vectors(M, N, a_rowsum, p["alpha"], p["w_zp"], p["col_term"], sfx)


def _half_grid(p: dict, N: int, keep: list):
    """(bias | None, out_scale, out_offset) of one half as contiguous float32, kept alive in `keep`; the grid is per-tensor."""
    b = _gemm_bias(p.get("bias"), N)
    os_, oo_ = _f32(p["out_scale"], "out_scale"), _f32(p["out_offset"], "out_offset")
    if os_.numel() != 1 or oo_.numel() != 1:
        raise RuntimeError(f"mobilequant_amd: out_scale and out_offset hold one element each (got {os_.numel()}, {oo_.numel()})")
    keep += [b, os_, oo_]
    return b, os_, oo_


def int8_linear_pair(a_tiled: torch.Tensor, rows: int, a_rowsum: Optional[torch.Tensor], first: dict, second: dict,
                     out_dtype: int = MQ_U8):
    """Two QLinears over the SAME fragment-blocked activation in one launch (w1 / w3 of a gated FFN).  `first` / `second`:
    dicts with w [N,K] int8, alpha, w_zp, col_term, bias (or None), out_scale, out_offset (8-bit unsigned output grids).
    Returns the two [rows, N] index tensors (u8, or i8 = index - 128)."""
    M, N, K = _gemm_images(a_tiled, first["w"], False, rows, "a_tiled", "first['w']")
    _pair_halves(M, N, a_rowsum, first, second)
    outs = [torch.empty((M, N), dtype=_OUT_TORCH[out_dtype], device=a_tiled.device) for _ in range(2)]
    ptrs, keep = [], []
    for p, o in zip((first, second), outs):
        b, os_, oo_ = _half_grid(p, N, keep)
        ptrs += [p["w"].data_ptr(), p["alpha"].data_ptr(), p["w_zp"].data_ptr(), p["col_term"].data_ptr(),
                 b.data_ptr() if b is not None else None, os_.data_ptr(), oo_.data_ptr(), o.data_ptr()]
    with _on(a_tiled, a_rowsum, first["w"], second["w"], first["alpha"], second["alpha"], *[k for k in keep if k is not None]):
        _lib.call("mq_w8a8_linear_tiled_pair", a_tiled.data_ptr(), M, N, K, a_rowsum.data_ptr() if a_rowsum is not None else None,
                  *ptrs, out_dtype, _stream())
    return outs[0], outs[1]


def int8_linear_gated(a_tiled: torch.Tensor, rows: int, a_rowsum: Optional[torch.Tensor], first: dict, second: dict, table: torch.Tensor,
                      w4: bool = False):
    """w1, w3 and the gate of a gated FFN in TWO launches (mq_w8a8_linear_tiled_gated): `first` (w1) writes its 8-bit indices, `second`
    (w3) looks (w1 index, w3 index) up in `table` (gated_table) inside its epilogue.  Returns (w2's int8 input image, fragment-blocked
    [ceil16(rows), N]; its row sums [rows]) -- the bits of int8_linear_pair + gated_lookup(tiled=True)."""
    # w4: both weights are mq_pack_w4 images ([N, K / 2] bytes) and the packed kernels run (mq_w4a8_linear_tiled_gated: identical bytes)
    M, N, K = _gemm_images(a_tiled, first["w"], w4, rows, "a_tiled", "first['w']")
    _pair_halves(M, N, a_rowsum, first, second)
    dev = a_tiled.device
    if _dev(table, "table").dtype != torch.int8 or table.numel() != 65536 or not table.is_contiguous():
        raise RuntimeError("mobilequant_amd: int8_linear_gated needs an int8 [65536] table (gated_table)")
    idx = torch.empty((M, N), dtype=torch.uint8, device=dev)
    q = torch.empty(((M + 15) // 16 * 16, N), dtype=torch.int8, device=dev)
    rs = torch.empty(M, dtype=torch.int32, device=dev)
    ptrs, keep = [], []
    for p in (first, second):
        b, os_, oo_ = _half_grid(p, N, keep)
        ptrs += [p["w"].data_ptr(), p["alpha"].data_ptr(), p["w_zp"].data_ptr(), p["col_term"].data_ptr(),
                 b.data_ptr() if b is not None else None, os_.data_ptr(), oo_.data_ptr()]
    with _on(a_tiled, a_rowsum, first["w"], second["w"], first["alpha"], second["alpha"], table, *[k for k in keep if k is not None]):
        _lib.call("mq_w4a8_linear_tiled_gated" if w4 else "mq_w8a8_linear_tiled_gated", a_tiled.data_ptr(), M, N, K,
                  a_rowsum.data_ptr() if a_rowsum is not None else None,
                  *ptrs, table.data_ptr(), idx.data_ptr(), q.data_ptr(), rs.data_ptr(), _stream())
    return q, rs


def gated_act_quant(a: torch.Tensor, b: torch.Tensor, act: str, out_grid, *, a_grid=None, b_grid=None, mid_grid=None, act_grid=None,
                    q_shift: int = 128, want_y: bool = False):
    """act(a) * b -> int8 image on `out_grid` (+ row sums, + the fp32 product when want_y) in one launch: the gated FFN between
    the w1 / w3 GEMMs and w2.  a / b: fp32 values [rows, cols], or uint8 output indices of the GEMMs with their grids
    (a_grid / b_grid).  Grids: (scale, offset, qmin, qmax) per-tensor or None."""
    a, b = _al16(_dev(a, "a").contiguous()), _al16(_dev(b, "b").contiguous())
    if a.dtype != b.dtype or a.shape != b.shape or a.dtype not in (torch.float32, torch.uint8):
        raise RuntimeError("mobilequant_amd: gated_act_quant needs two float32 or two uint8 tensors of one shape")
    cols = a.shape[-1]
    rows = a.numel() // max(cols, 1)
    q = torch.empty(a.shape, dtype=torch.int8, device=a.device)
    rs = torch.empty(rows, dtype=torch.int32, device=a.device)
    y = torch.empty(a.shape, dtype=torch.float32, device=a.device) if want_y else None
    ptrs, keep = [], []
    for g, with_limits in ((a_grid, False), (b_grid, False), (mid_grid, True), (act_grid, True), (out_grid, True)):
        if g is None:
            ptrs += [None, None] + ([0.0, 0.0] if with_limits else [])
        else:
            s, o = _f32(g[0], "scale"), _f32(g[1], "offset")
            if s.numel() != 1 or o.numel() != 1:
                raise RuntimeError(f"mobilequant_amd: the gated activation takes per-tensor grids: scale and offset of one element (got {s.numel()}, {o.numel()})")
            keep += [s, o]
            ptrs += [s.data_ptr(), o.data_ptr()] + ([float(g[2]), float(g[3])] if with_limits else [])
    with _on(a, b, *keep):
        _lib.call("mq_gated_act_quant", a.data_ptr(), b.data_ptr(), MQ_U8 if a.dtype == torch.uint8 else MQ_F32, rows, cols,
                  {"silu": 0, "gelu": 1}[act], *ptrs, int(q_shift), q.data_ptr(), rs.data_ptr(),
                  y.data_ptr() if y is not None else None, _stream())
    return (q, rs, y) if want_y else (q, rs)


def gated_table(act: str, out_grid, a_grid, b_grid, mid_grid=None, act_grid=None, q_shift: int = 128) -> torch.Tensor:
    """The 256 x 256 table of gated_act_quant on index inputs (mq_gated_table): int8 [65536], entry [ia * 256 + ib]."""
    dev = out_grid[0].device
    table = torch.empty(65536, dtype=torch.int8, device=dev)
    ptrs, keep = [], []
    for g, with_limits in ((a_grid, False), (b_grid, False), (mid_grid, True), (act_grid, True), (out_grid, True)):
        if g is None:
            ptrs += [None, None] + ([0.0, 0.0] if with_limits else [])
        else:
            s, o = _f32(g[0], "scale"), _f32(g[1], "offset")
            if s.numel() != 1 or o.numel() != 1:
                raise RuntimeError(f"mobilequant_amd: the gated activation takes per-tensor grids: scale and offset of one element (got {s.numel()}, {o.numel()})")
            keep += [s, o]
            ptrs += [s.data_ptr(), o.data_ptr()] + ([float(g[2]), float(g[3])] if with_limits else [])
    with _on(table, *keep):
        _lib.call("mq_gated_table", {"silu": 0, "gelu": 1}[act], *ptrs, int(q_shift), table.data_ptr(), _stream())
    return table


def gated_lookup(a: torch.Tensor, b: torch.Tensor, table: torch.Tensor, tiled: bool = False):
    """uint8 index tensors a, b [rows, cols] -> (int8 image, row sums) through a gated_table (mq_gated_lookup).  tiled: the image
    in the fragment-blocked layout of quantize_tiled ([ceil16(rows), cols], cols % 64 == 0)."""
    a, b = _al16(_dev(a, "a").contiguous()), _al16(_dev(b, "b").contiguous())
    _dev(table, "table")
    if (a.dtype != torch.uint8 or b.dtype != torch.uint8 or a.shape != b.shape or table.dtype != torch.int8 or table.numel() != 65536
            or not table.is_contiguous()):
        raise RuntimeError("mobilequant_amd: gated_lookup needs two uint8 tensors of one shape and an int8 [65536] table")
    cols = a.shape[-1]
    rows = a.numel() // max(cols, 1)
    q = torch.empty(((rows + 15) // 16 * 16, cols) if tiled else a.shape, dtype=torch.int8, device=a.device)
    rs = torch.empty(rows, dtype=torch.int32, device=a.device)
    with _on(a, b, table):
        _lib.call("mq_gated_lookup_tiled" if tiled else "mq_gated_lookup", a.data_ptr(), b.data_ptr(), rows, cols, table.data_ptr(), q.data_ptr(), rs.data_ptr(), _stream())
    return q, rs


def qmatmul(x1: torch.Tensor, x2: torch.Tensor, grid1, grid2, grid_out=None) -> torch.Tensor:
    """QMatMul.forward (qmodule.py:453-466) in one launch (include/mobilequant_amd.h: mq_qmatmul): x1 [..., M, K] @ x2 [..., K, N] with
    both input quantizers and the output quantizer fused around an exact int8 contraction.  Grids are (scale, offset, qmin, qmax) with
    1-element device tensors (static per-tensor), grid_out may be None.  x2 is read in place when it is a dense [..., K, N] tensor with
    N % 4 == 0 or a transposed view of a dense [..., N, K] one (hf_model.py:513 passes k.transpose(2, 3)); anything else is copied
    K-contiguous first.
    Leading dims must match (no broadcasting).  Returns fp32 [..., M, N]."""
    _dev(x1, "x1"), _dev(x2, "x2")
    if x1.dtype != torch.float32 or x2.dtype != torch.float32:
        raise RuntimeError("mobilequant_amd: qmatmul takes float32 operands")
    if x1.dim() < 2 or x2.dim() != x1.dim() or x1.shape[:-2] != x2.shape[:-2] or x1.shape[-1] != x2.shape[-2]:
        raise RuntimeError(f"mobilequant_amd: qmatmul shapes {tuple(x1.shape)} @ {tuple(x2.shape)} (equal leading dims, no broadcasting)")
    lead = tuple(x1.shape[:-2])
    M, K, N = x1.shape[-2], x1.shape[-1], x2.shape[-1]
    batch = 1
    for d in lead:
        batch *= d
    a = x1 if x1.is_contiguous() else x1.contiguous()
    if x2.is_contiguous() and N % 4 == 0 and x2.data_ptr() % 16 == 0:
        b, kc = x2, 0
    else:                       # a transposed view of a dense [..., N, K] tensor is read in place; anything else is copied into that order
        t = x2.transpose(-1, -2)
        b, kc = (t if t.is_contiguous() else t.contiguous()), 1
    out = torch.empty(lead + (M, N), dtype=torch.float32, device=x1.device)
    keep = [a, b]

    def struct(g):
        if g is None:
            return None
        sc, of = _f32(g[0], "grid scale").reshape(-1), _f32(g[1], "grid offset").reshape(-1)
        if sc.numel() != 1 or of.numel() != 1:
            raise RuntimeError("mobilequant_amd: qmatmul takes per-tensor grids")
        keep.extend((sc, of))
        return _lib.MqGrid(sc.data_ptr(), of.data_ptr(), float(g[2]), float(g[3]))
    g1, g2, go = struct(grid1), struct(grid2), struct(grid_out)
    with _on(a, b, *keep):
        _lib.call("mq_qmatmul", a.data_ptr(), b.data_ptr(), out.data_ptr(), batch, M, N, K, kc, ctypes.byref(g1), ctypes.byref(g2),
                  ctypes.byref(go) if go is not None else None, _stream())
    return out


def qmatmul_supported(x1: torch.Tensor, x2: torch.Tensor) -> bool:
    """Shapes mq_qmatmul serves (the grids are the caller's to check): fp32 device tensors with equal leading dims (no broadcasting);
    any M / N / K."""
    if not (x1.is_cuda and x2.is_cuda and x1.dtype == torch.float32 and x2.dtype == torch.float32):
        return False
    if x1.dim() < 2 or x2.dim() != x1.dim() or x1.shape[:-2] != x2.shape[:-2] or x1.shape[-1] != x2.shape[-2] or x1.numel() == 0 or x2.numel() == 0:
        return False
    return x1.shape[-1] <= 131071            # the int32 MFMA accumulators hold K x 128 x 128


def attention_image_cache(kv_heads: int, head_dim: int, max_len: int, device) -> dict:
    """Caller-owned K / vT image caches for attention_quant(cache=..., pos0=...): one per attention block and sequence."""
    rows = (int(max_len) + 63) // 64 * 64
    dev = torch.device(device)
    return {"rows": rows, "kv_heads": int(kv_heads), "head_dim": int(head_dim),
            "k_i8": torch.zeros(kv_heads * rows * head_dim, dtype=torch.int8, device=dev),
            "vt_i8": torch.zeros(kv_heads * rows * head_dim, dtype=torch.int8, device=dev),
            "k_rs": torch.zeros(kv_heads * rows, dtype=torch.int32, device=dev),
            "k_f16": torch.zeros(kv_heads * rows * head_dim, dtype=torch.float16, device=dev) if head_dim == 64 else None,
            "v_pre": torch.zeros(kv_heads * (rows // 64) * head_dim, dtype=torch.int32, device=dev) if head_dim != 64 else None}


def _image_cache(cache: dict, who: str) -> None:
    """The tensors of an attention_image_cache dict, every one of which goes to the entry by pointer: dtype, contiguity and the element
    count its kv_heads / head_dim / rows give."""
    KV, D, rows = int(cache["kv_heads"]), int(cache["head_dim"]), int(cache["rows"])
    for name, dt, n in (("k_i8", torch.int8, KV * rows * D), ("vt_i8", torch.int8, KV * rows * D), ("k_rs", torch.int32, KV * rows),
                        ("k_f16", torch.float16, KV * rows * D), ("v_pre", torch.int32, KV * (rows // 64) * D)):
        if cache.get(name) is not None:
            _raw(cache[name], f"{who} cache['{name}']", dt, n)
    if cache.get("v_pre") is None and D != 64:
        raise RuntimeError(f"mobilequant_amd: {who} cache['v_pre'] is missing (head_dim {D} keeps a value prefix)")


def _grid1(g, who: str):
    """(scale, offset) of a per-tensor grid tuple as contiguous float32, one element each."""
    s, o = _f32(g[0], "scale"), _f32(g[1], "offset")
    if s.numel() != 1 or o.numel() != 1:
        raise RuntimeError(f"mobilequant_amd: {who} takes per-tensor grids: scale and offset of one element (got {s.numel()}, {o.numel()})")
    return s, o


F16_OFFSETS = (-256.0, 511.0)     # q / k offsets the f16 score contraction holds exactly: |index - offset| <= 511 (mq_attention.hip)


def attention_f16_offsets_ok(*offsets: float) -> bool:
    """True when the f16 score contraction of attention_quant is exact for q / k grids with these offsets."""
    return all(F16_OFFSETS[0] <= float(o) <= F16_OFFSETS[1] for o in offsets)


def attention_quant(q: Optional[torch.Tensor], k: Optional[torch.Tensor], v: Optional[torch.Tensor], cos: torch.Tensor, sin: torch.Tensor,
                    heads: int, kv_heads: int, grids: dict, image=None, want_out: bool = True, qkv_idx=None, head_dim: int = 64,
                    cache=None, pos0: int = 0, f16: Optional[bool] = None):
    """Quantized causal prefill attention of ONE sequence (mq_attention_quant; head_dim 64 or 256 -- "64" below reads head_dim): q [S, heads*64], k / v [S, kv_heads*64] fp32
    projection outputs before RoPE, cos / sin [S, 64]; grids: qk_a, qk_b, qk_out, pv_a, pv_b, pv_out -> (scale, offset, qmin, qmax)
    per tensor or None (qk_out / pv_out only).  Returns pv_bmm's output [S, heads*64] fp32 (o_proj's input layout).
    image = (q_i8, row_sum [rows] int32, row0, shift, tiled): additionally (want_out=False: only) write the pv_out indices of this
    sequence as rows row0 .. row0+S-1 of the consumer linear's int8 input image: row-major [rows, heads*64], or (tiled) the
    fragment-blocked [ceil16(rows), heads*64] layout of quantize_tiled.
    Batch: q / k / v [B, S, ...] (or qkv_idx [B, S, ...]) run as ONE launch pair (mq_attention_args.batch; not with a cache); the
    result is [B, S, heads*64] and sequence b owns rows row0 + b * S of the image.
    cache = attention_image_cache(...) + pos0: cache continuation (chunked prefill).  The cache already holds positions 0 .. pos0 - 1
    from earlier calls (same grids); q / k / v / cos / sin describe positions pos0 .. pos0 + S - 1, which are appended and attend to
    everything before them.  pos0 % 64 == 0 (every chunk but the last is a multiple of 64 long).
    f16: head_dim 64 with a score grid contracts q.k^T over fp16 images of the centred indices, exact only while both q / k offsets
    lie in F16_OFFSETS (the prep kernel poisons the images with NaN otherwise).  True / False choose; None reads the offsets on the
    host (int8 contraction while a graph is being captured: no device read there).  The int8 contraction is exact for any grid."""
    cos, sin = _f32(cos, "cos", True), _f32(sin, "sin", True)
    D = int(head_dim)
    if D not in (64, 128, 256):
        raise RuntimeError("mobilequant_amd: attention_quant serves head_dim 64, 128 and 256")
    rot = cos.shape[-1]                  # partial rotary: cos / sin [S, rot_dim] with rot_dim < 64 (hf_model.py:489-500)
    if rot > D or rot % 2 or sin.shape != cos.shape:
        raise RuntimeError("mobilequant_amd: attention_quant cos / sin must be [S, rot_dim], rot_dim even and <= 64")
    idx = None
    if qkv_idx is not None:       # (uint8 [S, (heads + 2 kv_heads) * 64] of int8_linear_segmented, ((scale, offset) x 3))
        idx, in_grids = qkv_idx
        idx = _al16(_dev(idx, "qkv_idx").contiguous())
        B = idx.shape[0] if idx.dim() == 3 else 0                    # 0: one sequence, 2-D tensors
        S = idx.shape[-2]
        if idx.dtype != torch.uint8 or idx.shape[-2:] != (S, (heads + 2 * kv_heads) * D) or idx.dim() not in (2, 3) or cos.shape != (S, rot):
            raise RuntimeError("mobilequant_amd: attention_quant qkv_idx must be uint8 [(B,) S, (H + 2 KV) * 64], cos / sin [S, 64]")
        q = k = v = None
    else:
        q, k, v = (_al16(_dev(t, n).contiguous()) for t, n in ((q, "q"), (k, "k"), (v, "v")))
        B = q.shape[0] if q.dim() == 3 else 0
        S = q.shape[-2]
        lead = (B,) if B else ()
        if (q.dtype != torch.float32 or k.dtype != torch.float32 or v.dtype != torch.float32 or q.shape != lead + (S, heads * D)
                or k.shape != lead + (S, kv_heads * D) or v.shape != k.shape or cos.shape != (S, rot)):
            raise RuntimeError("mobilequant_amd: attention_quant needs fp32 q [(B,) S, H*64], k / v [(B,) S, KV*64], cos / sin [S, 64]")
    if B and cache is not None:
        raise RuntimeError("mobilequant_amd: attention_quant serves a batch in one launch only without an image cache (one call per sequence there)")
    nb = max(B, 1)
    S_real = S
    if S % 64:                    # pad the sequence: under the causal mask a padded key is only ever seen by padded queries
        pad = 64 - S % 64
        cos, sin = (torch.nn.functional.pad(t, (0, 0, 0, pad)) for t in (cos, sin))
        if idx is not None:
            idx = torch.nn.functional.pad(idx, (0, 0, 0, pad))
        else:
            q, k, v = (torch.nn.functional.pad(t, (0, 0, 0, pad)) for t in (q, k, v))
        S += pad
    a = _lib.MqAttentionArgs()
    keep = []
    for name in ("qk_a", "qk_b", "qk_out", "pv_a", "pv_b", "pv_out"):
        g = grids.get(name)
        if g is None:
            setattr(a, name, _lib.MqGrid(None, None, 0.0, 0.0))
        else:
            s, o = _grid1(g, "attention_quant")
            keep += [s, o]
            setattr(a, name, _lib.MqGrid(s.data_ptr(), o.data_ptr(), float(g[2]), float(g[3])))
    first = idx if idx is not None else q
    dev = first.device
    if idx is not None:
        a.qkv_idx = idx.data_ptr()
        for name, g in zip(("q_in", "k_in", "v_in"), in_grids):
            sc, of = _grid1(g, "attention_quant")
            keep += [sc, of]
            setattr(a, name, _lib.MqGrid(sc.data_ptr(), of.data_ptr(), 0.0, 255.0))
    out = torch.empty(((B,) if B else ()) + (S, heads * D), dtype=torch.float32, device=dev) if want_out or image is None else None
    q_i8 = torch.empty(nb * heads * S * D, dtype=torch.int8, device=dev)
    q_rs = torch.empty(nb * heads * S, dtype=torch.int32, device=dev)
    a.batch = B
    if cache is not None:
        if (cache["kv_heads"], cache["head_dim"]) != (kv_heads, D) or cache["k_i8"].device != dev:
            raise RuntimeError("mobilequant_amd: attention_quant cache was built for another shape / device")
        _image_cache(cache, "attention_quant")
        if pos0 % 64 or pos0 < 0 or pos0 + S > cache["rows"]:
            raise RuntimeError(f"mobilequant_amd: attention_quant cache continuation needs pos0 % 64 == 0 and pos0 + padded S <= {cache['rows']} "
                               f"(pos0={pos0}, S={S})")
        k_i8, vt_i8, k_rs, v_pre = cache["k_i8"], cache["vt_i8"], cache["k_rs"], cache["v_pre"]
        k_f16 = cache.get("k_f16")
        a.pos0, a.cache_seq = int(pos0), int(cache["rows"])
    else:
        if pos0:
            raise RuntimeError("mobilequant_amd: attention_quant(pos0 > 0) needs a cache (attention_image_cache)")
        k_i8 = torch.empty(nb * kv_heads * S * D, dtype=torch.int8, device=dev)
        vt_i8 = torch.empty(nb * kv_heads * S * D, dtype=torch.int8, device=dev)
        k_rs = torch.empty(nb * kv_heads * S, dtype=torch.int32, device=dev)
        v_pre = torch.empty(nb * kv_heads * (S // 64) * D, dtype=torch.int32, device=dev) if D != 64 else None
        k_f16 = torch.empty(nb * kv_heads * S * D, dtype=torch.float16, device=dev) if D == 64 else None
    if k_f16 is not None and grids.get("qk_out") is not None and f16 is None:
        f16 = not torch.cuda.is_current_stream_capturing() and attention_f16_offsets_ok(
            *(float(grids[n][1].detach().reshape(-1)[0]) for n in ("qk_a", "qk_b")))
    if cache is not None:                # the f16 form reads the fp16 K image of the earlier chunks: only where every one wrote it
        if pos0 == 0:
            cache["k_f16_valid"] = True
        f16 = f16 and cache.get("k_f16_valid", False)
    if k_f16 is not None and grids.get("qk_out") is not None and f16:
        # head_dim 64 with a score grid: fp16 images of the centred q / k indices -> the f16 score contraction (mq_attention_args.q_f16)
        q_f16 = torch.empty(nb * heads * S * D, dtype=torch.float16, device=dev)
        keep += [q_f16, k_f16]
        a.q_f16, a.k_f16 = q_f16.data_ptr(), k_f16.data_ptr()
    elif cache is not None:
        cache["k_f16_valid"] = False
    if v_pre is not None:
        keep.append(v_pre)
        a.v_prefix = v_pre.data_ptr()
    if idx is None:
        a.q, a.k, a.v = q.data_ptr(), k.data_ptr(), v.data_ptr()
    a.cos, a.sin = cos.data_ptr(), sin.data_ptr()
    a.seq, a.heads, a.kv_heads, a.head_dim, a.inv_sqrt_d = S, heads, kv_heads, D, 1.0 / (D ** 0.5)
    a.rot_dim = rot
    a.out, a.q_i8, a.k_i8, a.vt_i8 = out.data_ptr() if out is not None else None, q_i8.data_ptr(), k_i8.data_ptr(), vt_i8.data_ptr()
    a.q_rowsum, a.k_rowsum = q_rs.data_ptr(), k_rs.data_ptr()
    a.seq_real = S_real
    if image is not None:
        q_t, rs_t, row0, shift, tiled = image
        _dev(q_t, "image"), _dev(rs_t, "image row sums")
        need = (row0 + nb * S_real + 15) // 16 * 16 if tiled else row0 + nb * S_real
        if (q_t.dtype != torch.int8 or rs_t.dtype != torch.int32 or not q_t.is_contiguous() or not rs_t.is_contiguous() or q_t.shape[-1] != heads * D
                or row0 < 0 or row0 + nb * S_real > rs_t.numel() or need > q_t.shape[0]):
            raise RuntimeError("mobilequant_amd: attention_quant image must be int8 [rows (tiled: ceil16), heads*64] + int32 row sums [rows]")
        keep += [q_t, rs_t]
        a.out_i8, a.out_rowsum, a.out_row0, a.out_shift, a.out_i8_tiled = q_t.data_ptr(), rs_t.data_ptr(), int(row0), int(shift), int(bool(tiled))
    with _on(first, k, v, cos, sin, *keep):
        _lib.call("mq_attention_quant", ctypes.byref(a), _stream())
    if out is None:
        return None
    return out if S_real == S else out[..., :S_real, :].contiguous()


def _cache_bridge_args(fn: str, cache: dict, k: torch.Tensor, v: torch.Tensor, p0: int, n: int, v_chunked: bool):
    """Host-side checks (before any device is touched) and the argument block shared by attention_cache_import / _export."""
    D, KV, rows = int(cache["head_dim"]), int(cache["kv_heads"]), int(cache["rows"])
    if D not in (64, 128, 256):
        raise RuntimeError(f"mobilequant_amd: {fn} serves head_dim 64, 128 and 256 (got {D})")
    p0, n = int(p0), int(n)
    if n <= 0 or p0 < 0 or p0 + n > rows:
        raise RuntimeError(f"mobilequant_amd: {fn} positions {p0} .. {p0 + n - 1} outside the image cache's {rows} rows")
    if not isinstance(k, torch.Tensor) or not isinstance(v, torch.Tensor) or k.dtype != torch.int8 or v.dtype != torch.int8:
        raise RuntimeError(f"mobilequant_amd: {fn} takes int8 decode caches")
    L = k.shape[1] if k.dim() == 3 else -1
    v_shape = (KV, L // 16, D, 16) if v_chunked else (KV, L, D)
    if (k.dim() != 3 or tuple(k.shape) != (KV, L, D) or tuple(v.shape) != v_shape or (v_chunked and L % 16) or p0 + n > L
            or k.stride()[1:] != (D, 1) or v.stride()[1:] != ((16 * D, 16, 1) if v_chunked else (D, 1))):
        raise RuntimeError(f"mobilequant_amd: {fn} shape mismatch: k must be [{KV}, cache_len, {D}], v the same or (v_chunked) "
                           f"[{KV}, cache_len / 16, {D}, 16], dense behind the head dimension, with at least {p0 + n} positions "
                           f"(got k {tuple(k.shape)}, v {tuple(v.shape)})")
    _dev(k, "k"), _dev(v, "v")
    if cache["k_i8"].device != k.device or v.device != k.device:
        raise RuntimeError(f"mobilequant_amd: {fn} image cache and decode caches live on different devices")
    _image_cache(cache, fn)
    a = _lib.MqAttentionCacheArgs()
    a.k, a.v, a.k_head_stride, a.v_head_stride, a.v_chunked = k.data_ptr(), v.data_ptr(), int(k.stride(0)), int(v.stride(0)), int(bool(v_chunked))
    a.kv_heads, a.head_dim, a.cache_len, a.p0, a.n, a.cache_seq = KV, D, L, p0, n, rows
    a.k_i8, a.vt_i8 = cache["k_i8"].data_ptr(), cache["vt_i8"].data_ptr()
    return a


def attention_cache_import(cache: dict, k: torch.Tensor, v: torch.Tensor, n: int, grids: dict, v_chunked: bool = False,
                           k_f16_exact: Optional[bool] = None) -> None:
    """Build the images of `cache` (attention_image_cache) for positions 0 .. n - 1 from a decode engine's caches
    (mq_attention_cache_import, one launch): k [kv_heads, cache_len, D] int8, v the same or -- v_chunked -- the four-launch chain's
    [kv_heads, cache_len / 16, D, 16]; a view with its own head stride (a slot of the batched engine's caches) is read in place.
    n % 64 == 0.  grids: qk_a and qk_b as (scale, offset, qmin, qmax) -- the kernel reads their OFFSETS by pointer at launch (the zero
    points of k_rowsum and k_f16).  Rows >= n of the images are left as they are.
    k_f16 (head_dim 64) holds fp16(index - zk) exactly only for zk inside F16_OFFSETS; outside, the kernel poisons it with NaN as the
    prefill's own preparation does, and cache["k_f16_valid"] is set False so that attention_quant keeps this cache on the int8 score
    contraction.  k_f16_exact: the caller's knowledge of that (llama._f16_scores_ok); None reads qk_b's offset on the host (False while
    a graph is being captured: no device read there)."""
    if int(n) % 64:
        raise RuntimeError(f"mobilequant_amd: attention_cache_import needs n % 64 == 0 (got n={n}): the attention continues an image cache at multiples of 64")
    a = _cache_bridge_args("attention_cache_import", cache, k, v, 0, n, v_chunked)
    keep = []
    for name in ("qk_a", "qk_b"):
        g = grids[name]
        s, o = _grid1(g, "attention_cache_import")
        keep += [s, o]
        setattr(a, name, _lib.MqGrid(s.data_ptr(), o.data_ptr(), float(g[2]), float(g[3])))
    a.k_rowsum = cache["k_rs"].data_ptr()
    if cache.get("v_pre") is not None:
        a.v_prefix = cache["v_pre"].data_ptr()
    if cache.get("k_f16") is not None:
        a.k_f16 = cache["k_f16"].data_ptr()
        if k_f16_exact is None:
            k_f16_exact = not torch.cuda.is_current_stream_capturing() and attention_f16_offsets_ok(float(grids["qk_b"][1].detach().reshape(-1)[0]))
    with _on(k, v, *keep):
        _lib.call("mq_attention_cache_import", ctypes.byref(a), _stream())
    cache["k_f16_valid"] = bool(k_f16_exact) and cache.get("k_f16") is not None


def attention_cache_export(cache: dict, k: torch.Tensor, v: torch.Tensor, p0: int, n: int, v_chunked: bool = False) -> None:
    """The inverse for rows p0 .. p0 + n - 1 of the images (mq_attention_cache_export, one launch): the keys are copied, the values
    un-permuted into either decode layout.  n is any positive count -- the REAL rows of a ragged final chunk, not its pad rows.  No
    byte outside those positions is written (the other positions of a shared 16-position chunk keep their values)."""
    a = _cache_bridge_args("attention_cache_export", cache, k, v, p0, n, v_chunked)
    with _on(k, v):
        _lib.call("mq_attention_cache_export", ctypes.byref(a), _stream())


# ---- token scoring: the fp32 lm_head fused with its log-softmax ------------------------------------------------------------------
def score_head(y: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], targets: Optional[torch.Tensor]):
    """Per row of y [M, K] (fp32, unit column stride): (logprob [M] fp32, lse [M] fp32, argmax [M] int64) of the logits
    y @ weight.T (+ bias) without writing them (mq_score_head).  weight [V, K] fp32 is nn.Linear's layout.  targets [M] int64: a
    row's target index, < 0 = ignored (logprob 0); every target must be < V (checked here, on the host)."""
    _dev(y, "score_head y")
    if y.dim() != 2 or y.dtype != torch.float32:
        raise RuntimeError("mobilequant_amd: score_head y must be fp32 [M, K]")
    M, K = y.shape
    if y.stride(1) != 1 or y.stride(0) % 4:
        y = y.contiguous()
    if y.data_ptr() % 16:                # (.contiguous() hands a dense view off a 16-byte boundary back as it is)
        y = y.contiguous().clone()
    w = _f32(weight, "score_head weight", True)
    V = w.shape[0]
    if w.dim() != 2 or w.shape[1] != K:
        raise RuntimeError(f"mobilequant_amd: score_head weight must be [V, {K}], got {tuple(w.shape)}")
    if K % 4:
        raise RuntimeError(f"mobilequant_amd: score_head needs K % 4 == 0 (K = {K})")
    b = None
    if bias is not None:
        b = _f32(bias, "score_head bias")
        if b.shape != (V,):
            raise RuntimeError(f"mobilequant_amd: score_head bias must be [{V}]")
    t = None
    if targets is not None:
        _dev(targets, "score_head targets")
        if targets.shape != (M,) or targets.dtype.is_floating_point or targets.dtype == torch.bool:
            raise RuntimeError(f"mobilequant_amd: score_head targets must be [{M}] integers (got {tuple(targets.shape)}, {targets.dtype})")
        t = targets.to(torch.int64).contiguous()
        if M and int(t.max()) >= V:
            raise RuntimeError(f"mobilequant_amd: score_head target {int(t.max())} outside the vocabulary [0, {V})")
    dev = y.device
    logprob = torch.empty(M, dtype=torch.float32, device=dev)
    lse = torch.empty(M, dtype=torch.float32, device=dev)
    amax = torch.empty(M, dtype=torch.int64, device=dev)
    if M == 0:
        return logprob, lse, amax
    lib = _lib.load()
    nbytes = int(lib.mq_score_head_scratch_bytes(M, V))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)          # the caching allocator hands out 512-byte aligned blocks
    with _on(y, w, b, t):
        _lib.call("mq_score_head", y.data_ptr(), y.stride(0), w.data_ptr(), b.data_ptr() if b is not None else None,
                  t.data_ptr() if t is not None else None, M, K, V, scratch.data_ptr(), nbytes, logprob.data_ptr(), lse.data_ptr(),
                  amax.data_ptr(), _stream())
    return logprob, lse, amax


# ---- seeded token selection on the device (mq_sample): the binding lives with SamplingParams -------------------------
from .sampling import history_count as sample_history_count, history_count_ragged as sample_history_count_ragged  # noqa: E402,F401
from .sampling import history_prompt as sample_history_prompt, sample, sample_ragged, sample_rows, sample_uniforms  # noqa: E402,F401
from .sampling import logprob_top  # noqa: E402,F401
