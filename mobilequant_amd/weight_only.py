"""W4A16: weight-only 4-bit linears on mq_w4a16_linear (csrc/mq_w4a16.hip; the contract: DESIGN.md 4.9).

The reference packs into auto_gptq's QuantLinear for this mode (qmodule.py:803-829); here the packed form is the mq_pack_w4 image the W4A8
kernels read, with fp16 scales and zeros per (row, group):

    w16[n, k] = fp16(float(scales[n, G]) * float(u[n, k] - zeros[n, G]))      u = index - qmin (0..15), zeros = offset - qmin, G = k // g
    y[m, n]   = x.dtype(sum_k fp16(x[m, k]) * w16[n, k] + bias[n])            fp32 accumulation, one final rounding

`w4a16_pack` and `w4a16_linear` run on the device and raise otherwise; `w4a16_dequantize` is plain torch (tests, `to_float`).
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch

from . import _lib, ops
from ._lib import MQ_U8

BITS = 4
MAX_ZERO = 1024          # |offset - qmin| up to here: u - zero stays exact in fp16
RULE = "N % 16 == 0, K % 64 == 0, group_size a multiple of 32 that divides K"


def w4a16_variant(M: int, N: int, K: int, group_size: int) -> int:
    """mq_w4a16_supported: 0 when mq_w4a16_linear does not serve the shape, 1 when it takes the weight-streaming GEMV (M <= 8 and
    M * K <= 65536), 2 for the MFMA GEMM.  group_size -1 means K."""
    return int(_lib.load().mq_w4a16_supported(int(M), int(N), int(K), int(K if group_size == -1 else group_size)))


def w4a16_supported(N: int, K: int, group_size: int) -> bool:
    """True when every M >= 1 is served for weights [N, K] with this group size (the rule does not depend on M)."""
    return w4a16_variant(1, N, K, group_size) != 0


def _groups(K: int, group_size: int) -> Tuple[int, int]:
    g = K if group_size == -1 else int(group_size)
    if g <= 0 or K % g:
        raise ValueError(f"mobilequant_amd: w4a16 group_size {group_size} does not divide K = {K}")
    return g, K // g


def w4a16_pack(w: torch.Tensor, scale: torch.Tensor, offset: torch.Tensor, bitwidth: int = BITS, is_symmetric: bool = False,
               group_size: int = -1):
    """Weight [N, K] and its per-(row, group) grid -> (qweight uint8 [N, K / 2], scales fp16 [N, G], zeros fp16 [N, G]).
    The index is Quantizer.forward's, clamp(rint(w / s) + z, qmin, qmax) in fp32 (mq_quantize), stored as u = index - qmin and packed by
    mq_pack_w4; scales = fp16(s) to nearest even; zeros = z - qmin, which must be an integer with |zero| <= 1024 (ValueError otherwise:
    one host read per packed weight)."""
    if int(bitwidth) != BITS:
        raise ValueError(f"mobilequant_amd: w4a16_pack packs 4-bit grids only (got bitwidth {bitwidth})")
    ops._dev(w, "w4a16_pack weight")
    if w.dim() != 2:
        raise ValueError(f"mobilequant_amd: w4a16_pack weight must be [N, K] (got {tuple(w.shape)})")
    N, K = w.shape
    g, G = _groups(K, group_size)
    if not w4a16_supported(N, K, g):
        raise ValueError(f"mobilequant_amd: w4a16 does not serve N={N}, K={K}, group_size={g} ({RULE})")
    qmin = -(2 ** (BITS - 1)) if is_symmetric else 0
    qmax = qmin + 2 ** BITS - 1
    s = scale.detach().to(device=w.device, dtype=torch.float32).reshape(-1).contiguous()
    o = offset.detach().to(device=w.device, dtype=torch.float32).reshape(-1).contiguous()
    if s.numel() != N * G or o.numel() != N * G:
        raise ValueError(f"mobilequant_amd: w4a16_pack needs one (scale, offset) per row and group, {N} x {G} (got {s.numel()}, {o.numel()})")
    w32 = w.detach().to(torch.float32).reshape(N * G, g)
    nib = ops.quantize(w32, s, o, qmin, qmax, q_dtype=MQ_U8, shift=qmin, rows=N * G)
    qweight = ops.pack_w4(nib.view(N, K))
    zero = o - float(qmin)
    bad = (zero != zero.round()) | (zero.abs() > MAX_ZERO) | ~torch.isfinite(zero)
    s16 = s.to(torch.float16)
    if bool(bad.any()):
        raise ValueError(f"mobilequant_amd: w4a16 zero point (offset - qmin) must be an integer within +-{MAX_ZERO} (got {float(zero[bad][0])})")
    if not bool(torch.isfinite(s16).all()):
        raise ValueError("mobilequant_amd: w4a16 scale does not fit fp16")
    return qweight, s16.view(N, G), zero.to(torch.float16).view(N, G)


def w4a16_dequantize(qweight: torch.Tensor, scales: torch.Tensor, zeros: torch.Tensor, group_size: int = -1) -> torch.Tensor:
    """w16 [N, K] fp16 of a packed weight, in torch on the tensors' device (CPU included): fp16(float(s16) * float(u - zero)); the fp32
    product of an 11-bit significand and an integer below 2^11 is exact, so the conversion is the one rounding of the contract."""
    N, half = qweight.shape
    K = half * 2
    g, G = _groups(K, group_size)
    p = qweight.reshape(N, K // 32, 16)
    u = torch.stack((p & 15, p >> 4), dim=2).reshape(N, K).to(torch.float32)
    z = zeros.to(torch.float32).reshape(N, G, 1)
    s = scales.to(torch.float32).reshape(N, G, 1)
    return (s * (u.view(N, G, g) - z)).reshape(N, K).to(torch.float16)


def w4a16_linear(x: torch.Tensor, qweight: torch.Tensor, scales: torch.Tensor, zeros: torch.Tensor, bias: Optional[torch.Tensor] = None,
                 group_size: int = -1) -> torch.Tensor:
    """x [..., K] fp32 or fp16 (any layout: made contiguous) -> [..., N] of x's dtype, on x's device and the current stream.
    qweight / scales / zeros as w4a16_pack returns them (passed as they are: contiguous uint8 / fp16 device tensors); bias: any floating
    dtype, read as float32."""
    ops._dev(x, "w4a16_linear x")
    dt = ops._fdt(x, "w4a16_linear x")
    if qweight.dim() != 2:
        raise RuntimeError(f"mobilequant_amd: w4a16_linear qweight must be [N, K / 2] (got {tuple(qweight.shape)})")
    N, K = qweight.shape[0], qweight.shape[1] * 2
    g, G = _groups(K, group_size)
    if x.dim() < 1 or x.shape[-1] != K:
        raise RuntimeError(f"mobilequant_amd: w4a16_linear x has {x.shape[-1] if x.dim() else 0} input features, the weight {K}")
    ops._raw(qweight, "w4a16_linear qweight", torch.uint8, N * K // 2)
    ops._raw(scales, "w4a16_linear scales", torch.float16, N * G)
    ops._raw(zeros, "w4a16_linear zeros", torch.float16, N * G)
    lead = x.shape[:-1]
    x2d = ops._al16(x.reshape(-1, K).contiguous())
    M = x2d.shape[0]
    b = None
    if bias is not None:
        b = ops._f32(bias, "w4a16_linear bias", align16=True)          # (a converted copy lives until the launch is queued)
        if b.numel() != N:
            raise RuntimeError(f"mobilequant_amd: w4a16_linear bias holds {b.numel()} elements, the weight has {N} rows")
    out = torch.empty((M, N), dtype=x.dtype, device=x.device)
    if M == 0:
        return out.reshape(*lead, N)
    a = _lib.MqW4A16Args()
    a.x, a.x_dtype = x2d.data_ptr(), dt
    a.M, a.N, a.K, a.group_size = M, N, K, g
    a.w_packed, a.scales, a.zeros = qweight.data_ptr(), scales.data_ptr(), zeros.data_ptr()
    a.bias = b.data_ptr() if b is not None else None
    a.out, a.out_dtype = out.data_ptr(), dt
    with ops._on(x2d, qweight, scales, zeros, b, out):
        _lib.call("mq_w4a16_linear", ctypes.byref(a), ops._stream())
    del b, x2d
    return out.reshape(*lead, N)


# ---- the decode step's two launches (csrc/mq_w4a16_decode.hip) -------------------------------------------------------
# Thin wrappers: every pointer goes to its entry as it is (ops._raw: device, dtype, contiguity and element count are checked here, the
# 16-byte alignment by the entry), nothing is converted or copied, so both are capturable and write only `out` (and the cache row).
_PROLOGUES = {"plain": _lib.MQ_W4A16_PRO_PLAIN, "rmsnorm": _lib.MQ_W4A16_PRO_RMSNORM, "layernorm": _lib.MQ_W4A16_PRO_LAYERNORM}
_EPILOGUES = {"bias": _lib.MQ_W4A16_EPI_BIAS, "resid": _lib.MQ_W4A16_EPI_RESID, "gated": _lib.MQ_W4A16_EPI_GATED}
_ACTS = {"silu": 0, "gelu": 1}
DECODE_RULE = RULE + ", K <= 32768 (gated: N % 32 == 0)"


def w4a16_decode_supported(N: int, K: int, group_size: int, epilogue: str = "bias") -> bool:
    """mq_w4a16_decode_supported: whether mq_w4a16_decode_gemv serves a packed image of N rows (gated: both linears' rows) of length K."""
    return bool(_lib.load().mq_w4a16_decode_supported(int(N), int(K), int(K if group_size == -1 else group_size), _EPILOGUES[epilogue]))


def w4a16_decode_gemv_args(x: torch.Tensor, qweight: torch.Tensor, scales: torch.Tensor, zeros: torch.Tensor, out: torch.Tensor, *,
                           group_size: int = -1, prologue: str = "plain", norm_weight: Optional[torch.Tensor] = None,
                           norm_bias: Optional[torch.Tensor] = None, eps: float = 0.0, epilogue: str = "bias",
                           bias: Optional[torch.Tensor] = None, resid: Optional[torch.Tensor] = None,
                           act: str = "silu") -> "_lib.MqW4A16DecodeGemvArgs":
    """The checked argument block of w4a16_decode_gemv (an engine fills it once and keeps the tensors alive)."""
    who = "w4a16_decode_gemv"
    if prologue not in _PROLOGUES or epilogue not in _EPILOGUES or act not in _ACTS:
        raise ValueError(f"mobilequant_amd: {who} prologue {prologue!r} / epilogue {epilogue!r} / act {act!r}: one of {sorted(_PROLOGUES)}, "
                         f"{sorted(_EPILOGUES)}, {sorted(_ACTS)}")
    ops._dev(qweight, f"{who} qweight")
    if qweight.dim() != 2:
        raise RuntimeError(f"mobilequant_amd: {who} qweight must be [N, K / 2] (got {tuple(qweight.shape)})")
    N, K = qweight.shape[0], qweight.shape[1] * 2
    g, G = _groups(K, group_size)
    ops._raw(x, f"{who} x", torch.float32, K)
    ops._raw(qweight, f"{who} qweight", torch.uint8, N * K // 2)
    ops._raw(scales, f"{who} scales", torch.float16, N * G)
    ops._raw(zeros, f"{who} zeros", torch.float16, N * G)
    ops._raw(out, f"{who} out", torch.float32, N // 2 if epilogue == "gated" else N)
    for t, what, n in ((norm_weight, "norm_weight", K), (norm_bias, "norm_bias", K), (bias, "bias", N), (resid, "resid", N)):
        if t is not None:
            ops._raw(t, f"{who} {what}", torch.float32, n)
    a = _lib.MqW4A16DecodeGemvArgs()
    a.x, a.N, a.K, a.group_size = x.data_ptr(), N, K, g
    a.w_packed, a.scales, a.zeros = qweight.data_ptr(), scales.data_ptr(), zeros.data_ptr()
    a.prologue, a.eps, a.epilogue, a.act = _PROLOGUES[prologue], float(eps), _EPILOGUES[epilogue], _ACTS[act]
    a.norm_weight = norm_weight.data_ptr() if norm_weight is not None else None
    a.norm_bias = norm_bias.data_ptr() if norm_bias is not None else None
    a.bias = bias.data_ptr() if bias is not None else None
    a.resid = resid.data_ptr() if resid is not None else None
    a.out = out.data_ptr()
    return a


def w4a16_decode_gemv(x: torch.Tensor, qweight: torch.Tensor, scales: torch.Tensor, zeros: torch.Tensor, out: torch.Tensor, **kw) -> torch.Tensor:
    """mq_w4a16_decode_gemv: one fp32 row x [K] through a packed weight (w4a16_pack's tensors) into out (fp32 [N]; gated: [N / 2]), on
    the current stream.  prologue "plain" | "rmsnorm" | "layernorm" (norm_weight / norm_bias fp32 [K], eps); epilogue "bias" (bias fp32
    [N] or None) | "resid" (out = resid + (y + bias)) | "gated" (rows of the gate and the up linear interleaved; act "silu" | "gelu").
    Every tensor is passed as it is: contiguous device tensors of exactly these dtypes and sizes, 16-byte aligned."""
    a = w4a16_decode_gemv_args(x, qweight, scales, zeros, out, **kw)
    with ops._on(x, qweight, scales, zeros, out, kw.get("norm_weight"), kw.get("norm_bias"), kw.get("bias"), kw.get("resid")):
        _lib.call("mq_w4a16_decode_gemv", ctypes.byref(a), ops._stream())
    return out


def w4a16_decode_attention_args(qkv: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, rope_row: torch.Tensor, pos: torch.Tensor,
                                out: torch.Tensor, *, heads: int, kv_heads: int, head_dim: int, rot_dim: int, nsplit: int = 1,
                                part: Optional[torch.Tensor] = None,
                                ticket: Optional[torch.Tensor] = None) -> "_lib.MqW4A16DecodeAttentionArgs":
    """The checked argument block of w4a16_decode_attention."""
    who = "w4a16_decode_attention"
    H, KV, D, rot, ns = int(heads), int(kv_heads), int(head_dim), int(rot_dim), int(nsplit)
    if min(H, KV, D, rot, ns) < 1:
        raise ValueError(f"mobilequant_amd: {who} heads / kv_heads / head_dim / rot_dim / nsplit must be positive")
    ops._raw(qkv, f"{who} qkv", torch.float32, (H + 2 * KV) * D)
    ops._raw(k_cache, f"{who} k_cache", torch.float32)
    if k_cache.numel() == 0 or k_cache.numel() % (KV * D):
        raise RuntimeError(f"mobilequant_amd: {who} k_cache must hold [kv_heads = {KV}, cache_len, head_dim = {D}] (got {tuple(k_cache.shape)})")
    T = k_cache.numel() // (KV * D)
    ops._raw(v_cache, f"{who} v_cache", torch.float32, KV * T * D)
    ops._raw(rope_row, f"{who} rope_row", torch.float32, 2 * rot)
    ops._raw(pos, f"{who} pos", torch.int32, 1)
    ops._raw(out, f"{who} out", torch.float32, H * D)
    if ns > 1:
        if part is None or ticket is None:
            raise RuntimeError(f"mobilequant_amd: {who} nsplit = {ns} needs part (fp32 [heads, nsplit, head_dim + 4]) and ticket (int32 [heads], zeroed)")
        ops._raw(part, f"{who} part", torch.float32, H * ns * (D + 4))
        ops._raw(ticket, f"{who} ticket", torch.int32, H)
    a = _lib.MqW4A16DecodeAttentionArgs()
    a.qkv, a.k_cache, a.v_cache, a.rope_row, a.pos = qkv.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), rope_row.data_ptr(), pos.data_ptr()
    a.heads, a.kv_heads, a.head_dim, a.cache_len, a.rot_dim, a.nsplit = H, KV, D, T, rot, ns
    a.part = part.data_ptr() if ns > 1 else None
    a.ticket = ticket.data_ptr() if ns > 1 else None
    a.out = out.data_ptr()
    return a


def w4a16_decode_attention(qkv: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, rope_row: torch.Tensor, pos: torch.Tensor,
                           out: torch.Tensor, **kw) -> torch.Tensor:
    """mq_w4a16_decode_attention: RoPE on q and the new k, the append of (k, v) at position pos[0] of the fp32 caches [kv_heads, cache_len,
    head_dim] (one sequence of LlamaForCausalLM.new_cache) and the attention of the new token over positions 0 .. pos[0], into out
    (fp32 [heads * head_dim]).  qkv fp32 [(heads + 2 kv_heads) * head_dim]; rope_row fp32 [2 rot_dim] = cos | sin of this position; pos
    int32 [1] on the device.  nsplit > 1: part fp32 [heads, nsplit, head_dim + 4] and ticket int32 [heads] (zero).  A position outside
    the cache does nothing.  Every tensor is passed as it is."""
    a = w4a16_decode_attention_args(qkv, k_cache, v_cache, rope_row, pos, out, **kw)
    with ops._on(qkv, k_cache, v_cache, rope_row, pos, out, kw.get("part"), kw.get("ticket")):
        _lib.call("mq_w4a16_decode_attention", ctypes.byref(a), ops._stream())
    return out
