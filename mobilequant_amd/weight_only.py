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
