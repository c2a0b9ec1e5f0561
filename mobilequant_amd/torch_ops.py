"""``torch.ops.mobilequant_amd.*``: the C ABI's core entry points registered with ``torch.library`` ("Native
boundary").

The product path calls the C ABI through ``ops.py`` (ctypes; no dispatcher hop on the decode step's launch path).  This module
puts the same kernels behind PyTorch's operator registry so that a caller can reach them as ``torch.ops.mobilequant_amd.<op>``,
trace / export graphs that contain them (every op has a FakeTensor / meta kernel: shapes and dtypes without a device), and see
them in profiler traces under their own names.  Device implementations are registered for "cuda" (= ROCm) ONLY: a CPU tensor
has no kernel to dispatch to and raises ``NotImplementedError`` from the dispatcher -- there is no CPU path here either.

    import mobilequant_amd.torch_ops            # registers the operators
    y = torch.ops.mobilequant_amd.fake_quant(x, scale, offset, 0.0, 255.0)

Operators (reference code each one replaces):
    fake_quant(x, scale, offset, qmin, qmax) -> Tensor                              Quantizer.forward, qmodule.py:286-295
    quantize(x, scale, offset, qmin, qmax, shift, chan_scale?) -> (int8, int32)      the index half of it (+ row sums), n1
    minmax(x, per_channel) -> Tensor[2] | Tensor[2, C]                              compute_min_max_from_tensor, qmodule.py:26-34
    minmax_update_(running[2, n], x) -> ()                                         update_act_range, generate_act_range.py:49-76
    hist_minmax_update_(counts[2 NB], nan[1], running[2, 1], x, mantissa_bits) -> ()  (no reference code: DESIGN.md 4.1h; percentile ranges)
    w8a8_linear(xq, row_sum, wq, alpha, w_zp, col_term, bias?, out_scale?, out_offset?, out_qmin, out_qmax) -> Tensor
                                                                                    QLinear.forward, qmodule.py:341-358
    pack_w4(nibbles) -> uint8                                                       the 4-bit image of a quantised weight
    w4a8_linear(xq, row_sum, w_packed, ...) -> Tensor                               the same linear on packed 4-bit weights
    decode_cache_fork(caches, pos, parent) -> ()                                    (no reference code: DESIGN.md 4.3k; caches in place)
    decode_cache_reorder(caches, pos, parent) -> ()                                 (no reference code: DESIGN.md 4.3l; caches in place)
    beam_select(logits, cum, group, n_groups, n_cand) -> (score, row, token, logprob, row_lse)   (no reference code: DESIGN.md 4.3l)
    lwc_search(w2d, sig_lo, sig_hi, bitwidth, is_symmetric, col_weight?) -> (best_idx, best_cost, base_cost, costs)
                                                                                    (no reference code: DESIGN.md 4.7b; clip search)
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch

from . import ops
from ._lib import MQ_F32, MQ_I8

_NS = "mobilequant_amd"


@torch.library.custom_op(f"{_NS}::fake_quant", mutates_args=(), device_types="cuda")
def fake_quant(x: torch.Tensor, scale: torch.Tensor, offset: torch.Tensor, qmin: float, qmax: float) -> torch.Tensor:
    return ops.fake_quant(x, scale, offset, qmin, qmax)


@fake_quant.register_fake
def _(x, scale, offset, qmin, qmax):
    return torch.empty_like(x, memory_format=torch.contiguous_format)


@torch.library.custom_op(f"{_NS}::quantize", mutates_args=(), device_types="cuda")
def quantize(x: torch.Tensor, scale: torch.Tensor, offset: torch.Tensor, qmin: float, qmax: float, shift: int,
             chan_scale: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    rows = scale.numel() if scale.numel() > 1 else x.numel() // x.shape[-1]
    q, rs = ops.quantize(x, scale, offset, qmin, qmax, q_dtype=MQ_I8, shift=shift, rows=rows, want_row_sum=True, chan_scale=chan_scale)
    return q, rs


@quantize.register_fake
def _(x, scale, offset, qmin, qmax, shift, chan_scale=None):
    rows = scale.numel() if scale.numel() > 1 else x.numel() // x.shape[-1]
    return x.new_empty(x.shape, dtype=torch.int8), x.new_empty((rows,), dtype=torch.int32)


@torch.library.custom_op(f"{_NS}::minmax", mutates_args=(), device_types="cuda")
def minmax(x: torch.Tensor, per_channel: bool) -> torch.Tensor:
    if per_channel:
        mn, mx = ops.minmax_cols(x.reshape(-1, x.shape[-1]).contiguous())
        return torch.stack((mn, mx))
    mn, mx = ops.minmax_tensor(x)
    return torch.cat((mn.reshape(1), mx.reshape(1)))


@minmax.register_fake
def _(x, per_channel):
    return x.new_empty((2, x.shape[-1]) if per_channel else (2,), dtype=torch.float32)


@torch.library.custom_op(f"{_NS}::minmax_update_", mutates_args=("running",), device_types="cuda")
def minmax_update_(running: torch.Tensor, x: torch.Tensor) -> None:
    """running [2, n] (row 0 = min, row 1 = max): n == 1 -> per-tensor statistic of x, n == x.shape[-1] -> per channel."""
    if running.shape[1] == 1:
        ops.minmax_tensor_(x, running[0], running[1])
    else:
        ops.minmax_cols_(x.reshape(-1, x.shape[-1]).contiguous(), running[0], running[1])


@minmax_update_.register_fake
def _(running, x):
    return None


@torch.library.custom_op(f"{_NS}::hist_minmax_update_", mutates_args=("counts", "nan", "running"), device_types="cuda")
def hist_minmax_update_(counts: torch.Tensor, nan: torch.Tensor, running: torch.Tensor, x: torch.Tensor, mantissa_bits: int) -> None:
    """counts int64 [2 * (256 << mantissa_bits)] and nan int64 [1] grow by x's bit-pattern histogram; running [2, 1] (row 0 = min,
    row 1 = max) folds x's min / max in -- one pass over x."""
    ops.hist_minmax_tensor_(x, counts, nan, running[0], running[1], mantissa_bits)


@hist_minmax_update_.register_fake
def _(counts, nan, running, x, mantissa_bits):
    return None


def _linear(xq, row_sum, wq, alpha, w_zp, col_term, bias, out_scale, out_offset, out_qmin, out_qmax, w4):
    return ops.int8_linear(xq, wq, row_sum, alpha, w_zp, col_term, bias, out_scale=out_scale, out_offset=out_offset, out_qmin=out_qmin,
                           out_qmax=out_qmax, out_dtype=MQ_F32, w4=w4)


@torch.library.custom_op(f"{_NS}::w8a8_linear", mutates_args=(), device_types="cuda")
def w8a8_linear(xq: torch.Tensor, row_sum: torch.Tensor, wq: torch.Tensor, alpha: torch.Tensor, w_zp: torch.Tensor, col_term: torch.Tensor,
                bias: Optional[torch.Tensor] = None, out_scale: Optional[torch.Tensor] = None, out_offset: Optional[torch.Tensor] = None,
                out_qmin: float = 0.0, out_qmax: float = 255.0) -> torch.Tensor:
    return _linear(xq, row_sum, wq, alpha, w_zp, col_term, bias, out_scale, out_offset, out_qmin, out_qmax, False)


@w8a8_linear.register_fake
def _(xq, row_sum, wq, alpha, w_zp, col_term, bias=None, out_scale=None, out_offset=None, out_qmin=0.0, out_qmax=255.0):
    return xq.new_empty((xq.shape[0], wq.shape[0]), dtype=torch.float32)


@torch.library.custom_op(f"{_NS}::pack_w4", mutates_args=(), device_types="cuda")
def pack_w4(nibbles: torch.Tensor) -> torch.Tensor:
    return ops.pack_w4(nibbles)


@pack_w4.register_fake
def _(nibbles):
    return nibbles.new_empty((nibbles.shape[0], nibbles.shape[1] // 2), dtype=torch.uint8)


@torch.library.custom_op(f"{_NS}::w4a8_linear", mutates_args=(), device_types="cuda")
def w4a8_linear(xq: torch.Tensor, row_sum: torch.Tensor, w_packed: torch.Tensor, alpha: torch.Tensor, w_zp: torch.Tensor,
                col_term: torch.Tensor, bias: Optional[torch.Tensor] = None, out_scale: Optional[torch.Tensor] = None,
                out_offset: Optional[torch.Tensor] = None, out_qmin: float = 0.0, out_qmax: float = 255.0) -> torch.Tensor:
    return _linear(xq, row_sum, w_packed, alpha, w_zp, col_term, bias, out_scale, out_offset, out_qmin, out_qmax, True)


@w4a8_linear.register_fake
def _(xq, row_sum, w_packed, alpha, w_zp, col_term, bias=None, out_scale=None, out_offset=None, out_qmin=0.0, out_qmax=255.0):
    return xq.new_empty((xq.shape[0], w_packed.shape[0]), dtype=torch.float32)


@torch.library.custom_op(f"{_NS}::decode_cache_fork", mutates_args=("caches",), device_types="cuda")
def decode_cache_fork(caches: List[torch.Tensor], pos: torch.Tensor, parent: torch.Tensor) -> None:
    ops.decode_cache_fork(caches, pos, parent)


@decode_cache_fork.register_fake
def _(caches, pos, parent):
    return None


@torch.library.custom_op(f"{_NS}::decode_cache_reorder", mutates_args=("caches",), device_types="cuda")
def decode_cache_reorder(caches: List[torch.Tensor], pos: torch.Tensor, parent: torch.Tensor) -> None:
    ops.decode_cache_reorder(caches, pos, parent)


@decode_cache_reorder.register_fake
def _(caches, pos, parent):
    return None


@torch.library.custom_op(f"{_NS}::beam_select", mutates_args=(), device_types="cuda")
def beam_select(logits: torch.Tensor, cum: torch.Tensor, group: torch.Tensor, n_groups: int,
                n_cand: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    return ops.beam_select(logits, cum, group, n_groups, n_cand)


@beam_select.register_fake
def _(logits, cum, group, n_groups, n_cand):
    rows = logits.shape[0] if logits.dim() == 2 else 1
    f, i = (lambda *sh: logits.new_empty(sh, dtype=torch.float32)), (lambda *sh: logits.new_empty(sh, dtype=torch.int32))
    return f(n_groups, n_cand), i(n_groups, n_cand), i(n_groups, n_cand), f(n_groups, n_cand), f(rows)


@torch.library.custom_op(f"{_NS}::lwc_search", mutates_args=(), device_types="cuda")
def lwc_search(w2d: torch.Tensor, sig_lo: torch.Tensor, sig_hi: torch.Tensor, bitwidth: int, is_symmetric: bool,
               col_weight: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(best_idx int32 [rows], best_cost fp64 [rows], base_cost fp64 [rows], costs fp64 [rows, C]) of ops.lwc_search."""
    return ops.lwc_search(w2d, sig_lo, sig_hi, bitwidth, is_symmetric, col_weight, return_costs=True)


@lwc_search.register_fake
def _(w2d, sig_lo, sig_hi, bitwidth, is_symmetric, col_weight=None):
    rows, C = w2d.shape[0], sig_lo.shape[0]
    d = lambda *sh: w2d.new_empty(sh, dtype=torch.float64)  # noqa: E731
    return w2d.new_empty((rows,), dtype=torch.int32), d(rows), d(rows), d(rows, C)


OPS = ("fake_quant", "quantize", "minmax", "minmax_update_", "hist_minmax_update_", "w8a8_linear", "pack_w4", "w4a8_linear", "decode_cache_fork", "decode_cache_reorder",
       "beam_select", "lwc_search")
