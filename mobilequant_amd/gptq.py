"""GPTQ: error-compensated rounding of weights onto a fixed grid, on mq_gptq_round (csrc/mq_gptq.hip; the contract: DESIGN.md 4.10).

Round-to-nearest rounds every weight on its own.  GPTQ walks the columns of W, rounds one column and pushes its rounding error onto
the columns not yet rounded, through the upper Cholesky factor U of the inverse input Hessian (H = 2 X^T X / tokens):

    for t = 0 .. K-1:   k = perm[t]
        q   = clamp(round(w[k] / s) + o, qmin, qmax);   dq = (q - o) * s
        e   = (w[k] - dq) / U[t, t]
        w[perm[t']] -= e * U[t, t']          for every t' > t        (one fp32 fma each)

The grid (scale, offset per row and group, in the original column order: static groups) is fixed up front, so the result is a better
choice of INDICES on the grid the rest of the package already runs on: the packers, the W4A16 / W4A8 kernels and state_dict do not
change.  `gptq_factor` is plain torch in float64 (CPU tensors allowed); `gptq_round` runs on the device and raises otherwise.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Iterable, NamedTuple, Optional

import torch
import torch.nn as nn

from . import _lib, ops

__all__ = ["gptq_factor", "gptq_round", "GptqResult", "HessianCollector", "gptq_quantize_model", "GptqReport", "GptqLine"]

MIN_K, MAX_K = 16, 16384


class GptqResult(NamedTuple):
    index: torch.Tensor          # uint8 [N, K]: index - qmin at the original column (the form mq_pack_w4 reads)
    dequantized: torch.Tensor    # fp32 [N, K]: (index - offset) * scale
    loss: torch.Tensor           # fp64 [N]: sum over the steps of e^2


def gptq_factor(H: torch.Tensor, percdamp: float = 0.01, act_order: bool = False):
    """(U fp32 [K, K], perm int32 [K] | None, dead bool [K]) of an input Hessian H [K, K], in float64 on H's device:
    columns with a zero diagonal get H[k, k] = 1 and are reported in `dead`; with act_order, perm = argsort(diag, descending, stable)
    and H is permuted; H += percdamp * mean(diag) * I; U = cholesky(cholesky_inverse(cholesky(H)), upper=True), rounded once to fp32
    (H^-1 = U^T U in walk order).  ValueError when a factorization fails: percdamp is too small for this H."""
    if not torch.is_tensor(H) or H.dim() != 2 or H.shape[0] != H.shape[1] or not H.dtype.is_floating_point:
        raise ValueError(f"mobilequant_amd: gptq_factor takes a square floating-point Hessian (got {getattr(H, 'shape', type(H))})")
    H = H.detach().to(torch.float64).clone()
    K = H.shape[0]
    diag = torch.diagonal(H)
    dead = diag == 0
    diag[dead] = 1.0                                              # (a view: writes H's diagonal)
    perm = None
    if act_order:
        perm = torch.argsort(torch.diagonal(H), descending=True, stable=True)
        H = H[perm][:, perm].contiguous()
    H.diagonal().add_(float(percdamp) * float(torch.diagonal(H).mean()))
    why = f"mobilequant_amd: gptq_factor: the Cholesky factorization failed: percdamp = {percdamp} is too small for this H ([{K}, {K}])"
    if not bool(torch.isfinite(H).all()):
        raise ValueError(why + " (H is not finite)")
    L, info = torch.linalg.cholesky_ex(H)
    if int(info) != 0:
        raise ValueError(why)
    Hinv = torch.cholesky_inverse(L)
    U, info = torch.linalg.cholesky_ex(Hinv, upper=True)
    if int(info) != 0 or not bool(torch.isfinite(U).all()):
        raise ValueError(why)
    return U.to(torch.float32).contiguous(), (None if perm is None else perm.to(torch.int32)), dead


def _groups(K: int, group_size: int):
    g = K if group_size == -1 else int(group_size)
    if g <= 0 or K % g:
        raise ValueError(f"mobilequant_amd: gptq_round group_size {group_size} does not divide K = {K}")
    if g % 4:
        raise ValueError(f"mobilequant_amd: gptq_round group_size {g} must be a multiple of 4")
    return g, K // g


def gptq_round(w: torch.Tensor, scale: torch.Tensor, offset: torch.Tensor, qmin: int, qmax: int, U: torch.Tensor, group_size: int = -1,
               perm: Optional[torch.Tensor] = None, dead: Optional[torch.Tensor] = None) -> GptqResult:
    """GPTQ rounding of w [N, K] (fp32, device) onto the grid scale / offset [N, K / group_size] (any floating dtype, read as fp32),
    on w's device and the current stream.  U [K, K] fp32 and perm int32 [K] | None as gptq_factor returns them (moved to the device by
    the caller; passed as they are); dead bool [K] | None: those columns of the working copy are zeroed first, as GPTQ does.  w itself
    is not modified.  perm is checked to be a permutation (one host read)."""
    ops._dev(w, "gptq_round w")
    if w.dim() != 2:
        raise RuntimeError(f"mobilequant_amd: gptq_round w must be [N, K] (got {tuple(w.shape)})")
    N, K = w.shape
    ops._raw(w, "gptq_round w", torch.float32, N * K)
    if K % 4 or not MIN_K <= K <= MAX_K:
        raise ValueError(f"mobilequant_amd: gptq_round takes rows of {MIN_K} to {MAX_K} columns, a multiple of 4 (got K = {K})")
    g, G = _groups(K, group_size)
    qmin, qmax = int(qmin), int(qmax)
    if not qmin < qmax <= qmin + 255:
        raise ValueError(f"mobilequant_amd: gptq_round needs qmin < qmax <= qmin + 255, bit widths 2 to 8 (got {qmin}, {qmax})")
    s = ops._f32(scale, "gptq_round scale", align16=True)
    o = ops._f32(offset, "gptq_round offset", align16=True)
    if s.numel() != N * G or o.numel() != N * G:
        raise RuntimeError(f"mobilequant_amd: gptq_round needs one (scale, offset) per row and group, {N} x {G} (got {s.numel()}, {o.numel()})")
    ops._raw(U, "gptq_round U", torch.float32, K * K)
    if U.data_ptr() % 16:
        raise RuntimeError("mobilequant_amd: gptq_round U must be 16-byte aligned")
    if perm is not None:
        ops._raw(perm, "gptq_round perm", torch.int32, K)
        if perm.data_ptr() % 16:
            raise RuntimeError("mobilequant_amd: gptq_round perm must be 16-byte aligned")
        if not bool((torch.sort(perm.to(torch.int64)).values == torch.arange(K, device=perm.device)).all()):
            raise ValueError(f"mobilequant_amd: gptq_round perm is not a permutation of 0 .. {K - 1}")
    work = w
    if dead is not None:
        ops._raw(dead, "gptq_round dead", torch.bool, K)
        work = w.clone()
        work[:, dead] = 0.0
    work = ops._al16(work)
    index = torch.empty((N, K), dtype=torch.uint8, device=w.device)
    deq = torch.empty((N, K), dtype=torch.float32, device=w.device)
    loss = torch.empty((N,), dtype=torch.float64, device=w.device)
    if N == 0:
        return GptqResult(index, deq, loss)
    nbytes = int(_lib.load().mq_gptq_workspace_bytes(N, K))
    if nbytes < 0:
        raise ValueError(f"mobilequant_amd: gptq_round does not serve N = {N}, K = {K} (K times N rounded up to 64 stays below 2^31)")
    workspace = torch.empty((nbytes,), dtype=torch.uint8, device=w.device)
    a = _lib.MqGptqArgs()
    a.w, a.N, a.K, a.group_size = work.data_ptr(), N, K, g
    a.scale, a.offset, a.qmin, a.qmax = s.data_ptr(), o.data_ptr(), float(qmin), float(qmax)
    a.u, a.perm = U.data_ptr(), (perm.data_ptr() if perm is not None else None)
    a.workspace, a.workspace_bytes = workspace.data_ptr(), nbytes
    a.index, a.w_deq, a.loss = index.data_ptr(), deq.data_ptr(), loss.data_ptr()
    with ops._on(work, s, o, U, perm, workspace, index, deq, loss):
        _lib.call("mq_gptq_round", ctypes.byref(a), ops._stream())
    del work, s, o, workspace          # (the caching allocator keeps them until the stream has passed the launches)
    return GptqResult(index, deq, loss)


# ---- the input Hessians ----------------------------------------------------------------------------------------------------------------
class _Shared:
    """One accumulator for every module that is handed the SAME input tensor in one forward (q | k | v, w1 | w3)."""

    def __init__(self):
        self.H: Optional[torch.Tensor] = None
        self.tokens = 0
        self.last = None          # the input accumulated last, kept alive so that `is` identifies it


def _is_candidate(mod) -> bool:
    return isinstance(mod, nn.Linear)          # QLinear is one; a plain nn.Linear is a WeightOnlyLinear-to-be


class HessianCollector:
    """Context manager: forward pre-hooks on every nn.Linear / QLinear of `model` (names: only these; a name containing `lm_head` is
    left out unless it is listed) accumulate H += X^T X in fp32 (torch.addmm_: a library GEMM, plumbing as in calibration) and the token
    count, over every forward run inside the `with`.  Modules that are handed the same input tensor in the same forward share one H.
    ``hessian(name)`` -> 2 H / tokens, fp32 [K, K]."""

    def __init__(self, model, names: Optional[Iterable[str]] = None):
        self.model = model
        wanted = None if names is None else set(names)
        self.modules: Dict[str, nn.Module] = {}
        for name, mod in model.named_modules():
            if not _is_candidate(mod):
                continue
            if wanted is not None:
                if name in wanted:
                    self.modules[name] = mod
            elif "lm_head" not in name:
                self.modules[name] = mod
        if wanted is not None and wanted - set(self.modules):
            raise KeyError(f"mobilequant_amd: HessianCollector: not linears of this model: {sorted(wanted - set(self.modules))}")
        self._slot: Dict[str, _Shared] = {}
        self._slots: list = []
        self._handles: list = []

    def __enter__(self):
        for name, mod in self.modules.items():
            self._handles.append(mod.register_forward_pre_hook(self._hook(name)))
        return self

    def __exit__(self, *exc):
        for h in self._handles:
            h.remove()
        self._handles = []
        for sl in self._slots:
            sl.last = None
        return False

    def _hook(self, name):
        def pre(_mod, args):
            x = args[0]
            if not torch.is_tensor(x) or not x.dtype.is_floating_point:
                return
            sl = self._slot.get(name)
            if sl is None:
                sl = next((c for c in self._slots if c.last is x), None)          # a sibling took this very tensor already
                if sl is not None:
                    self._slot[name] = sl
                    return
                sl = self._slot[name] = _Shared()
                self._slots.append(sl)
            elif sl.last is x:
                return
            with torch.no_grad():
                x2 = x.detach().reshape(-1, x.shape[-1]).to(torch.float32)
                if sl.H is None:
                    sl.H = torch.zeros((x2.shape[1], x2.shape[1]), dtype=torch.float32, device=x2.device)
                sl.H.addmm_(x2.t(), x2)
                sl.tokens += x2.shape[0]
            sl.last = x
        return pre

    def tokens(self, name: str) -> int:
        sl = self._slot.get(name)
        return 0 if sl is None else sl.tokens

    def shares(self, a: str, b: str) -> bool:
        return a in self._slot and self._slot.get(a) is self._slot.get(b)

    def hessian(self, name: str) -> torch.Tensor:
        sl = self._slot.get(name)
        if sl is None or sl.H is None or sl.tokens == 0:
            raise KeyError(f"mobilequant_amd: HessianCollector saw no input of {name!r}")
        return sl.H * (2.0 / sl.tokens)


# ---- a model ---------------------------------------------------------------------------------------------------------------------------
class GptqLine(NamedTuple):
    rtn_error: float          # tr(dW H dW^T) of round-to-nearest on the same grid, float64 on the collected H
    gptq_error: float         # the same of the GPTQ indices
    loss_sum: float           # the kernel's sum of e^2 over rows and steps
    changed_fraction: float   # share of the indices that differ from round-to-nearest


class GptqReport(Dict[str, GptqLine]):
    """name -> GptqLine of every converted linear; ``skipped``: name -> reason; ``summary``: one line with the totals."""

    def __init__(self):
        super().__init__()
        self.skipped: Dict[str, str] = {}

    @property
    def summary(self) -> str:
        rtn, gq = sum(r.rtn_error for r in self.values()), sum(r.gptq_error for r in self.values())
        gain = f", layer objective {rtn:.6g} -> {gq:.6g}" if self else ""
        return f"{len(self)} linears rounded by GPTQ{gain}, {len(self.skipped)} modules skipped"


def _objective(dw: torch.Tensor, H64: torch.Tensor) -> float:
    dw = dw.to(torch.float64)
    return float(((dw @ H64) * dw).sum())


def _shape_reason(K: int, g: int) -> Optional[str]:
    if K % 4 or not MIN_K <= K <= MAX_K:
        return f"rows of {K} columns (GPTQ rounding takes {MIN_K} to {MAX_K}, a multiple of 4)"
    if g <= 0 or K % g:
        return f"group_size {g} does not divide K = {K}"
    if g % 4:
        return f"group_size {g} is not a multiple of 4"
    return None


def _qlinear_reason(mod) -> Optional[str]:
    wq = mod.weight_quantizer
    if wq is None or wq.bypassed():
        return "weight quantizer is absent or bypassed"
    if not wq.qcfg.is_per_channel:
        return "per-tensor weight grid"
    if wq.qcfg.bitwidth > 8:
        return f"{wq.qcfg.bitwidth}-bit weight grid"
    if wq.qcfg.is_dynamic:
        return "dynamic weight grid"
    if getattr(mod, "input_chan_scale", None) is not None:
        return "run-time input channel scale (the Hessian of x / s is not collected)"
    K = mod.weight.shape[1]
    return _shape_reason(K, K if wq.qcfg.group_size == -1 else int(wq.qcfg.group_size))


def _run(model, sample):
    if isinstance(sample, dict):
        return model(**sample)
    if isinstance(sample, (tuple, list)):
        return model(*sample)
    return model(sample)


def _freeze_grid(wq, scale: torch.Tensor, offset: torch.Tensor) -> None:
    """Leave (scale, offset) on the quantizer as an ordinary static grid: no LWC state, not an auto grid (never re-derived)."""
    kind = "buffer" if "scale" in wq._buffers else "parameter"
    wq.disable_lwc()
    wq._gen = getattr(wq, "_gen", 0) + 1
    for name in ("scale", "offset"):
        if hasattr(wq, name):
            delattr(wq, name)
    scale, offset = scale.detach().clone(), offset.detach().clone()
    if kind == "buffer":
        wq.register_buffer("scale", scale)
        wq.register_buffer("offset", offset)
    else:
        wq.register_parameter("scale", nn.Parameter(scale))
        wq.register_parameter("offset", nn.Parameter(offset))
    wq._host_range = None
    wq._auto_grid = False


@torch.no_grad()
def gptq_quantize_model(model, samples, w_qcfg=None, *, percdamp: float = 0.01, act_order: bool = False, weight_only: bool = False,
                        names: Optional[Iterable[str]] = None) -> GptqReport:
    """One collection pass of `model` as it stands over `samples` (an iterable of inputs: a tensor, a tuple or a dict per forward),
    then gptq_factor + gptq_round on every eligible linear, written back.  Sequential re-collection after each block is out of scope.

    QLinear: the grid is the one its weight quantizer uses on the current weight (per-channel or per-group, at most 8 bits, not
    dynamic; an LWC quantizer's clipped grid counts, so this composes with search_weight_clipping).  Afterwards weight.data is the
    dequantized weight and the quantizer holds that grid as an ordinary static grid without LWC state: Quantizer(weight) reproduces
    the GPTQ indices bit for bit (asserted).  nn.Linear: the grid comes from w_qcfg (min / max of the weight); the weight becomes the
    dequantized weight.  weight_only=True: scales are rounded to fp16 BEFORE the rounding, so the error feedback sees the deployed
    scale, and every converted module is replaced through to_weight_only_quantized_linear(module, w_qcfg, w_scale=, w_offset=), which
    re-derives the same indices from the dequantized weight (4-bit grids; its refusals are raised).  names: only these modules; a name
    containing `lm_head` is left out by default.  Returns a GptqReport."""
    from .quantization import qmodule as Q
    report = GptqReport()
    names = None if names is None else list(names)
    for name, mod in model.named_modules():
        if _is_candidate(mod) and "lm_head" in name and (names is None or name not in names):
            report.skipped[name] = "lm_head stays in floating point"
    with HessianCollector(model, names) as hc:
        for sample in samples:
            _run(model, sample)
    parents = {}
    for pname, parent in model.named_modules():
        for cname, child in parent._modules.items():
            parents[(pname + "." if pname else "") + cname] = (parent, cname)
    for name, mod in hc.modules.items():
        if isinstance(mod, Q.QLinear):
            why = _qlinear_reason(mod)
            cfg = mod.weight_quantizer.qcfg if why is None else None
        else:
            if w_qcfg is None:
                why = "a plain nn.Linear needs w_qcfg"
            elif not w_qcfg.is_per_channel or w_qcfg.bitwidth > 8 or w_qcfg.is_dynamic:
                why = "w_qcfg must be per-channel or per-group, at most 8 bits, not dynamic"
            else:
                K = mod.weight.shape[1]
                why = _shape_reason(K, K if w_qcfg.group_size == -1 else int(w_qcfg.group_size))
            cfg = w_qcfg
        if why is None and hc.tokens(name) == 0:
            why = "no calibration input reached it"
        if why is None and not mod.weight.is_cuda:
            why = "weight is not on a ROCm device"
        if why is not None:
            report.skipped[name] = why
            continue
        weight = mod.weight.detach().to(torch.float32).contiguous()
        N, K = weight.shape
        g = K if cfg.group_size == -1 else int(cfg.group_size)
        G = K // g
        if isinstance(mod, Q.QLinear):
            wq = mod.weight_quantizer
            wq(weight)                                            # leaves the grid it uses on this weight (the clipped one under LWC)
            scale, offset, qmin, qmax = wq.scale.detach(), wq.offset.detach(), int(wq.qmin), int(wq.qmax)
        else:
            mn, mx = Q.compute_min_max_from_tensor(weight, True, cfg.group_size)
            scale, offset, _, _, qmin, qmax = Q.compute_scale_offset_from_min_max(mn, mx, cfg.bitwidth, cfg.is_symmetric)
            qmin, qmax = int(qmin), int(qmax)
        if scale.numel() != N * G or offset.numel() != N * G:
            report.skipped[name] = f"the weight grid holds {scale.numel()} scales, {N} x {G} are needed"
            continue
        scale = scale.to(device=weight.device, dtype=torch.float32).reshape(N, G).contiguous()
        offset = offset.to(device=weight.device, dtype=torch.float32).reshape(N, G).contiguous()
        if weight_only:
            scale = scale.to(torch.float16).to(torch.float32)    # what WeightOnlyLinear multiplies by
        H = hc.hessian(name)
        U, perm, dead = gptq_factor(H, percdamp, act_order)
        res = gptq_round(weight, scale, offset, qmin, qmax, U, g, perm, dead if bool(dead.any()) else None)
        rows = weight.reshape(N * G, g)
        rtn_idx = ops.quantize(rows, scale.reshape(-1), offset.reshape(-1), qmin, qmax, q_dtype=_lib.MQ_U8, shift=qmin, rows=N * G).view(N, K)
        rtn = ops.fake_quant(rows, scale.reshape(-1), offset.reshape(-1), qmin, qmax).view(N, K)
        again = ops.quantize(res.dequantized.reshape(N * G, g), scale.reshape(-1), offset.reshape(-1), qmin, qmax, q_dtype=_lib.MQ_U8,
                             shift=qmin, rows=N * G).view(N, K)
        if not torch.equal(again, res.index):
            raise RuntimeError(f"mobilequant_amd: {name}: quantizing the GPTQ weight does not return the GPTQ indices "
                               f"({int((again != res.index).sum())} of {N * K} differ): a non-finite weight or a degenerate grid")
        H64 = H.to(torch.float64)
        report[name] = GptqLine(_objective(rtn - weight, H64), _objective(res.dequantized - weight, H64), float(res.loss.sum()),
                                float((rtn_idx != res.index).sum()) / float(N * K))
        mod.weight.data = res.dequantized.to(mod.weight.dtype)
        if isinstance(mod, Q.QLinear):
            _freeze_grid(mod.weight_quantizer, scale.reshape(N * G, 1) if G > 1 else scale.reshape(N, 1),
                         offset.reshape(N * G, 1) if G > 1 else offset.reshape(N, 1))
            mod._plan = None
            mod._scaled_weight = None
        if weight_only:
            parent, cname = parents[name]
            parent._modules[cname] = Q.to_weight_only_quantized_linear(mod, cfg, w_scale=scale, w_offset=offset, name=name)
    return report
