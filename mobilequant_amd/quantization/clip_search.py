"""Model-level clip search (no counterpart in the reference, which obtains clip factors by training only): Quantizer.search_lwc over every
eligible QLinear of a model.  DESIGN.md 4.7b; the recipes are in INTEGRATION.md."""
from __future__ import annotations

from typing import Dict, Optional

import torch

from .qmodule import LwcSearchReport, QLinear

__all__ = ["search_weight_clipping", "ClipSearchResult"]


class ClipSearchResult(Dict[str, LwcSearchReport]):
    """name -> LwcSearchReport of every searched QLinear; ``skipped``: name -> reason for every other module with a weight quantizer;
    ``summary``: one line with the totals."""

    def __init__(self):
        super().__init__()
        self.skipped: Dict[str, str] = {}

    @property
    def summary(self) -> str:
        rows = sum(r.rows for r in self.values())
        clipped = sum(r.clipped_rows for r in self.values())
        base, best = sum(r.base_cost for r in self.values()), sum(r.best_cost for r in self.values())
        gain = f", cost {base:.6g} -> {best:.6g}" if self else ""
        return f"{len(self)} QLinear weights searched ({clipped} of {rows} rows clipped{gain}), {len(self.skipped)} modules skipped"


def _act_scale_of(act_scales, name: str) -> torch.Tensor:
    for key in (name + "_input", name):              # get_act_scales keys "<module>_<field>"
        if key in act_scales:
            return act_scales[key]
    raise KeyError(f"mobilequant_amd: act_scales has no entry for {name!r} (looked for {name + '_input'!r})")


@torch.no_grad()
def search_weight_clipping(model, *, n_grid: int = 64, min_ratio: float = 0.5, act_scales: Optional[dict] = None, mode: str = "joint",
                           fold: bool = False) -> ClipSearchResult:
    """Quantizer.search_lwc on the weight of every QLinear whose weight quantizer is eligible (per-channel or per-group, at most 8 bits,
    not dynamic); every other module that has a weight quantizer is listed in ``.skipped`` with the reason.  act_scales: the dict of
    get_act_scales (per-input-channel abs-max, "<name>_input" -> [K]); when given the error of input channel k weighs scales[k] ** 2
    (fp32).  fold=True ends as the reference's training ends (algorithm.py:181-184): ``weight.data = run_lwc(weight)`` clamps every
    searched weight to its chosen range and drops the LWC state, so the model runs through the fused prefill and the decode engines
    like any other.  Without fold the quantizers stay ordinary LWC quantizers, a better start for the training loops."""
    out = ClipSearchResult()
    for name, mod in model.named_modules():
        wq = getattr(mod, "weight_quantizer", None)
        if wq is None:
            continue
        if not isinstance(mod, QLinear):
            out.skipped[name] = f"{type(mod).__name__} is not a QLinear"
            continue
        why = wq.lwc_search_skip_reason(mod.weight)
        if why is not None:
            out.skipped[name] = why
            continue
        cw = None
        if act_scales is not None:
            sc = _act_scale_of(act_scales, name).detach().to(device=mod.weight.device, dtype=torch.float32).reshape(-1)
            cw = sc * sc
        out[name] = wq.search_lwc(mod.weight, n_grid=n_grid, min_ratio=min_ratio, col_weight=cw, mode=mode)
        if fold:
            mod.weight.data = wq.run_lwc(mod.weight)
    return out
