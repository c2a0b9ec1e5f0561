"""Ragged decode steps: BatchDecodeEngine.step_tokens at R = 8 rows spread over the slots as 8x1, 4x2, 2x4 and 1x8 (slots x tokens per
slot) against BatchDecodeEngine.step() at B = R and, for the 1x8 plan, DecodeEngine.step_tokens at T = R -- all timed in the same
process on the full-size TinyLlama shape, W8A8 and W4A8, at 256 and 2 048 cached positions.

    python tools/bench_decode_ragged.py [--steps 64] [--contexts 256,2048] [--wbits 8,4]

Protocol of tools/bench_decode_multi.py: random-init model -> the reference's surgery and mixed-precision rules -> one calibration pass
-> engines; random cached keys / values (fill_cache_random); captured hipGraphs (the ragged step: ONE graph for all four plans, the
plan is device data); HIP events around `steps` graph replays, best of 3.  The replays of a ragged plan run the uploaded row table
again and again: the same rows at the same positions.  Prints ONE JSON line.
  ragged_{S}x{T}_ctx{c}: the 8-row ragged step with S slots moving T tokens each; x_batch = its time over the batched step at B = 8 and
    the same positions (the goal DESIGN.md 4.3d set: <= 1.1), goal = "hit" / "miss".
  batch8_ctx{c}: BatchDecodeEngine.step() at B = 8.   multi8_{L}launch_ctx{c}: DecodeEngine.step_tokens at T = 8 (L launches)."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_decode_batch import _model, _time  # noqa: E402

R = 8
PLANS = [(8, 1), (4, 2), (2, 4), (1, 8)]          # (slots, tokens per slot)
GOAL = 1.1


def run(wbits, contexts, steps, dev):
    from mobilequant_amd.decode import DecodeEngine
    from mobilequant_amd.decode_batch import BatchDecodeEngine
    cache_len = (max(contexts) + steps * R + 16 + 15) // 16 * 16
    model, shape = _model(dev, wbits, max(2048, cache_len))
    out = {}
    be = BatchDecodeEngine(model, R, cache_len=cache_len)
    assert be.max_rows == R
    for b in range(R):
        be.fill_cache_random(b, max(contexts), seed=b)
    be.tok.fill_(17)
    be.capture()

    def set_pos(ctx):
        for b in range(R):
            be.set_position(b, ctx)
    for ctx in contexts:
        ms = _time(be.graph.replay, lambda: set_pos(ctx), steps)
        out[f"batch{R}_ctx{ctx}"] = {"ms_per_step": round(ms, 4)}
    for slots, toks in PLANS:
        for ctx in contexts:
            def prime(ctx=ctx, slots=slots, toks=toks):
                set_pos(ctx)
                be.step_tokens({b: [17] * toks for b in range(slots)})      # uploads the plan at ctx (and records the R-row graph once)
            ms = _time(lambda: be._row_graphs[R].replay(), prime, steps)
            x = ms / out[f"batch{R}_ctx{ctx}"]["ms_per_step"]
            out[f"ragged_{slots}x{toks}_ctx{ctx}"] = {"ms_per_step": round(ms, 4), "x_batch": round(x, 3), "goal": "hit" if x <= GOAL else "miss"}
    assert set(be._row_graphs) == {R}                          # one graph served every plan
    del be
    torch.cuda.empty_cache()
    for L in (4, 5):
        eng = DecodeEngine(model, cache_len=cache_len, launches=L)
        eng.fill_cache_random(max(contexts))
        eng.capture()
        eng.set_position(min(contexts))
        eng.step_tokens([17] * R)                              # records the T-row graph
        for ctx in contexts:
            ms = _time(eng._row_graphs[R].replay, lambda: eng.set_position(ctx), steps)
            out[f"multi{R}_{eng.launches}launch_ctx{ctx}"] = {"ms_per_step": round(ms, 4),
                                                            "ragged_1x8_over_it": round(out[f"ragged_1x{R}_ctx{ctx}"]["ms_per_step"] / ms, 3)}
        del eng
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--contexts", default="256,2048")
    ap.add_argument("--wbits", default="8,4")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_decode_ragged needs the GPU"
    dev = torch.device("cuda:0")
    contexts = [int(c) for c in a.contexts.split(",")]
    res = {"metric": "decode_ragged_tinyllama", "steps": a.steps, "unit": "ms per step", "goal_x_batch": GOAL}
    for wb in (int(w) for w in a.wbits.split(",")):
        res["w8a8" if wb == 8 else "w4a8"] = run(wb, contexts, a.steps, dev)
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
