#!/usr/bin/env python3
"""Decode speed of a weight-only (W4A16) TinyLlama: tokens/s at 256 and 2 048 cached positions, group_size 128,
random-init weights.

Three figures per cache length:
  engine        WeightOnlyDecodeEngine after capture(): one hipGraph replay per token;
  module_chain  the same model stepped as `model(ids[:, t:t+1], cache, pos=t)` -- what a user had before the engine;
  w4a8_engine   for context: DecodeEngine (captured) on the same shape with W4A8 QLinear chains (8-bit activations, int8 caches).
Method: the cache is filled to the stated position (random rows: the time does not depend on the values), then `steps` steps are run
between two HIP events after a warm-up, the position put back each round; the figure is the median round over `steps`.  The engine's
per-launch times are one step's launches replayed `inner` times each from a graph of that launch alone (weights L2 / Infinity-Cache
warm, so they add up to less than a step in which every launch streams from HBM): they say where the time is, not how long a step
takes.  The shader clock is not pinned: the sclk rocm-smi reports before and after is printed (read only).

    python tools/bench_w4a16_decode.py [--steps 32] [--rounds 7] [--positions 256 2048] [--attn-splits N] [--no-context]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from bench_w4a16 import graph_time, sclk  # noqa: E402

GROUP = 128


def weight_only_model(dev, max_pos):
    import mobilequant_amd.quantization.qmodule as Q
    from mobilequant_amd.llama import LlamaForCausalLM, LlamaShape
    model = LlamaForCausalLM(LlamaShape.tinyllama(max_pos=max_pos))
    model.reset_parameters(seed=1337)
    model = model.to(dev).eval().requires_grad_(False)
    return Q.create_weight_only_qmodel(model, Q.QuantConfig(bitwidth=4, group_size=GROUP, is_symmetric=False, is_per_channel=True))


def rounds_us(step, restore, steps, rounds):
    """Median microseconds per step of `steps` calls of step() between two events; restore() puts the position back before each round."""
    out = []
    for r in range(rounds + 1):
        restore()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            step()
        e1.record()
        e1.synchronize()
        if r:                                                   # round 0 warms up
            out.append(e0.elapsed_time(e1) * 1e3 / steps)
    return statistics.median(out), min(out), max(out)


def per_launch(eng, inner=32, repeats=9):
    """[(entry, median us)] of one step's launches, each replayed alone."""
    from mobilequant_amd import _lib
    st = lambda: torch.cuda.current_stream(eng.dev).cuda_stream   # noqa: E731
    out = []
    for entry, a in eng.phases[:5]:                              # layer 0: the other layers repeat it
        t = graph_time(lambda i, entry=entry, a=a: _lib.call(entry, ctypes.byref(a), st()), 1, inner, repeats)
        out.append((entry, round(statistics.median(t), 2)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--positions", type=int, nargs="+", default=[256, 2048])
    ap.add_argument("--no-context", action="store_true", help="skip the W4A8 DecodeEngine figure")
    ap.add_argument("--attn-splits", type=int, default=None, help="workgroups per head of the attention launch (default: the engine's choice)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_w4a16_decode.py measures on the GPU only"
    dev = torch.device("cuda:0")
    from mobilequant_amd import WeightOnlyDecodeEngine
    print(json.dumps({"sclk_before": sclk()}), flush=True)
    cache_len = max(args.positions) + args.steps + 16
    model = weight_only_model(dev, cache_len)
    g = torch.Generator(device=dev).manual_seed(3)
    for P in args.positions:
        eng = WeightOnlyDecodeEngine(model, cache_len=cache_len, attn_splits=args.attn_splits)
        for k, v in eng.caches:
            k[:, :, :P].normal_(generator=g)
            v[:, :, :P].normal_(generator=g)
        eng.tok.fill_(17)
        res = {"cached_positions": P, "attn_splits": eng.attn_splits, "launches_per_token": eng.launches_per_token}
        eng.set_position(P)
        eager = rounds_us(lambda: eng.step(), lambda: eng.set_position(P), args.steps, 2)
        eng.capture()
        us = rounds_us(lambda: eng.step(), lambda: eng.set_position(P), args.steps, args.rounds)
        res["engine"] = {"us_per_token": round(us[0], 1), "tok_s": round(1e6 / us[0], 1), "spread_us": [round(us[1], 1), round(us[2], 1)],
                         "uncaptured_us_per_token": round(eager[0], 1)}
        res["engine_launch_us_layer0"] = per_launch(eng)
        ids = torch.full((1, 1), 17, dtype=torch.int64, device=dev)
        pos = [P]

        def chain_step():
            with torch.no_grad():
                model(ids, cache=eng.caches, pos=pos[0])
            pos[0] += 1
        us = rounds_us(chain_step, lambda: pos.__setitem__(0, P), args.steps, max(3, args.rounds // 2))
        res["module_chain"] = {"us_per_token": round(us[0], 1), "tok_s": round(1e6 / us[0], 1), "spread_us": [round(us[1], 1), round(us[2], 1)]}
        res["engine_over_module_chain"] = round(res["module_chain"]["us_per_token"] / res["engine"]["us_per_token"], 2)
        print(json.dumps(res), flush=True)
        del eng
    if not args.no_context:
        from bench_decode_batch import _model
        from mobilequant_amd.decode import DecodeEngine
        qmodel, _ = _model(dev, 4, cache_len // 16 * 16 + 16)
        for P in args.positions:
            eng = DecodeEngine(qmodel, cache_len=cache_len // 16 * 16 + 16)
            eng.fill_cache_random(P)
            eng.tok.fill_(17)
            eng.capture()
            us = rounds_us(lambda: eng.step(), lambda: eng.set_position(P), args.steps, args.rounds)
            print(json.dumps({"cached_positions": P, "w4a8_engine": {"us_per_token": round(us[0], 1), "tok_s": round(1e6 / us[0], 1),
                                                                     "spread_us": [round(us[1], 1), round(us[2], 1)]}}), flush=True)
            del eng
    print(json.dumps({"sclk_after": sclk()}), flush=True)


if __name__ == "__main__":
    main()
