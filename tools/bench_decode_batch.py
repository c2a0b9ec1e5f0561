"""Batched decode throughput: BatchDecodeEngine at B = 1, 2, 4, 8 against the single-sequence DecodeEngine (four and five launches),
timed in the same process on the full-size TinyLlama shape, W8A8 and W4A8, at 256 and 2 048 cached positions.

    python tools/bench_decode_batch.py [--steps 64] [--contexts 256,2048] [--batches 1,2,4,8] [--wbits 8,4] [--group-size G] [--trace]

Recipe of bench.bench_decode_full: random-init model -> the reference's surgery and mixed-precision rules -> one calibration pass ->
engines; random cached keys / values (fill_cache_random, per slot); one captured hipGraph per step; HIP events around `steps` graph
replays, best of 3.  Prints ONE JSON line.  --trace: a short run without timing for `rocprofv3 --kernel-trace --stats`
(B = 1 and B = 8 at 256 positions, W8A8).  --group-size G: per wbits also a model with per-group weight grids of G input channels on
every linear (mq_decode_gemv_grouped: the five-launch chain), timed beside the per-channel engines of the same run ("w4a8_g128" ...,
"x_perchannel5" = its single-engine rate over the per-channel five-launch one); with --trace: the grouped W4A8 model instead."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _model(dev, wbits, max_pos, group_size=None):
    import mobilequant_amd as mq
    from mobilequant_amd.calibration import get_act_range
    from mobilequant_amd.llama import LlamaForCausalLM, LlamaShape
    shape = LlamaShape.tinyllama(max_pos=max_pos)
    model = LlamaForCausalLM(shape)
    model.reset_parameters(seed=1337)
    model = model.to(dev).eval().requires_grad_(False)
    g = torch.Generator().manual_seed(1337)
    act = get_act_range(model, [torch.randint(3, shape.vocab, (1, 256), generator=g) for _ in range(2)])
    mq.create_sim_qmodel(model, mq.QuantConfig(bitwidth=wbits, is_per_channel=wbits != 8 or group_size is not None, group_size=group_size or -1),
                         mq.QuantConfig(bitwidth=8))
    for name, mod in model.named_modules():               # ptq/mobilequant.py:175-201
        if isinstance(mod, mq.QLinear):
            if "w2" in name:
                mod.weight_quantizer.qcfg.is_per_channel = True
                mod.output_quantizer.qcfg.bitwidth = 16
            elif "o_proj" in name:
                mod.output_quantizer.qcfg.bitwidth = 16
        elif isinstance(mod, (mq.QRMSNorm, mq.QLayerNorm)):
            mod.input_quantizer.qcfg.bitwidth = 16
            mod.weight_quantizer.qcfg.bitwidth = 16
            mod.weight_quantizer.qcfg.is_symmetric = False
            mod.weight_quantizer.qcfg.is_per_channel = False
        elif isinstance(mod, mq.QMatMul):
            if "qk_bmm" in name:
                mod.output_quantizer.qcfg.bitwidth = 16
            if "pv_bmm" in name:
                mod.input_quantizer.qcfg.bitwidth = 16
    mq.set_scale_and_offset(model, act, "buffer")
    return model, shape


def _time(replay, set_pos, steps):
    best = float("inf")
    for _ in range(3):
        set_pos()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            replay()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / steps)
    return best                                            # ms per step


def run(wbits, contexts, batches, steps, dev, trace=False, group_size=None):
    from mobilequant_amd.decode import DecodeEngine
    from mobilequant_amd.decode_batch import BatchDecodeEngine
    cache_len = max(contexts) + steps + 16
    cache_len = (cache_len + 15) // 16 * 16
    model, shape = _model(dev, wbits, max(2048, cache_len), group_size)
    # per-group weight grids: the five-launch chain only
    singles = {} if trace else {L: DecodeEngine(model, cache_len=cache_len, launches=L) for L in ((5,) if group_size else (4, 5))}
    batched = {B: BatchDecodeEngine(model, B, cache_len=cache_len) for B in batches}
    for p in model.parameters():                            # the float weights of the decoder layers are no longer needed
        if p.dim() == 2 and p.shape[0] != shape.vocab:
            p.data = torch.empty(0, device=dev)
    torch.cuda.empty_cache()
    out = {}
    for L, eng in singles.items():
        eng.fill_cache_random(max(contexts))
        eng.tok.fill_(17)
        eng.capture()
        for ctx in contexts:
            def replay(ctx=ctx, eng=eng):
                (eng.graph_long if eng.graph_long is not None and ctx >= eng._long_threshold() else eng.graph).replay()
            ms = _time(replay, lambda: eng.set_position(ctx), steps)
            out[f"single_{L}launch_ctx{ctx}"] = {"ms_per_step": round(ms, 4), "tok_s": round(1000.0 / ms, 1)}
    for B, be in batched.items():
        for b in range(B):
            be.fill_cache_random(b, max(contexts), seed=b)
        be.tok.fill_(17)
        be.capture()
        for ctx in contexts:
            def set_pos(ctx=ctx, be=be):
                for b in range(be.batch):
                    be.set_position(b, ctx)
            if trace:
                set_pos()
                for _ in range(steps):
                    be.graph.replay()
                torch.cuda.synchronize()
                continue
            ms = _time(be.graph.replay, set_pos, steps)
            out[f"batch{B}_ctx{ctx}"] = {"ms_per_step": round(ms, 4), "tok_s": round(1000.0 * B / ms, 1),
                                         "tok_s_per_seq": round(1000.0 / ms, 1)}
    if not trace:
        for ctx in contexts:
            base = out[f"single_{5 if group_size else 4}launch_ctx{ctx}"]["tok_s"]
            for B in batches:
                out[f"batch{B}_ctx{ctx}"]["x_single5" if group_size else "x_single4"] = round(out[f"batch{B}_ctx{ctx}"]["tok_s"] / base, 3)
            if 1 in batches:
                out[f"batch1_ctx{ctx}"]["x_single5"] = round(out[f"batch1_ctx{ctx}"]["tok_s"] / out[f"single_5launch_ctx{ctx}"]["tok_s"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--contexts", default="256,2048")
    ap.add_argument("--batches", default="1,2,4,8")
    ap.add_argument("--wbits", default="8,4")
    ap.add_argument("--group-size", type=int, default=None, help="also time models with per-group weight grids of this many input channels")
    ap.add_argument("--trace", action="store_true", help="replays only (B = 1 and 8, 256 positions, W8A8) for a kernel trace")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_decode_batch needs the GPU"
    dev = torch.device("cuda:0")
    if a.trace:
        run(4 if a.group_size else 8, [256], [1, 8], 16, dev, trace=True, group_size=a.group_size)
        print(json.dumps({"metric": "decode_batch_trace", "done": True}))
        return
    contexts = [int(c) for c in a.contexts.split(",")]
    batches = [int(b) for b in a.batches.split(",")]
    res = {"metric": "decode_batch_tinyllama", "steps": a.steps, "unit": "tok/s aggregate (tok_s) and per sequence (tok_s_per_seq)"}
    for wb in (int(w) for w in a.wbits.split(",")):
        tag = "w8a8" if wb == 8 else "w4a8"
        res[tag] = run(wb, contexts, batches, a.steps, dev)
        torch.cuda.empty_cache()
        if a.group_size:
            g = res[f"{tag}_g{a.group_size}"] = run(wb, contexts, batches, a.steps, dev, group_size=a.group_size)
            for ctx in contexts:
                g[f"single_5launch_ctx{ctx}"]["x_perchannel5"] = round(g[f"single_5launch_ctx{ctx}"]["tok_s"] /
                                                                       res[tag][f"single_5launch_ctx{ctx}"]["tok_s"], 3)
            torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
