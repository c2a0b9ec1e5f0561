"""prefill(append=True) against extend() on one device, in one process.

TinyLlama-1.1B shape (W8A8, the mixed-precision rules of bench.py's decode model, fused through fuse_decoder_layer), cache_len 4096,
a live sequence of P = 1024 random cached positions; N = 64 / 128 / 512 / 2048 tokens are appended both ways.  extend() is the
yardstick: N / max_rows dependent multi-token steps, each streaming all weights.  HIP events around the whole call, one warm-up call
per variant and size (graphs of the row steps recorded, image caches allocated, kernels loaded), best and median of --reps.  The
import launch is timed alone too: bytes per second (it reads 2 bytes per cached element and writes 2 + the derived images) and its
share of the append.  Prints one JSON line.

    python tools/bench_append.py [--layers 22] [--reps 5] [--sizes 64,128,512,2048] [--small 8,16,24,32,48]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build(dev, layers, cache_len):
    import mobilequant_amd as mq
    from mobilequant_amd import llama
    from mobilequant_amd.calibration import get_act_range
    from mobilequant_amd.decode import DecodeEngine
    from mobilequant_amd.llama import LlamaForCausalLM, LlamaShape
    shape = LlamaShape.tinyllama(layers=layers, max_pos=cache_len)
    model = LlamaForCausalLM(shape)
    model.reset_parameters(seed=1337)
    model = model.to(dev).eval().requires_grad_(False)
    g = torch.Generator().manual_seed(1337)
    act = get_act_range(model, [torch.randint(3, shape.vocab, (1, 256), generator=g) for _ in range(2)])
    a8 = mq.QuantConfig(bitwidth=8)
    mq.create_sim_qmodel(model, mq.QuantConfig(bitwidth=8), a8)
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
    eng = DecodeEngine(model, cache_len=cache_len)
    assert llama.fuse_decoder_layer(model) == layers
    return model, eng


def timed(fn, reset, reps):
    out = []
    for i in range(reps + 1):                              # the first call is the warm-up
        reset()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i:
            out.append(e0.elapsed_time(e1))
    return {"best_ms": round(min(out), 4), "median_ms": round(statistics.median(out), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=22)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--position", type=int, default=1024)
    ap.add_argument("--cache-len", type=int, default=4096)
    ap.add_argument("--sizes", default="64,128,512,2048")
    ap.add_argument("--small", default="8,16,24,32,48", help="sizes for the APPEND_MIN_TOKENS crossover")
    a = ap.parse_args()
    from mobilequant_amd import ops
    from mobilequant_amd.decode import DecodeEngine
    dev = torch.device("cuda:0")
    model, eng = build(dev, a.layers, a.cache_len)
    P = a.position
    eng.fill_cache_random(P)
    eng.capture()
    ids = torch.randint(3, model.shape.vocab, (a.cache_len,), generator=torch.Generator().manual_seed(2)).tolist()
    res = {"shape": "tinyllama", "layers": a.layers, "cache_len": a.cache_len, "position": P, "launches": eng.launches, "max_rows": eng.max_rows,
           "sizes": {}, "small": {}}
    keep = DecodeEngine.APPEND_MIN_TOKENS
    try:
        DecodeEngine.APPEND_MIN_TOKENS = 2                 # time the fused path at every size, whatever the threshold says
        for group, sizes in (("sizes", a.sizes), ("small", a.small)):
            for n in [int(v) for v in sizes.split(",") if v]:
                if P + n > a.cache_len:
                    continue
                ext = timed(lambda: eng.extend(ids[:n]), lambda: eng.set_position(P), a.reps)
                app = timed(lambda: eng.prefill(ids[:n], append=True), lambda: eng.set_position(P), a.reps)
                assert eng.append_stats["prefilled"] == n, eng.append_stats
                res[group][n] = {"extend": ext, "append": app, "speedup_best": round(ext["best_ms"] / app["best_ms"], 3)}
    finally:
        DecodeEngine.APPEND_MIN_TOKENS = keep
    # the import launch alone, one layer, P positions
    s = model.shape
    qk = model.layers[0].self_attn.qk_bmm
    grids = {k: (q.scale.detach(), q.offset.detach(), q.qmin, q.qmax) for k, q in (("qk_a", qk.input_quantizer), ("qk_b", qk.input2_quantizer))}
    img = eng._append_images[0].per_sequence[0]
    imp = timed(lambda: [ops.attention_cache_import(img, eng.k_cache[0], eng.v_cache[0], P, grids, v_chunked=eng.v_transposed, k_f16_exact=True)
                         for _ in range(20)], lambda: None, a.reps)
    elems = s.kv_heads * P * s.head_dim
    bytes_moved = elems * (2 + 2 + (2 if s.head_dim == 64 else 0)) + s.kv_heads * P * 4
    us = imp["best_ms"] * 1e3 / 20
    res["import"] = {"us_per_launch_back_to_back": round(us, 3), "bytes": bytes_moved, "TB_per_s": round(bytes_moved / us * 1e-6, 4),
                     "ms_per_append_all_layers": round(us * a.layers * 1e-3, 4)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
