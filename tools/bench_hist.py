#!/usr/bin/env python3
"""Cost of the one-pass histogram beside the min / max pass it sits next to.

Per tensor: mq_hist_minmax_tensor and mq_minmax_tensor on the same box and the same tensors, WARM (one tensor re-read: it sits in the
caches) and COLD (a ring of copies larger than the Infinity Cache, each read once per replay); hipGraphs of >= 20 launches, the two
kernels timed alternately, best and median of the repeats.  The all-equal tensor is the contention worst case (every LDS atomic of a
wave on one address); it and the Gaussian case are also timed with the wave-uniform aggregation switched off
(mq_hist_set_aggregate(0)).  One JSON line per tensor.

Calibration: samples/s of get_act_range(method="percentile") beside method="minmax" with the fused statistics passes switched off (the
like-for-like comparison: what the histogram adds to a hook), on the stub-GEMM calibration model of bench.py's calibration leg.

    python tools/bench_hist.py [--layers 4] [--samples 6] [--seq 2048] [--mantissa-bits 5] [--skip-calibration]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from mobilequant_amd import _lib, ops  # noqa: E402

RING_BYTES = 768 << 20              # > 256 MB Infinity Cache + 8 x 4 MB L2


def graph_of(fns):
    """One hipGraph that runs every fn once; returns a callable giving microseconds per launch of one replay."""
    for f in fns[:2]:
        f()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for f in fns:
            f()
    g.replay()
    torch.cuda.synchronize()

    def once():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / len(fns)
    return once


def alternate(timers, repeats=7):
    """{name: (best, median)} with the candidates timed in turn, so that drift of the box hits all alike."""
    runs = {k: [] for k in timers}
    for _ in range(repeats):
        for k, t in timers.items():
            runs[k].append(t())
    return {k: (min(v), statistics.median(v)) for k, v in runs.items()}


def bench_tensor(name, make, shape, m, dev, ab):
    lib = _lib.load()
    x = make(shape)
    nbytes = x.numel() * x.element_size()
    n_ring = max(2, -(-RING_BYTES // nbytes))
    ring = [x] + [x.clone() for _ in range(n_ring - 1)]
    counts, nan = ops.hist_new(1, m, dev)
    mn, mx = ops.minmax_new(1, dev)
    mn2, mx2 = ops.minmax_new(1, dev)

    def hist(t):
        return lambda: ops.hist_minmax_tensor_(t, counts[0], nan, mn, mx, m)

    def mm(t):
        return lambda: ops.minmax_tensor_(t, mn2, mx2)
    reps = max(20, n_ring)
    cold = [ring[i % n_ring] for i in range(reps)]
    timers = {"hist_warm": graph_of([hist(x)] * 20), "minmax_warm": graph_of([mm(x)] * 20),
              "hist_cold": graph_of([hist(t) for t in cold]), "minmax_cold": graph_of([mm(t) for t in cold])}
    if ab:
        lib.mq_hist_set_aggregate(0)                        # (the kernel variant is chosen at capture time)
        try:
            timers["hist_noagg_warm"] = graph_of([hist(x)] * 20)
            timers["hist_noagg_cold"] = graph_of([hist(t) for t in cold])
        finally:
            lib.mq_hist_set_aggregate(1)
    res = alternate(timers)
    torch.cuda.synchronize()
    assert int(counts.sum()) + int(nan.sum()) > 0 and float(mn) == float(mn2) and float(mx) == float(mx2)
    out = {"tensor": name, "shape": list(shape), "dtype": str(x.dtype).replace("torch.", ""), "bytes": nbytes, "mantissa_bits": m, "ring": n_ring}
    for k, (best, med) in res.items():
        out[k + "_us"] = round(best, 2)
        out[k + "_median_us"] = round(med, 2)
        out[k + "_TBps"] = round(nbytes / best / 1e6, 2)
    for temp in ("warm", "cold"):
        out[f"ratio_{temp}"] = round(res[f"hist_{temp}"][0] / res[f"minmax_{temp}"][0], 2)
    print(json.dumps(out), flush=True)
    return out


def bench_calibration(layers, n_samples, seq, m, dev):
    import bench
    from mobilequant_amd.calibration import ActRangeCollector, get_act_range
    from mobilequant_amd.llama import LlamaForCausalLM, LlamaShape
    shape = LlamaShape.tinyllama(layers=layers, max_pos=seq)
    model = LlamaForCausalLM(shape)
    model.reset_parameters(seed=1337)
    model = model.to(dev).eval()
    bench._stub_gemms(model)
    g = torch.Generator().manual_seed(1337)
    samples = [torch.randint(3, shape.vocab, (1, seq), generator=g).to(dev) for _ in range(n_samples)]
    fused = (ActRangeCollector.fuse_layer_statistics, ActRangeCollector.fuse_attention_statistics)
    modes = {"minmax_unfused": dict(), "percentile": dict(method="percentile", percentile=0.999, mantissa_bits=m), "minmax_fused": dict()}
    runs = {k: [] for k in modes}
    try:
        for rep in range(3):                                # the first round is the warm-up
            for k, kw in modes.items():
                ActRangeCollector.fuse_layer_statistics = ActRangeCollector.fuse_attention_statistics = (k == "minmax_fused")
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                act = get_act_range(model, samples, **kw)   # (act_dict()'s readback ends the device work)
                torch.cuda.synchronize()
                if rep:
                    runs[k].append(n_samples / (time.perf_counter() - t0))
                assert len(act) > 10 * layers
    finally:
        ActRangeCollector.fuse_layer_statistics, ActRangeCollector.fuse_attention_statistics = fused
    out = {"calibration": f"TinyLlama-shaped, {layers} layers, S={seq}, stub GEMMs, {n_samples} samples", "mantissa_bits": m}
    for k, v in runs.items():
        out[k + "_samples_per_s"] = round(max(v), 2)
    out["percentile_over_minmax_unfused"] = round(max(runs["minmax_unfused"]) / max(runs["percentile"]), 2)
    print(json.dumps(out), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--layers", type=int, default=4)
    p.add_argument("--samples", type=int, default=6)
    p.add_argument("--seq", type=int, default=2048)
    p.add_argument("--mantissa-bits", type=int, default=5)
    p.add_argument("--skip-calibration", action="store_true")
    a = p.parse_args()
    assert torch.cuda.is_available(), "bench_hist.py measures on the GPU only"
    dev = torch.device("cuda:0")
    info = _lib.device_info()
    print(json.dumps({"device": info["arch"], "cu_count": info["cu_count"], "max_clock_mhz": info["max_clock_khz"] // 1000}), flush=True)
    torch.manual_seed(0)
    normal = lambda s: torch.randn(*s, device=dev)                               # noqa: E731
    m = a.mantissa_bits
    bench_tensor("N(0,1)", normal, (2048, 2048), m, dev, ab=False)
    bench_tensor("N(0,1)", normal, (2048, 5632), m, dev, ab=True)
    bench_tensor("N(0,1)", normal, (32, 2048, 2048), m, dev, ab=False)
    bench_tensor("all equal", lambda s: torch.full(s, 0.75, device=dev), (2048, 5632), m, dev, ab=True)
    bench_tensor("N(0,1) fp16", lambda s: torch.randn(*s, device=dev).half(), (2048, 5632), m, dev, ab=False)
    if m != 6:
        bench_tensor("N(0,1)", normal, (2048, 5632), 6, dev, ab=False)          # 128 KiB of LDS: one workgroup per CU
    if not a.skip_calibration:
        torch.cuda.empty_cache()
        bench_calibration(a.layers, a.samples, a.seq, m, dev)


if __name__ == "__main__":
    main()
