#!/usr/bin/env python3
"""Time of the W4A16 linear: mq_w4a16_linear beside torch.nn.functional.linear on the dense fp16 w16 of the same layer --
what a user without the kernel would run.

Shapes: (N, K) = (5632, 2048), (2048, 5632), (2048, 2048), group_size 128, fp16 activations.
  decode   M = 1 and M = 8: microseconds per launch and effective weight GB/s (packed bytes + scales + zeros over the time; the dense
           linear's GB/s counts ITS bytes, 2 N K);
  prefill  M = 2048: microseconds and TFLOP/s (2 M N K over the time).
Method: per (shape, M) a hipGraph of `inner` back-to-back launches is captured for each side and replayed `repeats` times between two
HIP events, after a warm-up replay; the figure is the MEDIAN window over `inner`.  Host launch cost is therefore outside the figure (a
decode launch is shorter than its Python call).  `rotating`: launch i reads copy i of the weights, copies enough to exceed 512 MiB, so
every launch streams from HBM as a decode step's does; `resident`: one copy, L2 / Infinity Cache warm.  The two sides alternate.  The
shader clock is not pinned: the sclk rocm-smi reports before and after is printed (read only).  Results are checked against each other
before timing (same w16, fp32 against fp16-output accumulation: within 2^-8 relative to sum |x w|).

    python tools/bench_w4a16.py [--repeats 30] [--inner 64]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import mobilequant_amd.quantization.qmodule as Q  # noqa: E402
from mobilequant_amd import _lib, weight_only  # noqa: E402

SHAPES = ((5632, 2048), (2048, 5632), (2048, 2048))
GROUP = 128
ROTATE_BYTES = 512 << 20


def sclk():
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "--json"], capture_output=True, text=True, timeout=10)
        d = json.loads(r.stdout)
        return sorted({v.get("sclk clock speed:", "?") for v in d.values() if isinstance(v, dict)})
    except Exception as e:      # noqa: BLE001  (the clock is a note beside the figures, not a condition of them)
        return f"not read ({type(e).__name__})"


def graph_time(fn, n_copies, inner, repeats):
    """Median microseconds per launch of fn(i % n_copies), `inner` launches per captured graph."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for i in range(min(inner, 2 * n_copies)):
            fn(i % n_copies)                             # warm-up outside the capture (code objects, LDS attribute, library algorithms)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(inner):
            fn(i % n_copies)
    g.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / inner)
    return out


def bench(N, K, M, inner, repeats, dev):
    rng = np.random.default_rng(N + K)
    w = torch.from_numpy((rng.standard_normal((N, K)) * 0.02).astype(np.float32)).to(dev)
    mn, mx = Q.compute_min_max_from_tensor(w, True, GROUP)
    s, o, *_ = Q.compute_scale_offset_from_min_max(mn, mx, 4, False)
    qw, sc, zp = weight_only.w4a16_pack(w, s, o, 4, False, GROUP)
    w16 = weight_only.w4a16_dequantize(qw, sc, zp, GROUP)
    x = torch.from_numpy(rng.standard_normal((M, K)).astype(np.float16)).to(dev)
    ours, dense = weight_only.w4a16_linear(x, qw, sc, zp, None, GROUP), F.linear(x, w16)
    tol = 2.0 ** -8 * (x.float().abs() @ w16.float().abs().T)
    assert bool(((ours.float() - dense.float()).abs() <= tol).all()), "the two sides disagree"
    packed_bytes = qw.numel() + 2 * sc.numel() + 2 * zp.numel()
    dense_bytes = 2 * N * K
    res = {"N": N, "K": K, "M": M, "group_size": GROUP, "kernel": {1: "gemv", 2: "gemm"}[weight_only.w4a16_variant(M, N, K, GROUP)]}
    for mode in ("rotating", "resident"):
        nq = max(1, -(-ROTATE_BYTES // packed_bytes)) if mode == "rotating" else 1
        nd = max(1, -(-ROTATE_BYTES // dense_bytes)) if mode == "rotating" else 1
        qws, scs, zps = qw.repeat(nq, 1, 1), sc.repeat(nq, 1, 1), zp.repeat(nq, 1, 1)
        w16s = w16.repeat(nd, 1, 1)
        t_o, t_d = [], []
        for _ in range(2):                               # in turn, so that drift of the box hits both alike
            t_o += graph_time(lambda i: weight_only.w4a16_linear(x, qws[i], scs[i], zps[i], None, GROUP), nq, inner, repeats)
            t_d += graph_time(lambda i: F.linear(x, w16s[i]), nd, inner, repeats)
        a, b = statistics.median(t_o), statistics.median(t_d)
        res[mode] = {"w4a16_us": round(a, 2), "dense_fp16_us": round(b, 2), "dense_over_w4a16": round(b / a, 2),
                     "w4a16_spread_us": [round(min(t_o), 2), round(max(t_o), 2)], "dense_spread_us": [round(min(t_d), 2), round(max(t_d), 2)]}
        if M <= 8:
            res[mode]["w4a16_weight_GBps"] = round(packed_bytes / a * 1e-3, 1)
            res[mode]["dense_weight_GBps"] = round(dense_bytes / b * 1e-3, 1)
        else:
            res[mode]["w4a16_TFLOPs"] = round(2.0 * M * N * K / a * 1e-6, 1)
            res[mode]["dense_TFLOPs"] = round(2.0 * M * N * K / b * 1e-6, 1)
        del qws, scs, zps, w16s
    print(json.dumps(res), flush=True)
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--repeats", type=int, default=30)
    p.add_argument("--inner", type=int, default=64)
    a = p.parse_args()
    assert torch.cuda.is_available(), "bench_w4a16.py measures on the GPU only"
    dev = torch.device("cuda:0")
    info = _lib.device_info()
    print(json.dumps({"device": info["arch"], "cu_count": info["cu_count"], "max_clock_mhz": info["max_clock_khz"] // 1000, "sclk_before": sclk()}),
          flush=True)
    res = []
    for N, K in SHAPES:
        for M in (1, 8):
            res.append(bench(N, K, M, a.inner, a.repeats, dev))
        res.append(bench(N, K, 2048, max(4, a.inner // 8), a.repeats, dev))
    behind = [f"M={r['M']} {r['N']}x{r['K']}" for r in res if r["rotating"]["dense_over_w4a16"] < 1.0]
    print(json.dumps({"sclk_after": sclk(), "w4a16_behind_dense_fp16_at": behind}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
