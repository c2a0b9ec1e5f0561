#!/usr/bin/env python3
"""Time of the clip search: mq_lwc_search beside the only way to run the same search without it.

Per shape, 4-bit asymmetric grid, 64 joint candidates (lwc_factor_table), Student-t(4) * 0.02 weights:
  (a) ops.lwc_search: one launch, the weight read once;
  (b) a loop over the candidates of ops.lwc_fake_quant (one pass writing Q(w)) plus a torch fp64 reduction of (Q(w) - w)^2 per row and
      the running strict-< selection -- the per-row [rows] sigmoid vectors of every candidate are built before the clock starts.
HIP events around 50 searches (a) / one whole loop (b), warmed, best of several windows, (a) and (b) in turn.  Both must choose the same
candidates (rows whose two best costs lie within the summation tolerance aside).  One JSON line per shape: times, ratio, (a)'s rate in element-candidates per
second, rows clipped and the reduction of sum (Q(w) - w)^2 against candidate 0 -- on these synthetic weights, not a model.

    python tools/bench_lwc_search.py [--candidates 64] [--repeats 5]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mobilequant_amd import _lib, lwc_factor_table, ops  # noqa: E402

SEARCH_CALLS_PER_WINDOW = 50      # (a) is a fraction of a millisecond: a window holds 50 launches; (b) is milliseconds, 64 x several launches
# (N, K, group_size): per-channel weights of a TinyLlama layer and a 16384-row one; the 5632 x 2048 weight per group
SHAPES = ((2048, 2048, -1), (5632, 2048, -1), (2048, 5632, -1), (16384, 2048, -1), (5632, 2048, 128), (5632, 2048, 64))


def timed(fn, repeats, inner=1):
    """Best of `repeats` windows of `inner` back-to-back calls between two HIP events: milliseconds per call, the last result."""
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            res = fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / inner)
    return min(out), res


def bench_shape(n, k, g, n_cand, repeats, dev):
    rng = np.random.default_rng(n + k + max(g, 0))
    w = torch.from_numpy((rng.standard_t(4, size=(n, k)) * 0.02).astype(np.float32)).to(dev)
    x = w.reshape(-1, g).contiguous() if g != -1 else w
    rows, cols = x.shape
    sig = torch.sigmoid(lwc_factor_table(n_cand).to(dev))
    per_row = [sig[c].expand(rows).contiguous() for c in range(n_cand)]

    def search():
        return ops.lwc_search(x, sig, sig, 4, False)

    def loop():
        best = base = idx = None
        for c in range(n_cand):
            y = ops.lwc_fake_quant(x, per_row[c], per_row[c], 4, False)[0]
            cost = (y - x).double().square_().sum(1)
            if c == 0:
                best, base, idx = cost, cost, torch.zeros(rows, dtype=torch.int32, device=dev)
            else:
                win = cost < best
                best, idx = torch.where(win, cost, best), torch.where(win, torch.full_like(idx, c), idx)
        return idx, best, base
    search()
    loop()
    torch.cuda.synchronize()
    t_a = t_b = float("inf")
    for _ in range(2):                                   # in turn, so that drift of the box hits both alike
        ta, (idx, best, base) = timed(search, repeats, inner=SEARCH_CALLS_PER_WINDOW)
        tb, (idx_b, best_b, base_b) = timed(loop, max(2, repeats // 2))
        t_a, t_b = min(t_a, ta), min(t_b, tb)
    same = float((idx == idx_b).double().mean())
    assert same > 0.999 and torch.allclose(best, best_b, rtol=1e-9, atol=0) and torch.allclose(base, base_b, rtol=1e-9, atol=0), same
    out = {"weight": f"{n}x{k}", "group_size": g, "rows": rows, "cols": cols, "candidates": n_cand, "search_ms": round(t_a, 3),
           "loop_ms": round(t_b, 3), "loop_over_search": round(t_b / t_a, 1),
           "element_candidates_per_s": float(f"{rows * cols * n_cand / (t_a * 1e-3):.4g}"), "rows_same_choice": round(same, 6),
           "rows_clipped": round(float((idx != 0).double().mean()), 4),
           "error_reduction": round(1.0 - float(best.sum()) / float(base.sum()), 4)}
    print(json.dumps(out), flush=True)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--candidates", type=int, default=64)
    p.add_argument("--repeats", type=int, default=5)
    a = p.parse_args()
    assert torch.cuda.is_available(), "bench_lwc_search.py measures on the GPU only"
    dev = torch.device("cuda:0")
    info = _lib.device_info()
    print(json.dumps({"device": info["arch"], "cu_count": info["cu_count"], "max_clock_mhz": info["max_clock_khz"] // 1000}), flush=True)
    res = [bench_shape(n, k, g, a.candidates, a.repeats, dev) for n, k, g in SHAPES]
    slower = [r["weight"] + (f" g{r['group_size']}" if r["group_size"] != -1 else "") for r in res if r["search_ms"] >= r["loop_ms"]]
    print(json.dumps({"search_faster_everywhere": not slower, "slower_at": slower}), flush=True)
    return 1 if slower else 0


if __name__ == "__main__":
    sys.exit(main())
