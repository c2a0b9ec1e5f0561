#!/usr/bin/env python3
"""Time of GPTQ rounding: gptq_round (mq_gptq_round) beside what a user has without it.

Per shape, 4-bit asymmetric grid with groups of 128, Student-t(4) * 0.02 weights, the Hessian of synthetic correlated heavy-tailed
inputs (4096 tokens), with and without activation order:
  (a) gptq.gptq_round: the transposes, one kernel that walks all K columns, the transposes back;
  (b) the same blocked algorithm in torch, written here: a per-column loop on the device (quantize, error, rank-1 update of the rest of a
      128-column block) with one GEMM per block for the trailing columns -- K dependent steps of several launches each.
HIP events, warmed, median of --repeats (--loop-repeats) runs per window, two windows with (a) and (b) in turn, the lower median.  Also: the one-off gptq_factor time (host clock around a synchronise),
the layer objective tr(dW H dW^T) of (a) and (b) relative to round-to-nearest, and the share of indices (a) and (b) agree on ((b) rounds
its rank-1 updates differently: not bit-equal).  One JSON line per measurement; exit status 1 if (a) is not faster everywhere.

    python tools/bench_gptq.py [--repeats 5] [--loop-repeats 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mobilequant_amd import _lib, gptq, ops  # noqa: E402

SHAPES = ((2048, 2048), (5632, 2048), (2048, 5632))          # (N, K): q/o_proj, w1/w3 and w2 of TinyLlama
GROUP = 128
LOOP_BLOCK = 128
TOKENS = 4096


def timed(fn, repeats):
    """Median of `repeats` runs between two HIP events: milliseconds, the last result."""
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out), min(out), res


def make_inputs(n, k, dev):
    rng = np.random.default_rng(n + 3 * k)
    w = torch.from_numpy((rng.standard_t(4, size=(n, k)) * 0.02).astype(np.float32)).to(dev)
    gen = torch.Generator(device=dev).manual_seed(n + k)
    z = torch.randn((TOKENS, k), device=dev, generator=gen) * torch.rand((TOKENS, 1), device=dev, generator=gen).add_(0.2).reciprocal_().sqrt_()
    x = z + 0.6 * torch.roll(z, 1, 1) + 0.35 * torch.roll(z, 2, 1) + 0.2 * torch.roll(z, 5, 1)
    x = x * torch.exp(torch.rand((1, k), device=dev, generator=gen) * 4.6 - 2.3)          # channel scales two decades wide
    H = torch.zeros((k, k), device=dev)
    H.addmm_(x.t(), x)
    H *= 2.0 / TOKENS
    rows = w.reshape(-1, GROUP)
    mn, mx = ops.minmax_rows(rows)
    scale, offset = ops.scale_offset_from_minmax(mn, mx, 4, False)
    return w, H, scale.reshape(n, -1).contiguous(), offset.reshape(n, -1).contiguous()


def torch_loop(w, scale, offset, qmin, qmax, U, perm):
    """Blocked GPTQ in torch on the device (the structure of AutoGPTQ's fasterquant, static groups): returns (index uint8, w_deq)."""
    n, k = w.shape
    W = w.clone() if perm is None else w[:, perm.long()].contiguous()
    S = scale.repeat_interleave(GROUP, 1)
    O = offset.repeat_interleave(GROUP, 1)
    if perm is not None:
        S, O = S[:, perm.long()].contiguous(), O[:, perm.long()].contiguous()
    Q = torch.empty_like(W)
    I = torch.empty_like(W)
    for i1 in range(0, k, LOOP_BLOCK):
        i2 = min(i1 + LOOP_BLOCK, k)
        W1 = W[:, i1:i2].clone()
        E1 = torch.empty_like(W1)
        U1 = U[i1:i2, i1:i2]
        for i in range(i2 - i1):
            col = W1[:, i]
            s, o = S[:, i1 + i], O[:, i1 + i]
            q = torch.clamp(torch.round(col / s) + o, qmin, qmax)
            dq = (q - o) * s
            err = (col - dq) / U1[i, i]
            W1[:, i:] -= err.unsqueeze(1) * U1[i, i:].unsqueeze(0)
            E1[:, i] = err
            Q[:, i1 + i] = dq
            I[:, i1 + i] = q
        if i2 < k:
            W[:, i2:] -= E1 @ U[i1:i2, i2:]
    if perm is not None:
        inv = torch.empty_like(perm, dtype=torch.long)
        inv[perm.long()] = torch.arange(k, device=w.device)
        Q, I = Q[:, inv], I[:, inv]
    return (I - qmin).to(torch.uint8), Q


def objective(dq, w, H64):
    d = (dq - w).double()
    return float(((d @ H64) * d).sum())


def bench_shape(n, k, act_order, repeats, loop_repeats, dev):
    w, H, scale, offset = make_inputs(n, k, dev)
    qmin, qmax = 0, 15
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    U, perm, dead = gptq.gptq_factor(H, 0.01, act_order)
    torch.cuda.synchronize()
    factor_ms = (time.perf_counter() - t0) * 1e3
    assert not bool(dead.any())

    def kernel():
        return gptq.gptq_round(w, scale, offset, qmin, qmax, U, GROUP, perm)

    def loop():
        return torch_loop(w, scale, offset, qmin, qmax, U, perm)
    kernel()
    loop()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(2):                                    # in turn, so that drift of the box hits both alike
        med, best, res = timed(kernel, repeats)
        ta.append((med, best))
        med, best, (idx_b, dq_b) = timed(loop, loop_repeats)
        tb.append((med, best))
    t_a, t_b = min(m for m, _ in ta), min(m for m, _ in tb)
    H64 = H.double()
    rtn = ops.fake_quant(w.reshape(-1, GROUP), scale.reshape(-1), offset.reshape(-1), qmin, qmax).view(n, k)
    base = objective(rtn, w, H64)
    out = {"weight": f"{n}x{k}", "group_size": GROUP, "act_order": act_order, "kernel_ms": round(t_a, 3), "kernel_best_ms": round(min(b for _, b in ta), 3),
           "loop_ms": round(t_b, 1), "loop_over_kernel": round(t_b / t_a, 1), "factor_ms": round(factor_ms, 1),
           "fma_per_s": float(f"{n * k * (k - 1) / 2 / (t_a * 1e-3):.4g}"),
           "objective_over_rtn": round(objective(res.dequantized, w, H64) / base, 4), "loop_objective_over_rtn": round(objective(dq_b, w, H64) / base, 4),
           "indices_same_as_loop": round(float((res.index == idx_b).double().mean()), 4)}
    print(json.dumps(out), flush=True)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--loop-repeats", type=int, default=5)
    a = p.parse_args()
    assert torch.cuda.is_available(), "bench_gptq.py measures on the GPU only"
    dev = torch.device("cuda:0")
    info = _lib.device_info()
    print(json.dumps({"device": info["arch"], "cu_count": info["cu_count"], "max_clock_mhz": info["max_clock_khz"] // 1000}), flush=True)
    res = [bench_shape(n, k, ao, a.repeats, a.loop_repeats, dev) for n, k in SHAPES for ao in (False, True)]
    slower = [r["weight"] + (" act_order" if r["act_order"] else "") for r in res if r["kernel_ms"] >= r["loop_ms"]]
    print(json.dumps({"kernel_faster_everywhere": not slower, "slower_at": slower}), flush=True)
    return 1 if slower else 0


if __name__ == "__main__":
    sys.exit(main())
