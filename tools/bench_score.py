"""Token scoring throughput: the fused lm_head log-softmax (ops.score_head) against the path it replaces.

    python tools/bench_score.py [--vocabs 32000,100352,256000] [--rows 2048] [--hidden 2048] [--iters 20] [--e2e] [--trace]

Head (M = rows, K = hidden, per vocabulary): HIP events around `iters` warmed calls, best of 3, for
  fused      ops.score_head(y, W, None, targets)
  replaced   F.linear + log_softmax + gather + argmax (what scoring by hand does)
  linear     F.linear alone
with TFLOP/s (2 M K V per call) and the share of the 157.3 TF fp32 matrix peak, and the allocator's peak growth per call.
--e2e: tokens scored per second on a TinyLlama-shaped 22-layer W8A8 model with fused decoder layers, 8 x 2 048 positions:
scoring.token_logprobs against model(ids) followed by torch log_softmax / gather / argmax.
--trace: one fused call per vocabulary and nothing else, for `rocprofv3 --kernel-trace --stats`.
Prints ONE JSON line."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_TF = 157.3


def _time(fn, iters):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1) / iters)
    return best


def _peak(fn, dev):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated(dev) - base


def _replaced(y, w, t):
    logits = F.linear(y, w)
    lp = torch.log_softmax(logits, -1)
    return lp.gather(1, t[:, None])[:, 0], logits.argmax(-1)


def bench_head(dev, vocabs, M, K, iters, trace):
    from mobilequant_amd import ops
    out = {}
    g = torch.Generator(device=dev).manual_seed(0)
    y = torch.randn(M, K, device=dev, generator=g)
    for V in vocabs:
        w = torch.randn(V, K, device=dev, generator=g) * (3.0 / K ** 0.5)
        t = torch.randint(0, V, (M,), device=dev, generator=g)
        fused = lambda: ops.score_head(y, w, None, t)          # noqa: E731
        if trace:
            fused()
            torch.cuda.synchronize()
            continue
        flop = 2.0 * M * K * V
        r = {}
        for name, fn in (("fused", fused), ("replaced", lambda: _replaced(y, w, t)), ("linear", lambda: F.linear(y, w))):
            ms = _time(fn, iters)
            r[name] = dict(ms=round(ms, 4), tflops=round(flop / ms / 1e9, 1), peak_share=round(flop / ms / 1e9 / PEAK_TF, 3),
                           peak_extra_mib=round(_peak(fn, dev) / 2 ** 20, 1))
        r["fused_vs_replaced"] = round(r["replaced"]["ms"] / r["fused"]["ms"], 3)
        r["fused_vs_linear"] = round(r["linear"]["ms"] / r["fused"]["ms"], 3)
        out[str(V)] = r
        del w
    return out


def bench_e2e(dev, iters):
    from mobilequant_amd import llama, scoring
    from tools.bench_decode_batch import _model
    m, shape = _model(dev, 8, 2048)
    assert llama.fuse_decoder_layer(m) == shape.layers
    g = torch.Generator().manual_seed(2)
    ids = torch.randint(0, shape.vocab, (8, 2048), generator=g).to(dev)
    tg = torch.cat([ids[:, 1:], torch.full_like(ids[:, :1], -1)], 1)

    def by_hand():
        with torch.no_grad():
            lp = torch.log_softmax(m(ids), -1)
            return lp[:, :-1].gather(2, ids[:, 1:, None]), lp.argmax(-1)
    n_tok = 8 * 2047
    res = {}
    for name, fn in (("token_logprobs", lambda: scoring.token_logprobs(m, ids, tg)), ("forward_log_softmax", by_hand)):
        ms = _time(fn, iters)
        res[name] = dict(ms=round(ms, 3), tokens_per_s=round(n_tok / ms * 1e3), peak_extra_mib=round(_peak(fn, dev) / 2 ** 20, 1))
    res["speedup"] = round(res["forward_log_softmax"]["ms"] / res["token_logprobs"]["ms"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vocabs", default="32000,100352,256000")
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--hidden", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    vocabs = [int(v) for v in a.vocabs.split(",")]
    res = dict(M=a.rows, K=a.hidden, head=bench_head(dev, vocabs, a.rows, a.hidden, a.iters, a.trace))
    if a.e2e and not a.trace:
        res["e2e_tinyllama_w8a8_fused_8x2048"] = bench_e2e(dev, max(2, a.iters // 5))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
