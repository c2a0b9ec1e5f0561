"""Forking a cached sequence into other slots (mq_decode_cache_fork): the launch and BatchDecodeEngine.fork() against the
slice-copy loop it replaces, and the time to the first new token of generate(n=8) against eight prefills, in one process.

    python tools/bench_fork.py [--calls 20] [--positions 256,2048] [--fans 1,3,7] [--no-generate]

copy: the TinyLlama-1.1B shape (22 layers, 4 KV heads of 64), batch 8; slot 0 holds `positions` cached positions of random bytes.  Per
  (positions, fan-out) HIP events around `calls` back-to-back eager calls, warmed, best of 3, microseconds per call (tools/bench_sample.py's
  protocol): `launch` -- ops.decode_cache_fork alone, over the engine's prebuilt pointer table (the eager call: its argument checks
  on the host included); `fork` -- BatchDecodeEngine.fork(), the launch plus the fork table's upload and the per-slot state copies;
  `slices` -- what a user could write before: per cache and per destination c[dst, :, :n] = c[src, :, :n] (44 x fan-out strided torch
  copies).  `kernel` -- the launch's time on the device: `calls` launches recorded into ONE hipGraph, events around its replay, so no
  host time between them counts.  gb_s = (bytes read once + bytes written) / kernel time for the launch, and (bytes read per copy +
  bytes written) / time for the loop, which reads the source once per destination.
generate: W8A8, one prompt of `positions` tokens, one new token, engine captured; wall clock around generate(), best of 3:
  `n8` -- generate([p], 1, sampling=..., n=8): one prefill and one fork; `repeat8` -- generate([p] * 8, 1, sampling=...): eight prefills.
Prints ONE JSON line."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_sample import _events, _wall  # noqa: E402

BATCH = 8


def copy_table(eng, positions, fans, calls):
    from mobilequant_amd import ops
    s = eng.shape
    caches = eng.k_cache + eng.v_cache
    out = {}
    for P in positions:
        for b in range(BATCH):
            eng.release(b)
        eng.fill_cache_random(0, P, seed=P)
        once = P * s.head_dim * s.kv_heads * len(caches)          # the source's live bytes, all caches
        for f in fans:
            dsts = list(range(1, 1 + f))
            parent = torch.tensor([0] * (1 + f) + list(range(1 + f, BATCH)), dtype=torch.int32).to(eng.dev)

            def launch():
                ops.decode_cache_fork(caches, eng.pos, parent, table=eng._fork_table)

            def fork():
                eng.fork({0: dsts})

            def slices():
                for c in caches:
                    for d in dsts:
                        c[d, :, :P] = c[0, :, :P]

            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(calls):
                    launch()

            for fn in (launch, fork, slices, g.replay):
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            l_us, f_us, s_us, k_us = _events(launch, calls), _events(fork, calls), _events(slices, calls), _events(g.replay, 1) / calls
            for d in dsts:                                         # (fork() made them active: the next cell starts from one live slot)
                eng.release(d)
            out[f"pos{P}_fan{f}"] = {"kernel_us": round(k_us, 2), "launch_us": round(l_us, 2), "fork_us": round(f_us, 2), "slices_us": round(s_us, 2),
                                     "kernel_gb_s": round((1 + f) * once / k_us / 1e3, 1), "slices_gb_s": round(2 * f * once / s_us / 1e3, 1),
                                     "bytes_written": f * once, "x_slices_launch": round(l_us / s_us, 4), "x_slices_fork": round(f_us / s_us, 4),
                                     "miss": bool(l_us >= s_us)}
    return out


def generate_table(eng, positions):
    from mobilequant_amd import SamplingParams
    sp = SamplingParams(temperature=0.7, top_k=40, top_p=0.9, seed=3)
    out = {}
    for P in positions:
        g = torch.Generator().manual_seed(P)
        prompt = torch.randint(3, eng.shape.vocab, (P,), generator=g).tolist()
        paths = {"n8": lambda: eng.generate([prompt], 1, sampling=sp, n=BATCH), "repeat8": lambda: eng.generate([prompt] * BATCH, 1, sampling=sp)}
        assert paths["n8"]()[0] == paths["repeat8"]()                  # warm-up, and the contract at the benchmark's own size
        cell = {name: round(1e3 * min(_wall(fn) for _ in range(3)), 3) for name, fn in paths.items()}
        out[f"pos{P}"] = {"n8_ms": cell["n8"], "repeat8_ms": cell["repeat8"], "x_repeat8": round(cell["n8"] / cell["repeat8"], 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--positions", default="256,2048")
    ap.add_argument("--fans", default="1,3,7")
    ap.add_argument("--no-generate", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fork.py needs an MI355X: there is no CPU path")
    from bench_decode_batch import _model
    from mobilequant_amd.decode_batch import BatchDecodeEngine
    dev = torch.device("cuda:0")
    positions, fans = [int(v) for v in a.positions.split(",")], [int(v) for v in a.fans.split(",")]
    if any(not 1 <= f < BATCH for f in fans):
        raise SystemExit(f"bench_fork.py: a fan-out outside 1..{BATCH - 1}")
    cache_len = (max(positions) + 1 + 31) // 16 * 16             # the longest prompt and its first new token
    model, _ = _model(dev, 8, max(2048, cache_len))
    eng = BatchDecodeEngine(model, BATCH, cache_len=cache_len).capture()
    res = {"cache_len": cache_len, "copy": copy_table(eng, positions, fans, a.calls)}
    if not a.no_generate:
        res["generate"] = generate_table(eng, positions)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
