"""Beam search on the batched engine: mq_beam_select, mq_decode_cache_reorder and a whole generate_beam step, each beside
the thing a reader would compare it with, in one process.

    python tools/bench_beam.py [--calls 20] [--positions 256,2048] [--no-step]

select: V = 32 000, eight rows of Gaussian logits, as 1 group x 8 beams (K = 16) and 2 groups x 4 beams (K = 8).  `kernel` -- the launches'
  time on the device: `calls` calls recorded into ONE hipGraph, HIP events around its replay (tools/bench_sample.py's protocol: warmed,
  best of 3); `eager` -- ops.beam_select back to back, its host-side checks included; `select_readback` -- wall clock of the call plus
  the ONE read-back of the n_groups x K records, what a generate_beam step pays; `host_sort` -- the alternative it replaces: read the
  eight logits rows back (8 x 128 KB), log-softmax, add cum and take the top K per group in torch on the host.
reorder: the TinyLlama-1.1B shape (22 layers: 44 caches of 4 KV heads x 64), batch 8, every slot at `positions` cached positions of random
  bytes.  Per (positions, table) the `kernel` time as above for a swap of two slots, the rotation of all eight and a fan-out of 7 from a
  slot that survives; beside each, mq_decode_cache_fork's kernel time at the nearest bytes written (fan-out 1, 7 and 7): the yardstick
  of DESIGN.md 4.3k.  gb_s = (bytes read + bytes written) / kernel time.
step: W8A8, one prompt of 256 tokens, 8 beams, engine captured: wall clock per step of generate_beam (select, read-back, host rule,
  upload, reorder, step(); the difference of a 33-token and a 1-token run over 32) against the plain batched step() with eight slots
  live at the same positions.
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
TABLES = {"swap": [1, 0, 2, 3, 4, 5, 6, 7], "rotation8": [1, 2, 3, 4, 5, 6, 7, 0], "fan7": [0] * 8}
FORK_FAN = {"swap": 1, "rotation8": 7, "fan7": 7}                  # the fork launch nearest in bytes written (it cannot write a source)


def _graph_us(fn, calls):
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            fn()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    return _events(g.replay, 1) / calls


def select_table(dev, calls, V=32000):
    from mobilequant_amd import _lib, ops
    gen = torch.Generator().manual_seed(1)
    logits = (torch.randn(BATCH, V, generator=gen) * 3).to(dev)
    cum = (-torch.rand(BATCH, generator=gen) * 20).to(dev)
    scratch = torch.empty(_lib.MQ_BEAM_SCRATCH_BYTES, dtype=torch.uint8, device=dev)
    out = {}
    for name, G, K in (("1x8", 1, 16), ("2x4", 2, 8)):
        group = torch.tensor([r // (BATCH // G) for r in range(BATCH)], dtype=torch.int32).to(dev)
        rec = torch.zeros(4 * G * K + BATCH, dtype=torch.int32, device=dev)
        n = G * K
        bufs = (rec[:n].view(torch.float32).view(G, K), rec[n:2 * n].view(G, K), rec[2 * n:3 * n].view(G, K), rec[3 * n:4 * n].view(torch.float32).view(G, K),
                rec[4 * n:].view(torch.float32))

        def launch():
            ops.beam_select(logits, cum, group, G, K, out=bufs, scratch=scratch)

        def select_readback():
            launch()
            return rec[:4 * n].cpu()

        def host_sort():
            rows = logits.cpu().double()
            s = (cum.cpu().double()[:, None] + torch.log_softmax(rows, dim=-1)).view(G, -1)
            return s.topk(K, dim=-1)

        for fn in (launch, select_readback, host_sort):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        out[name] = {"kernel_us": round(_graph_us(launch, calls), 2), "eager_us": round(_events(launch, calls), 2),
                     "select_readback_us": round(1e6 * min(_wall(select_readback) for _ in range(5)), 1),
                     "host_sort_us": round(1e6 * min(_wall(host_sort) for _ in range(5)), 1), "record_bytes": 16 * n, "row_bytes": 4 * V * BATCH}
    return out


def reorder_table(eng, positions, calls):
    from mobilequant_amd import ops
    s = eng.shape
    caches = eng.k_cache + eng.v_cache
    out = {}
    for P in positions:
        for b in range(BATCH):
            eng.fill_cache_random(b, P, seed=P + b)
        once = P * s.head_dim * s.kv_heads * len(caches)          # one slot's live bytes, all caches
        for name, table in TABLES.items():
            parent = torch.tensor(table, dtype=torch.int32).to(eng.dev)
            written = sum(p != d for d, p in enumerate(table)) * once
            read = len({p for d, p in enumerate(table) if p != d}) * once
            fan = FORK_FAN[name]
            fparent = torch.tensor([0] * (1 + fan) + list(range(1 + fan, BATCH)), dtype=torch.int32).to(eng.dev)
            r_us = _graph_us(lambda: ops.decode_cache_reorder(caches, eng.pos, parent, table=eng._fork_table), calls)
            f_us = _graph_us(lambda: ops.decode_cache_fork(caches, eng.pos, fparent, table=eng._fork_table), calls)
            e_us = _events(lambda: ops.decode_cache_reorder(caches, eng.pos, parent, table=eng._fork_table), calls)
            out[f"pos{P}_{name}"] = {"kernel_us": round(r_us, 2), "eager_us": round(e_us, 2), "bytes_written": written,
                                     "gb_s": round((read + written) / r_us / 1e3, 1), "fork_fan": fan, "fork_kernel_us": round(f_us, 2),
                                     "fork_bytes_written": fan * once, "fork_gb_s": round((1 + fan) * once / f_us / 1e3, 1),
                                     "us_per_mb": round(r_us / (written / 1e6), 3), "fork_us_per_mb": round(f_us / (fan * once / 1e6), 3)}
        for b in range(BATCH):
            eng.release(b)
    return out


def step_table(eng, P=256, steps=32):
    g = torch.Generator().manual_seed(P)
    prompt = torch.randint(3, eng.shape.vocab, (P,), generator=g).tolist()
    eng.generate_beam([prompt], 2, BATCH)                          # warm-up
    one = min(_wall(lambda: eng.generate_beam([prompt], 1, BATCH)) for _ in range(3))
    many = min(_wall(lambda: eng.generate_beam([prompt], 1 + steps, BATCH)) for _ in range(3))
    stats = dict(eng.beam_stats)
    for b in range(BATCH):
        eng.fill_cache_random(b, P, seed=b)

    def plain():
        for b in range(BATCH):
            eng.set_position(b, P)
        for _ in range(steps):
            eng.step()
    plain()
    plain_s = min(_wall(plain) for _ in range(3))
    for b in range(BATCH):
        eng.release(b)
    beam_us, plain_us = 1e6 * (many - one) / steps, 1e6 * plain_s / steps
    return {"prompt": P, "beams": BATCH, "beam_step_us": round(beam_us, 1), "plain_step_us": round(plain_us, 1), "overhead_us": round(beam_us - plain_us, 1),
            "x_plain": round(beam_us / plain_us, 3), "beam_stats": stats}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--positions", default="256,2048")
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_beam.py needs an MI355X: there is no CPU path")
    from bench_decode_batch import _model
    from mobilequant_amd.decode_batch import BatchDecodeEngine
    dev = torch.device("cuda:0")
    positions = [int(v) for v in a.positions.split(",")]
    cache_len = (max(positions + [256 + 40]) + 1 + 31) // 16 * 16
    res = {"cache_len": cache_len, "select": select_table(dev, a.calls)}
    model, _ = _model(dev, 8, max(2048, cache_len))
    eng = BatchDecodeEngine(model, BATCH, cache_len=cache_len).capture()
    res["reorder"] = reorder_table(eng, positions, a.calls)
    if not a.no_step:
        res["step"] = step_table(eng)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
