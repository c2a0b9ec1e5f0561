"""Multi-token decode steps: DecodeEngine.step_tokens at T = 1 .. 8 against the single step (four and five launches) and
BatchDecodeEngine at B = T, timed in the same process on the full-size TinyLlama shape, W8A8 and W4A8, at 256 and 2 048 cached
positions; the break-even acceptance per T; one self-draft speculative run.

    python tools/bench_decode_multi.py [--steps 64] [--contexts 256,2048] [--rows 1,...,8] [--wbits 8,4] [--new-tokens 64]

Recipe of tools/bench_decode_batch.py: random-init model -> the reference's surgery and mixed-precision rules -> one calibration pass
-> engines; random cached keys / values (fill_cache_random); one captured hipGraph per step kind (step_tokens: one per row count);
HIP events around `steps` graph replays, best of 3.  Prints ONE JSON line.
  rows{T}_{L}launch_ctx{c}: the T-row step of an L-launch engine (L = 4: the 16-position-chunked value cache); x_batch = its time over
    BatchDecodeEngine's B = T step at the same positions (the goal: <= 1.1), x_single = over one single step of the same engine.
  breakeven_accept: per T, the per-proposal acceptance rate a at which a round of T rows -- (1 - a^T) / (1 - a) tokens expected for one
    T-row step -- matches T-row-step-time / single-step-time tokens, i.e. at which greedy speculation stops losing to plain decoding
    (the draft's own cost NOT included).
  spec_selfdraft: generate() with the target as its own draft (a second engine on the same model): every proposal is accepted, so this
    is an UPPER BOUND on acceptance and says nothing about real drafts (random weights: acceptance rates of real drafts mean nothing);
    tok_s includes the draft's time, target_only_tok_s counts the target's T-row steps only."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_decode_batch import _model, _time  # noqa: E402


def _breakeven(ratio: float, T: int) -> float:
    """The acceptance a in [0, 1] with (1 - a^T) / (1 - a) = ratio (T tokens at a = 1); None when even a = 1 does not pay."""
    if ratio > T:
        return None
    if ratio <= 1.0:
        return 0.0
    lo, hi = 0.0, 1.0
    for _ in range(60):
        a = (lo + hi) / 2
        e = sum(a ** i for i in range(T))
        lo, hi = (a, hi) if e < ratio else (lo, a)
    return round((lo + hi) / 2, 3)


def run(wbits, contexts, rows, steps, new_tokens, dev):
    from mobilequant_amd.decode import DecodeEngine
    from mobilequant_amd.decode_batch import BatchDecodeEngine
    cache_len = max(contexts) + steps * max(rows) + 16
    cache_len = (cache_len + 15) // 16 * 16
    model, shape = _model(dev, wbits, max(2048, cache_len))
    singles = {L: DecodeEngine(model, cache_len=cache_len, launches=L) for L in (4, 5)}
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
        for T in rows:
            eng.set_position(min(contexts))
            eng.step_tokens([17] * T)                       # records the T-row graph
            for ctx in contexts:
                ms = _time(eng._row_graphs[T].replay, lambda: eng.set_position(ctx), steps)
                out[f"rows{T}_{L}launch_ctx{ctx}"] = {"ms_per_step": round(ms, 4), "tok_s_all_accepted": round(1000.0 * T / ms, 1),
                                                      "x_single": round(ms / out[f"single_{L}launch_ctx{ctx}"]["ms_per_step"], 3)}
    for B in rows:
        be = BatchDecodeEngine(model, B, cache_len=cache_len)
        for b in range(B):
            be.fill_cache_random(b, max(contexts), seed=b)
        be.tok.fill_(17)
        be.capture()
        for ctx in contexts:
            def set_pos(ctx=ctx, be=be):
                for b in range(be.batch):
                    be.set_position(b, ctx)
            ms = _time(be.graph.replay, set_pos, steps)
            out[f"batch{B}_ctx{ctx}"] = {"ms_per_step": round(ms, 4)}
            for L in singles:
                r = out[f"rows{B}_{L}launch_ctx{ctx}"]
                r["x_batch"] = round(r["ms_per_step"] / ms, 3)
        del be
        torch.cuda.empty_cache()
    for ctx in contexts:
        base = out[f"single_4launch_ctx{ctx}"]["ms_per_step"]
        out[f"breakeven_accept_ctx{ctx}"] = {f"T{T}": _breakeven(out[f"rows{T}_4launch_ctx{ctx}"]["ms_per_step"] / base, T) for T in rows}
    # self-draft speculative run (upper bound: every proposal accepted)
    eng, draft = singles[4], DecodeEngine(model, cache_len=cache_len)
    draft.capture()
    g = torch.Generator().manual_seed(3)
    ctx_ids = torch.randint(3, shape.vocab, (min(contexts),), generator=g).tolist()
    res = {}
    for name, kw in (("plain", {}), ("selfdraft_k7", {"draft": draft, "num_draft": 7})):
        ids = eng.generate(ctx_ids, 2, **kw)                     # warm-up (graphs of every row count used below)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ids = eng.generate(ctx_ids, new_tokens, **kw)
        torch.cuda.synchronize()
        res[name] = {"s": time.perf_counter() - t0, "ids": ids}
    plain, spec = res["plain"], res["selfdraft_k7"]
    st = eng.spec_stats
    t8 = out[f"rows8_4launch_ctx{min(contexts)}"]["ms_per_step"]
    out["spec_selfdraft"] = {"label": "UPPER BOUND: the target is its own draft, every proposal accepted", "context": min(contexts),
                             "new_tokens": new_tokens, "same_ids_as_plain": spec["ids"] == plain["ids"], **st,
                             "plain_generate_s": round(plain["s"], 4), "spec_generate_s": round(spec["s"], 4),
                             "target_only_tok_s": round(1000.0 * (new_tokens - 1) / (st["target_steps"] * t8), 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--contexts", default="256,2048")
    ap.add_argument("--rows", default="1,2,3,4,5,6,7,8")
    ap.add_argument("--wbits", default="8,4")
    ap.add_argument("--new-tokens", type=int, default=64)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_decode_multi needs the GPU"
    dev = torch.device("cuda:0")
    contexts = [int(c) for c in a.contexts.split(",")]
    rows = [int(r) for r in a.rows.split(",")]
    if 8 not in rows:
        ap.error("--rows must include 8 (the self-draft run is priced with the 8-row step)")
    res = {"metric": "decode_multi_tinyllama", "steps": a.steps, "unit": "ms per step; tok/s"}
    for wb in (int(w) for w in a.wbits.split(",")):
        res["w8a8" if wb == 8 else "w4a8"] = run(wb, contexts, rows, a.steps, a.new_tokens, dev)
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
