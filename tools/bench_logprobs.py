"""Per-token log-probabilities (mq_logprob_top): the launch against one read of the rows (mq_sample's unfiltered call)
and against the torch sequence it replaces, and tokens/s of generate(sampling=...) with and without logprobs=, in one process.

    python tools/bench_logprobs.py [--calls 200] [--vocabs 32000,100352,256000] [--rows 1,8] [--tops 0,5,20] [--new-tokens 128] [--context 256]
                                   [--no-generate]

kernel: per (V, rows, n_top) HIP events around `calls` back-to-back eager calls, best of 3, microseconds per call (tools/bench_sample.py's
  protocol): mq_logprob_top; mq_sample's unfiltered call (temperature 0.7: its launch 1 is the natural floor for one read of the rows);
  the torch sequence: log_softmax, topk, gather, rank by comparison.  gb_s = rows * V * 4 bytes / the launch's time.
  All on random Gaussian logits (scale 3) that stay in the caches.
generate: the TinyLlama-1.1B shape (random weights, the reference's surgery), W8A8, a `context`-token prompt, `new-tokens` new tokens,
  engine captured; wall clock around generate() without the prefill, best of 3, tokens/s for sampling= alone (run twice: its own spread)
  and with logprobs=0 / 5 / 20.
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


def kernel_table(vocabs, rows_list, tops, calls, dev):
    from mobilequant_amd import SamplingParams
    from mobilequant_amd.sampling import LogprobLaunch, SampleLaunch
    out = {}
    for V in vocabs:
        for rows in rows_list:
            g = torch.Generator(device=dev).manual_seed(V + rows)
            logits = torch.randn(rows, V, generator=g, device=dev) * 3.0
            pos = torch.arange(rows, dtype=torch.int32, device=dev) + 5
            tok = torch.randint(0, V, (rows,), generator=g, device=dev)
            sl = SampleLaunch(logits, pos, tok.clone(), cache_len=64)
            sl.set_rows([SamplingParams(temperature=0.7, seed=1)] * rows, list(range(rows)))
            for _ in range(5):
                sl.launch()
            torch.cuda.synchronize()
            s_us = _events(sl.launch, calls)
            for n in tops:
                lp = LogprobLaunch(logits, pos, tok, cache_len=64, n_top=n)

                def torch_seq():
                    ls = torch.log_softmax(logits, dim=-1)
                    chosen = ls.gather(1, tok.view(-1, 1))
                    rank = (ls > chosen).sum(dim=-1) + 1
                    top = torch.topk(ls, n, dim=-1) if n else None
                    return chosen, rank, top

                for _ in range(5):
                    lp.launch()
                    torch_seq()
                torch.cuda.synchronize()
                k_us, t_us = _events(lp.launch, calls), _events(torch_seq, calls)
                out[f"V{V}_rows{rows}_top{n}"] = {"mq_logprob_top_us": round(k_us, 2), "mq_sample_us": round(s_us, 2), "torch_us": round(t_us, 2),
                                                  "x_sample": round(k_us / s_us, 3), "x_torch": round(k_us / t_us, 3),
                                                  "gb_s": round(rows * V * 4 / k_us / 1e3, 1), "miss": bool(k_us >= t_us)}
    return out


def generate_table(context, new_tokens, tops, dev):
    from bench_decode_batch import _model
    from mobilequant_amd import SamplingParams
    from mobilequant_amd.decode import DecodeEngine
    cache_len = (context + new_tokens + 31) // 16 * 16
    model, shape = _model(dev, 8, max(2048, cache_len))
    eng = DecodeEngine(model, cache_len=cache_len).capture()
    g = torch.Generator().manual_seed(9)
    prompt = torch.randint(3, shape.vocab, (context,), generator=g).tolist()
    sp = SamplingParams(temperature=0.7, top_k=40, top_p=0.9, seed=3)
    paths = {"sampling": lambda: eng.generate(prompt, new_tokens, sampling=sp, stream=0)}
    for n in tops:
        paths[f"logprobs{n}"] = lambda n=n: eng.generate(prompt, new_tokens, sampling=sp, stream=0, logprobs=n)
    paths["sampling_again"] = paths["sampling"]

    def prefill_only():
        eng.reset()
        eng.prefill(prompt)
        torch.cuda.synchronize()
    out = {}
    for _ in range(2):
        prefill_only()
    t_pre = min(_wall(prefill_only) for _ in range(3))
    for name, fn in paths.items():
        fn()                                                    # warm-up (records the sample + step graph of its kind)
        best = min(_wall(fn) for _ in range(3))
        out[name] = {"tok_s": round(new_tokens / max(best - t_pre, 1e-9), 1), "ms_per_token": round(1e3 * (best - t_pre) / new_tokens, 4)}
    out["prefill_ms"] = round(1e3 * t_pre, 2)
    for n in tops:
        out[f"x_sampling_logprobs{n}"] = round(out[f"logprobs{n}"]["tok_s"] / out["sampling"]["tok_s"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--vocabs", default="32000,100352,256000")
    ap.add_argument("--rows", default="1,8")
    ap.add_argument("--tops", default="0,5,20")
    ap.add_argument("--context", type=int, default=256)
    ap.add_argument("--new-tokens", type=int, default=128)
    ap.add_argument("--no-generate", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_logprobs.py needs an MI355X: there is no CPU path")
    dev = torch.device("cuda:0")
    tops = [int(v) for v in a.tops.split(",")]
    res = {"kernel": kernel_table([int(v) for v in a.vocabs.split(",")], [int(v) for v in a.rows.split(",")], tops, a.calls, dev)}
    if not a.no_generate:
        res["generate"] = generate_table(a.context, a.new_tokens, tops, dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
