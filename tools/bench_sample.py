"""Seeded device-side sampling (mq_sample): the selection launch against the torch sequence it replaces, and tokens/s
of generate() with and without it, in one process.

    python tools/bench_sample.py [--calls 200] [--vocabs 32000,100352,256000] [--rows 1,8] [--new-tokens 128] [--context 256] [--no-generate]
                                 [--penalties]

kernel: per (V, rows, mode) HIP events around `calls` back-to-back eager calls, best of 3, microseconds per call.
  mode temp     : mq_sample, temperature 0.7                      vs  multinomial(softmax(logits / T))          (generate(do_sample=True)'s rule)
  mode filtered : mq_sample, temperature 0.7, top_k 40, top_p 0.9  vs  sort, top-k mask, softmax, cumsum, top-p mask, multinomial
  Both sides are eager launches on random Gaussian logits (scale 3) that stay in the caches; mq_sample is two launches.
generate: the TinyLlama-1.1B shape (random weights, the reference's surgery), W8A8, a `context`-token prompt, `new-tokens` new tokens,
  engine captured; wall clock around generate() (it reads one token id per step), best of 3, tokens/s:
  greedy (argmax + .item() + step graph), do_sample (softmax + multinomial + .item() + step graph) -- the two legacy paths, whose code
  this feature does not touch -- and sampling= with top_k 40 / top_p 0.9 (one sample + step graph replay + one token read-back).
--penalties: per cell also mq_sample_penalized (repetition 1.3, presence 0.2, frequency 0.1 and a logit bias, all active, on a history
  with 5 % of its entries seen, observe on) as mq_sample_penalized_us and x_plain = penalised / plain; generate also runs the same
  top_k 40 / top_p 0.9 request with the penalties.
Prints ONE JSON line."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _events(fn, calls):
    best = float("inf")
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / calls)
    return best * 1e3                                       # us per call


PENALTIES = dict(repetition_penalty=1.3, presence_penalty=0.2, frequency_penalty=0.1, logit_bias={5: -1.0, 11: float("-inf")})


def kernel_table(vocabs, rows_list, calls, dev, penalties=False):
    from mobilequant_amd import SamplingParams
    from mobilequant_amd.sampling import SampleLaunch
    out = {}
    T = 0.7
    for V in vocabs:
        for rows in rows_list:
            g = torch.Generator(device=dev).manual_seed(V + rows)
            logits = torch.randn(rows, V, generator=g, device=dev) * 3.0
            pos = torch.arange(rows, dtype=torch.int32, device=dev) + 5
            tok = torch.zeros(rows, dtype=torch.int64, device=dev)
            sl = SampleLaunch(logits, pos, tok, cache_len=1 << 20)
            gen = torch.Generator(device=dev).manual_seed(1)

            def torch_temp():
                tok.copy_(torch.multinomial(torch.softmax(logits / T, dim=-1), num_samples=1, generator=gen).view(-1))

            def torch_filtered():
                z, idx = torch.sort(logits / T, dim=-1, descending=True)
                z[:, 40:] = float("-inf")
                p = torch.softmax(z, dim=-1)
                before = torch.cumsum(p, dim=-1) - p
                p = p.masked_fill(before >= 0.9, 0.0)
                tok.copy_(idx.gather(1, torch.multinomial(p, num_samples=1, generator=gen)).view(-1))

            for mode, sp, ref in (("temp", SamplingParams(temperature=T, seed=1), torch_temp),
                                  ("filtered", SamplingParams(temperature=T, top_k=40, top_p=0.9, seed=1), torch_filtered)):
                sl.set_rows([sp] * rows, list(range(rows)))
                for _ in range(5):
                    sl.launch()
                    ref()
                torch.cuda.synchronize()
                k_us, t_us = _events(sl.launch, calls), _events(ref, calls)
                cell = out[f"V{V}_rows{rows}_{mode}"] = {"mq_sample_us": round(k_us, 2), "torch_us": round(t_us, 2), "x_torch": round(k_us / t_us, 3),
                                                         "miss": bool(k_us >= t_us)}
                if penalties:
                    import dataclasses
                    sl.set_rows([dataclasses.replace(sp, **PENALTIES)] * rows, list(range(rows)))
                    seen = torch.rand(rows, V, generator=g, device=dev) < 0.05          # 5 % of the entries seen: prompt bit or a count
                    sl.history.copy_(torch.where(seen, torch.randint(1, 6, (rows, V), generator=g, device=dev, dtype=torch.int32), 0))
                    for _ in range(5):
                        sl.launch()
                    torch.cuda.synchronize()
                    p_us = _events(sl.launch, calls)
                    cell["mq_sample_penalized_us"], cell["x_plain"] = round(p_us, 2), round(p_us / k_us, 3)
    return out


def generate_table(context, new_tokens, dev, penalties=False):
    from bench_decode_batch import _model
    from mobilequant_amd import SamplingParams
    from mobilequant_amd.decode import DecodeEngine
    cache_len = (context + new_tokens + 31) // 16 * 16
    model, shape = _model(dev, 8, max(2048, cache_len))
    eng = DecodeEngine(model, cache_len=cache_len).capture()
    g = torch.Generator().manual_seed(9)
    prompt = torch.randint(3, shape.vocab, (context,), generator=g).tolist()
    sp = SamplingParams(temperature=0.7, top_k=40, top_p=0.9, seed=3)
    paths = {"greedy": lambda: eng.generate(prompt, new_tokens),
             "do_sample": lambda: eng.generate(prompt, new_tokens, do_sample=True, temperature=0.7, generator=torch.Generator(device=dev).manual_seed(3)),
             "sampling_topk40_topp0.9": lambda: eng.generate(prompt, new_tokens, sampling=sp, stream=0),
             "sampling_temperature_only": lambda: eng.generate(prompt, new_tokens, sampling=SamplingParams(temperature=0.7, seed=3), stream=0)}
    if penalties:
        spp = SamplingParams(temperature=0.7, top_k=40, top_p=0.9, seed=3, **PENALTIES)
        paths["sampling_topk40_topp0.9_penalized"] = lambda: eng.generate(prompt, new_tokens, sampling=spp, stream=0)
    # the prefill forward is the same in every path: time it once and take it off
    def prefill_only():
        eng.reset()
        eng.prefill(prompt)
        torch.cuda.synchronize()
    out = {}
    for _ in range(2):
        prefill_only()
    t_pre = min(_wall(prefill_only) for _ in range(3))
    for name, fn in paths.items():
        fn()                                                    # warm-up (records the sample + step graph)
        best = float("inf")
        for _ in range(3):
            t = _wall(fn)
            best = min(best, t)
        out[name] = {"tok_s": round(new_tokens / max(best - t_pre, 1e-9), 1), "ms_per_token": round(1e3 * (best - t_pre) / new_tokens, 4)}
    out["prefill_ms"] = round(1e3 * t_pre, 2)
    out["x_greedy"] = round(out["sampling_topk40_topp0.9"]["tok_s"] / out["greedy"]["tok_s"], 4)
    return out


def _wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--vocabs", default="32000,100352,256000")
    ap.add_argument("--rows", default="1,8")
    ap.add_argument("--context", type=int, default=256)
    ap.add_argument("--new-tokens", type=int, default=128)
    ap.add_argument("--no-generate", action="store_true")
    ap.add_argument("--penalties", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sample.py needs an MI355X: there is no CPU path")
    dev = torch.device("cuda:0")
    res = {"kernel": kernel_table([int(v) for v in a.vocabs.split(",")], [int(v) for v in a.rows.split(",")], a.calls, dev, a.penalties)}
    if not a.no_generate:
        res["generate"] = generate_table(a.context, a.new_tokens, dev, a.penalties)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
