"""Speculative decoding under seeded sampling in the batched engine (mq_sample_ragged): the ragged selection launch beside
the entries it stands next to, one captured ragged step with the selection behind it beside the bare step, and generate_speculative
beside the batched plain sampled generation, in one process (tools/bench_spec_sample.py's protocol: HIP events, warmed, `calls`
back-to-back calls, best of 3; the yardstick is run twice and both runs are printed).

    python tools/bench_spec_sample_batch.py [--calls 200] [--vocabs 32000,256000] [--context 256] [--new-tokens 64] [--no-engine]

kernel (a): per (V, plan, neutral | penalised) microseconds per eager call of mq_sample_ragged over R = 8 rows laid out as 8x1, 4x2, 2x4
  and 1x8 (runs x rows per run, a sequence per run; temperature 0.7, top_k 40, top_p 0.9; penalised: repetition 1.3, presence 0.2,
  frequency 0.1 and a logit bias on histories with 5 % of their entries seen, random row tokens), beside mq_sample_rows at T = 8 (the
  yardstick: the parent's entry, the same work per row apart from the locator's scalar loads; timed twice, `rows_us` and `rows_again_us`,
  whose gap is the spread to judge a difference by) and mq_sample / mq_sample_penalized over the same 8 rows as 8 sequences.
round (b): the TinyLlama-1.1B shape (random weights, the reference's surgery), W8A8, batch 4, captured, `context` cached positions per
  slot: microseconds of step_sample_tokens (ragged step + selection, ONE graph) + rewinds beside step_tokens + rewinds at R = 8 (4 x 2).
generate (c): wall clock around generate_speculative (num_draft 4) for 4 prompts with an oracle draft (it proposes the plain ids) and with
  prompt_lookup_draft beside the batched generate(sampling=...), the prefills taken off, tokens/s over all prompts, best of 3, with
  the acceptance counts.  Random weights: this is the mechanism's cost, not a speed-up claim.
Prints ONE JSON line."""
from __future__ import annotations

import argparse
import dataclasses
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_sample import PENALTIES, _events, _wall  # noqa: E402

R = 8
PLANS = {"8x1": (8, 1), "4x2": (4, 2), "2x4": (2, 4), "1x8": (1, 8)}


def kernel_table(vocabs, calls, dev):
    from mobilequant_amd import SamplingParams
    from mobilequant_amd.sampling import RaggedRowsLaunch, RowsLaunch, SampleLaunch
    out = {}
    sp = SamplingParams(temperature=0.7, top_k=40, top_p=0.9, seed=1)
    spp = dataclasses.replace(sp, **PENALTIES)
    for V in vocabs:
        g = torch.Generator(device=dev).manual_seed(V)
        logits = torch.randn(R, V, generator=g, device=dev) * 3.0
        pos = torch.arange(R, dtype=torch.int32, device=dev) + 5
        tok = torch.zeros(R, dtype=torch.int64, device=dev)
        hist = torch.where(torch.rand(R, V, generator=g, device=dev) < 0.05, torch.randint(1, 6, (R, V), generator=g, device=dev, dtype=torch.int32), 0)
        sl = SampleLaunch(logits, pos, tok, cache_len=1 << 20)                          # 8 sequences: the batch whose requests the ragged launch reads
        one = SampleLaunch(logits[:1], pos[:1], tok[:1], cache_len=1 << 20)             # the one request mq_sample_rows reads
        row_tok = torch.randint(0, V, (R,), generator=g, device=dev)
        rl = RowsLaunch(one, logits, pos[:1], row_tok[1:], torch.zeros(R, dtype=torch.int64, device=dev))
        row_seq, row_pos = torch.zeros(R, dtype=torch.int32, device=dev), torch.zeros(R, dtype=torch.int32, device=dev)
        gl = RaggedRowsLaunch(sl, logits, row_seq, row_pos, row_tok, torch.zeros(R, dtype=torch.int64, device=dev), cache_len=1 << 20)
        for mode, req in (("neutral", sp), ("penalised", spp)):
            sl.set_rows([req] * R, [0] * R)
            one.set_rows([req], [0])
            if req.penalized:
                sl.history.copy_(hist)
                one.history.copy_(hist[:1])
                sl.pargs.observe = 0                                                   # the same history in every call
            entry = "mq_sample_penalized" if req.penalized else "mq_sample"
            fns = {"rows_us": lambda: rl.launch(R), entry + "_us": sl.launch}
            for fn in list(fns.values()) + [lambda: gl.launch(R)]:
                for _ in range(5):
                    fn()
            torch.cuda.synchronize()
            cell = {k: round(_events(fn, calls), 2) for k, fn in fns.items()}
            for plan, (runs, per) in PLANS.items():
                row_seq.copy_(torch.arange(runs, dtype=torch.int32).repeat_interleave(per))
                row_pos.copy_(torch.arange(per, dtype=torch.int32).repeat(runs) + 5)
                torch.cuda.synchronize()
                cell[f"ragged_{plan}_us"] = round(_events(lambda: gl.launch(R), calls), 2)
            cell["rows_again_us"] = round(_events(fns["rows_us"], calls), 2)
            cell["yardstick_spread_us"] = round(abs(cell["rows_again_us"] - cell["rows_us"]), 2)
            cell["x_rows_1x8"] = round(cell["ragged_1x8_us"] / min(cell["rows_us"], cell["rows_again_us"]), 3)
            out[f"V{V}_{mode}"] = cell
    return out


def engine_tables(context, new_tokens, calls, dev):
    from bench_decode_batch import _model
    from mobilequant_amd import SamplingParams
    from mobilequant_amd.decode import prompt_lookup_draft
    from mobilequant_amd.decode_batch import BatchDecodeEngine
    NB = 4
    cache_len = (context + new_tokens + 31) // 16 * 16
    model, shape = _model(dev, 8, max(2048, cache_len))
    eng = BatchDecodeEngine(model, NB, cache_len=cache_len).capture()
    g = torch.Generator().manual_seed(9)
    prompts = [torch.randint(3, shape.vocab, (context,), generator=g).tolist() for _ in range(NB)]
    sp = SamplingParams(temperature=0.7, top_k=40, top_p=0.9, seed=3)
    spp = dataclasses.replace(sp, **PENALTIES)
    # (b) one round at R = 8: two rows per slot
    rnd = {}
    for name, req in (("neutral", sp), ("penalised", spp)):
        for b in range(NB):
            eng.release(b)
        for b in range(NB):
            eng.prefill(b, prompts[b])
        eng.set_sampling(req, list(range(NB)))
        for b in range(NB):
            eng.observe_history(b, prompts[b])
        toks = {b: prompts[b][:2] for b in range(NB)}

        def back():
            for b in range(NB):
                eng.rewind(b, context)

        def bare():
            eng.step_tokens(toks)
            back()

        def with_selection():
            eng.step_sample_tokens(toks)
            back()
        for fn in (bare, with_selection):
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        a, a2, b_ = _events(bare, calls), _events(bare, calls), _events(with_selection, calls)
        rnd[f"R8_{name}"] = {"step_tokens_us": round(a, 2), "step_tokens_again_us": round(a2, 2), "step_sample_tokens_us": round(b_, 2),
                             "selection_us": round(b_ - min(a, a2), 2)}
    # (c) generation

    def prefill_only():
        for b in range(NB):
            eng.release(b)
        for b in range(NB):
            eng.prefill(b, prompts[b])
        torch.cuda.synchronize()
    for _ in range(2):
        prefill_only()
    t_pre = min(_wall(prefill_only) for _ in range(3))
    gen = {"prefill_ms": round(1e3 * t_pre, 2)}
    for name, req in (("neutral", sp), ("penalised", spp)):
        want = eng.generate(prompts, new_tokens, sampling=req)
        oracle = [(lambda ids, k, t=t: t[len(ids):len(ids) + k]) for t in want]
        paths = {"plain": lambda: eng.generate(prompts, new_tokens, sampling=req),
                 "oracle": lambda: eng.generate_speculative(prompts, new_tokens, oracle, sampling=req, num_draft=4),
                 "prompt_lookup": lambda: eng.generate_speculative(prompts, new_tokens, prompt_lookup_draft(3), sampling=req, num_draft=4)}
        for path, fn in paths.items():
            ids = fn()                                              # warm-up (records the graphs)
            best = min(_wall(fn) for _ in range(3)) - t_pre
            cell = gen[f"{name}_{path}"] = {"tok_s": round(NB * new_tokens / max(best, 1e-9), 1), "ms_per_round_of_tokens": round(1e3 * best / new_tokens, 4),
                                          "same_ids": ids == want}
            if path != "plain":
                cell.update({k: eng.spec_stats[k] for k in ("rounds", "proposed", "accepted")})
                cell["x_plain"] = round(cell["tok_s"] / gen[f"{name}_plain"]["tok_s"], 3)
    return rnd, gen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--vocabs", default="32000,256000")
    ap.add_argument("--context", type=int, default=256)
    ap.add_argument("--new-tokens", type=int, default=64)
    ap.add_argument("--no-engine", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_spec_sample_batch.py needs an MI355X: there is no CPU path")
    dev = torch.device("cuda:0")
    res = {"kernel": kernel_table([int(v) for v in a.vocabs.split(",")], a.calls, dev)}
    if not a.no_engine:
        res["round"], res["generate"] = engine_tables(a.context, a.new_tokens, a.calls, dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
