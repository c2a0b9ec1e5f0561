"""Speculative decoding under seeded sampling (mq_sample_rows): the multi-row selection launch beside the entries it
stands next to, one speculative round beside the bare multi-token step, and generate_speculative beside plain sampled generation, in
one process (tools/bench_sample.py's protocol: HIP events, warmed, `calls` back-to-back calls, best of 3).

    python tools/bench_spec_sample.py [--calls 200] [--vocabs 32000,100352,256000] [--rows 1,4,8] [--parent-lib PATH]
                                      [--context 256] [--new-tokens 128] [--no-engine]

kernel (a): per (V, T, neutral | penalised) microseconds per eager call of mq_sample_rows over T rows of one sequence (temperature 0.7,
  top_k 40, top_p 0.9; penalised: repetition 1.3, presence 0.2, frequency 0.1 and a logit bias on a history with 5 % of its entries
  seen, T - 1 random proposals) beside mq_sample / mq_sample_penalized over the same T rows as T sequences.  --parent-lib: another build
  of the library (the parent commit's), whose mq_sample / mq_sample_penalized are timed on the same argument blocks in the same process:
  the two entries are the parent's code and must not have moved.
round (b): the TinyLlama-1.1B shape (random weights, the reference's surgery), W8A8, captured, `context` cached positions: microseconds of
  step_sample_tokens (rows step + selection, ONE graph) + rewind beside step_tokens + rewind, T = 5 and 8.
generate (c): wall clock around generate_speculative (num_draft 4) with a self-draft engine and with prompt_lookup_draft beside plain
  generate(sampling=...), prefill taken off, tokens/s, best of 3, with the acceptance counts.  Random weights: this is the mechanism's
  cost, not a speed-up claim -- a self-draft costs as much as the target and random text has nothing to look up.
Prints ONE JSON line."""
from __future__ import annotations

import argparse
import ctypes
import dataclasses
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_sample import PENALTIES, _events, _wall  # noqa: E402


def _parent(path):
    """mq_sample / mq_sample_penalized of another build of the library, on this package's argument blocks."""
    from mobilequant_amd import _lib
    _lib.load()
    lib = ctypes.CDLL(path)
    for name, blk in (("mq_sample", _lib.MqSampleArgs), ("mq_sample_penalized", _lib.MqSamplePenalizedArgs)):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = ctypes.c_int, [ctypes.POINTER(blk), ctypes.c_void_p]
    if lib.mq_version() // 100 != _lib.HEADER_MAJOR:
        raise SystemExit(f"--parent-lib {path}: version {lib.mq_version()} is another major")
    return lib


def kernel_table(vocabs, rows_list, calls, dev, parent=None):
    from mobilequant_amd import SamplingParams
    from mobilequant_amd.sampling import RowsLaunch, SampleLaunch
    out = {}
    sp = SamplingParams(temperature=0.7, top_k=40, top_p=0.9, seed=1)
    spp = dataclasses.replace(sp, **PENALTIES)
    for V in vocabs:
        for T in rows_list:
            g = torch.Generator(device=dev).manual_seed(V + T)
            logits = torch.randn(T, V, generator=g, device=dev) * 3.0
            pos = torch.arange(T, dtype=torch.int32, device=dev) + 5
            tok = torch.zeros(T, dtype=torch.int64, device=dev)
            hist = torch.where(torch.rand(T, V, generator=g, device=dev) < 0.05, torch.randint(1, 6, (T, V), generator=g, device=dev, dtype=torch.int32), 0)
            sl = SampleLaunch(logits, pos, tok, cache_len=1 << 20)                      # T sequences
            one = SampleLaunch(logits[:1], pos[:1], tok[:1], cache_len=1 << 20)         # the one request mq_sample_rows reads
            prop = torch.randint(0, V, (max(T - 1, 1),), generator=g, device=dev)
            rl = RowsLaunch(one, logits, pos[:1], prop, torch.zeros(T, dtype=torch.int64, device=dev))
            for mode, req in (("neutral", sp), ("penalised", spp)):
                sl.set_rows([req] * T, [0] * T)
                one.set_rows([req], [0])
                if req.penalized:
                    sl.history.copy_(hist)
                    one.history.copy_(hist[:1])
                    sl.pargs.observe = 0                                               # the same history in every call
                st = lambda: torch.cuda.current_stream(dev).cuda_stream                # noqa: E731
                entry = "mq_sample_penalized" if req.penalized else "mq_sample"
                blk = sl.pargs if req.penalized else sl.args
                fns = {"mq_sample_rows_us": lambda: rl.launch(T), entry + "_us": sl.launch}
                if parent is not None:
                    fns["parent_" + entry + "_us"] = lambda: getattr(parent, entry)(ctypes.byref(blk), st())
                for fn in fns.values():
                    for _ in range(5):
                        fn()
                torch.cuda.synchronize()
                cell = {k: round(_events(fn, calls), 2) for k, fn in fns.items()}
                cell["x_entry"] = round(cell["mq_sample_rows_us"] / cell[entry + "_us"], 3)
                if parent is not None:
                    cell["x_parent"] = round(cell[entry + "_us"] / cell["parent_" + entry + "_us"], 3)
                out[f"V{V}_T{T}_{mode}"] = cell
    return out


def engine_tables(context, new_tokens, calls, dev):
    from bench_decode_batch import _model
    from mobilequant_amd import SamplingParams
    from mobilequant_amd.decode import DecodeEngine, prompt_lookup_draft
    cache_len = (context + new_tokens + 31) // 16 * 16
    model, shape = _model(dev, 8, max(2048, cache_len))
    eng = DecodeEngine(model, cache_len=cache_len).capture()
    g = torch.Generator().manual_seed(9)
    prompt = torch.randint(3, shape.vocab, (context,), generator=g).tolist()
    sp = SamplingParams(temperature=0.7, top_k=40, top_p=0.9, seed=3)
    spp = dataclasses.replace(sp, **PENALTIES)
    # (b) one round
    rnd = {}
    for name, req in (("neutral", sp), ("penalised", spp)):
        eng.set_sampling(req, 0)
        eng.reset()
        eng.prefill(prompt)
        eng.observe_history(prompt)
        for T in (5, 8):
            toks = prompt[:T]

            def bare():
                eng.step_tokens(toks)
                eng.rewind(context)

            def with_selection():
                eng.step_sample_tokens(toks)
                eng.rewind(context)
            for fn in (bare, with_selection):
                for _ in range(5):
                    fn()
            torch.cuda.synchronize()
            a, b = _events(bare, calls), _events(with_selection, calls)
            rnd[f"T{T}_{name}"] = {"step_tokens_us": round(a, 2), "step_sample_tokens_us": round(b, 2), "selection_us": round(b - a, 2)}
    # (c) generation
    self_draft = DecodeEngine(model, cache_len=cache_len).capture()

    def prefill_only():
        eng.reset()
        eng.prefill(prompt)
        torch.cuda.synchronize()
    for _ in range(2):
        prefill_only()
    t_pre = min(_wall(prefill_only) for _ in range(3))
    gen = {"prefill_ms": round(1e3 * t_pre, 2)}
    for name, req in (("neutral", sp), ("penalised", spp)):
        paths = {"plain": (lambda: eng.generate(prompt, new_tokens, sampling=req, stream=0), 1),
                 "self_draft": (lambda: eng.generate_speculative(prompt, new_tokens, self_draft, sampling=req, stream=0, num_draft=4), 2),
                 "prompt_lookup": (lambda: eng.generate_speculative(prompt, new_tokens, prompt_lookup_draft(3), sampling=req, stream=0, num_draft=4), 1)}
        want = None
        for path, (fn, prefills) in paths.items():
            ids = fn()                                              # warm-up (records the graphs)
            want = ids if want is None else want
            best = min(_wall(fn) for _ in range(3)) - prefills * t_pre
            cell = gen[f"{name}_{path}"] = {"tok_s": round(new_tokens / max(best, 1e-9), 1), "ms_per_token": round(1e3 * best / new_tokens, 4),
                                          "same_ids": ids == want}
            if path != "plain":
                cell.update({k: eng.spec_stats[k] for k in ("rounds", "proposed", "accepted")})
                cell["x_plain"] = round(cell["tok_s"] / gen[f"{name}_plain"]["tok_s"], 3)
    return rnd, gen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--vocabs", default="32000,100352,256000")
    ap.add_argument("--rows", default="1,4,8")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--context", type=int, default=256)
    ap.add_argument("--new-tokens", type=int, default=128)
    ap.add_argument("--no-engine", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_spec_sample.py needs an MI355X: there is no CPU path")
    dev = torch.device("cuda:0")
    parent = _parent(a.parent_lib) if a.parent_lib else None
    res = {"kernel": kernel_table([int(v) for v in a.vocabs.split(",")], [int(v) for v in a.rows.split(",")], a.calls, dev, parent)}
    if not a.no_engine:
        res["round"], res["generate"] = engine_tables(a.context, a.new_tokens, a.calls, dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
