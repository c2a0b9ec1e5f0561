"""BatchDecodeEngine.generate_beam against the host rule of tests/beam_ref.py driven by a single DecodeEngine that
re-encodes every hypothesis (prefill + step): independent of the batched slots, of mq_beam_select and of mq_decode_cache_reorder -- the
only device result it shares is mq_logprob_top's m and logf(S) of a row, pinned by tests/test_gpu_logprob.py.  Sequences, the bits of
sum_logprobs and the scores must be equal.  The toy model is the TinyLlama-geometry one of the sampling and fork tests (vocabulary 160)."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import beam_ref  # noqa: E402
import logprob_ref  # noqa: E402
from test_gpu_decode_batch import _model, _prompts  # noqa: E402

pytestmark = pytest.mark.gpu

CACHE_LEN, B, NEW = 80, 8, 12
_STATE = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _setup(dev):
    """(model, single reference engine, eager batched engine, captured batched engine, the reference's rows by sequence), built once."""
    from mobilequant_amd.decode import DecodeEngine
    from mobilequant_amd.decode_batch import BatchDecodeEngine
    if not _STATE:
        m = _model(dev, "llama", 2, 8)
        _STATE.update(model=m, ref=DecodeEngine(m, cache_len=CACHE_LEN), eager=BatchDecodeEngine(m, B, cache_len=CACHE_LEN),
                      graph=BatchDecodeEngine(m, B, cache_len=CACHE_LEN).capture(), rows={})
    return _STATE


def _lister(dev, plen):
    """beam_ref's view of the model: the first-K list of the row behind `ids`, from the single engine alone (the first plen ids are the
    prompt: encoded as generate encodes it, the rest stepped).  Every sequence is encoded once and its 20-entry list is kept."""
    from mobilequant_amd import sampling
    st = _setup(dev)
    ref, rows = st["ref"], st["rows"]

    def lister(ids, K):
        key = (plen, tuple(ids))
        if key not in rows:
            ref.reset()
            if plen == 1:
                ref.step(ids[0])
            else:
                ref.prefill(ids[:plen])
            for t in ids[plen:]:
                ref.step(t)
            row = ref.logits.view(1, -1)
            _, _, top_id, top_lp = sampling.logprob_top(row, torch.zeros(1, dtype=torch.int64, device=dev), n_top=20)
            l, top_id, top_lp = row[0].cpu().numpy(), top_id[0].cpu().numpy(), top_lp[0].cpu().numpy()
            toks, lps = beam_ref.row_list(l, logprob_ref.normalise(l)[top_id[0]], -top_lp[0], 20)
            assert np.array_equal(toks, top_id) and np.array_equal(lps.view(np.int32), top_lp.view(np.int32))
            rows[key] = (toks, lps)
        toks, lps = rows[key]
        return toks[:K], lps[:K]
    return lister


def _prompt(st, n, seed=3):
    return _prompts(st["model"].shape.vocab, [n], seed=seed + n)[0]


def _same(got, want):
    seqs, scores, sums = want[:3]
    assert got.sequences == seqs, (got.sequences, seqs)
    assert np.array_equal(np.array(got.sum_logprobs, dtype=np.float32).view(np.int32), np.array(sums, dtype=np.float32).view(np.int32))
    assert all(float(np.float32(v)) == v for v in got.sum_logprobs)
    assert got.scores == scores, (got.scores, scores)


@pytest.mark.parametrize("W,plen", [(1, 5), (2, 1), (2, 17), (4, 5), (4, 17), (8, 1), (8, 5)])
def test_generate_beam_returns_the_references_hypotheses(dev, W, plen):
    st = _setup(dev)
    eng, lister, prompt = st["graph"], _lister(dev, plen), _prompt(st, plen)
    # without an EOS every hypothesis runs to max_new_tokens
    for new, lp, nrs in itertools.product((1, NEW), (0.0, 1.0, 2.0), sorted({1, W})):
        want = beam_ref.beam_search(lister, prompt, new, W, (), lp, True, nrs)
        got = eng.generate_beam([prompt], new, W, length_penalty=lp, num_return_sequences=nrs)
        assert len(got) == 1 and len(got[0].sequences) == nrs and all(len(s) == plen + new for s in got[0].sequences)
        _same(got[0], want)
    full = beam_ref.beam_search(lister, prompt, NEW, W, (), 1.0, True, W)
    if W > 1:
        assert any(p != list(range(W)) for p in full[3])           # the reference's beams really change parents
        assert eng.beam_stats["reorders"] >= 1 and eng.beam_stats["positions"] > 0 and eng.beam_stats["bytes"] > 0
    assert eng.beam_stats["selects"] == NEW and eng.beam_stats["steps"] == NEW - 1
    assert all(not eng.active(s) for s in range(B))
    # an EOS chosen from the run's own hypotheses, so that some finish mid-run
    eos_sets = [(full[0][-1][plen + 3],)]
    if W == 4:
        eos_sets.append((full[0][-1][plen + 3], full[0][0][plen + 5]))
    for eos in eos_sets:
        short = 0
        for lp, es, nrs in itertools.product((0.0, 1.0, 2.0), (True, False), sorted({1, W})):
            want = beam_ref.beam_search(lister, prompt, NEW, W, eos, lp, es, nrs)
            got = eng.generate_beam([prompt], NEW, W, eos_token_id=eos[0] if len(eos) == 1 else list(eos), length_penalty=lp, early_stopping=es,
                                    num_return_sequences=nrs)
            _same(got[0], want)
            short += sum(len(s) < plen + NEW and s[-1] in eos for s in got[0].sequences)
        assert short > 0                                           # hypotheses did finish at an EOS before max_new_tokens


def test_one_beam_is_greedy_generation(dev):
    st = _setup(dev)
    eng = st["graph"]
    for n in (1, 5, 17):
        p = _prompt(st, n)
        greedy = eng.generate([p], NEW)[0]
        got = eng.generate_beam([p], NEW, 1)[0]
        assert got.sequences == [greedy]
        eos = greedy[n + 4]
        assert eng.generate_beam([p], NEW, 1, eos_token_id=eos)[0].sequences == [eng.generate([p], NEW, eos_token_id=eos)[0]]


def test_a_prompts_result_does_not_depend_on_its_neighbours_its_group_or_the_graph(dev):
    st = _setup(dev)
    p, q = _prompt(st, 17), _prompt(st, 5)
    eos = beam_ref.beam_search(_lister(dev, 17), p, NEW, 4, (), 1.0, True, 4)[0][-1][17 + 3]
    kw = dict(eos_token_id=eos, length_penalty=1.0, early_stopping=False, num_return_sequences=4)
    outs = {}
    for name in ("graph", "eager"):
        eng = st[name]
        alone_p, alone_q = eng.generate_beam([p], NEW, 4, **kw)[0], eng.generate_beam([q], NEW, 4, **kw)[0]
        both = eng.generate_beam([p, q], NEW, 4, **kw)
        assert eng.beam_stats["reorders"] >= 1
        swapped = eng.generate_beam([q, p], NEW, 4, **kw)
        assert both == [alone_p, alone_q] and swapped == [alone_q, alone_p]
        outs[name] = both
    assert outs["graph"] == outs["eager"]
    for res, plen, prompt in ((outs["graph"][0], 17, p), (outs["graph"][1], 5, q)):
        _same(res, beam_ref.beam_search(_lister(dev, plen), prompt, NEW, 4, (eos,), 1.0, False, 4))


def test_the_engine_generates_as_before_afterwards(dev):
    from mobilequant_amd import SamplingParams
    st = _setup(dev)
    eng = st["graph"]
    prompts = [_prompt(st, 17), _prompt(st, 5), [7]]
    sp = SamplingParams(temperature=0.9, top_k=20, seed=4, repetition_penalty=1.2)
    before = (eng.generate(prompts, NEW), eng.generate(prompts, NEW, sampling=sp, logprobs=2))
    eng.generate_beam(prompts[:2], NEW, 4, eos_token_id=3)
    after = (eng.generate(prompts, NEW), eng.generate(prompts, NEW, sampling=sp, logprobs=2))
    assert before[0] == after[0] and before[1][0] == after[1][0]
    for x, y in zip(before[1][1], after[1][1]):
        for f in x._fields:
            assert torch.equal(getattr(x, f).view(torch.int32), getattr(y, f).view(torch.int32))
