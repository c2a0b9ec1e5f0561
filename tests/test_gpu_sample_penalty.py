"""GPU: repetition / presence / frequency penalties and logit bias in front of the seeded selection (mq_sample_penalized, step 0 of the
rule; csrc/mq_sample.hip).

The oracle is tests/sampling_penalty_ref.py (numpy fp32, one operation per line) feeding tests/sampling_ref.py.  Everything is exact
equality: the token against the reference, mq_sample_penalized(l, h) against mq_sample(transform(l, h)) with the transform done in numpy
and uploaded, a neutral request against mq_sample bit for bit, the histories against a numpy loop, and the engines against a host loop
over their own logits and against each other (slot b of a batch == the single engine on that sequence)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sampling_penalty_ref as PR  # noqa: E402
import sampling_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SAT = 0xFFFF


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def _logits(rng, V, plus_inf):
    """Gaussian logits (scale 3) with planted -inf, NaN, -0.0, an exact tie at the maximum and a block of equal values; +inf where the
    request has no filter (with a +inf in the row no softmax exists: the filters' masses are not defined)."""
    l = (rng.standard_normal(V) * 3.0).astype(np.float32)
    if V >= 64:
        idx = rng.choice(V, size=24, replace=False)
        l[idx[0:4]] = -np.inf
        l[idx[4]] = np.nan
        l[idx[5:7]] = -0.0
        l[idx[7:9]] = l.max() + np.float32(0.5)                      # a tie at the maximum
        l[idx[9:15]] = np.float32(1.25)                              # equal values inside the row
        if plus_inf:
            l[idx[15:17]] = np.inf
    else:
        l[V - 1] = -0.0
        l[1] = l[0]
        if plus_inf:
            l[2] = np.inf
    return l


def _history(rng, V, kind, logits):
    """About 5 % of the entries seen, and the row's three largest logits among them so that the penalties decide the draw: kind 0 prompt
    only, 1 generated only, 2 both, 3 both with one saturated count."""
    seen = rng.random(V) < 0.05
    with np.errstate(invalid="ignore"):
        seen[np.argsort(-np.nan_to_num(logits, nan=-np.inf), kind="stable")[:3]] = True
    idx = np.flatnonzero(seen)
    h = np.zeros(V, dtype=np.uint32)
    if kind in (0, 2, 3):
        h[idx[rng.random(len(idx)) < (1.0 if kind == 0 else 0.6)]] |= PR.PROMPT_BIT
    if kind in (1, 2, 3):
        cnt = rng.integers(1, 6, size=len(idx)).astype(np.uint32)
        gen = rng.random(len(idx)) < (1.0 if kind == 1 else 0.6)
        h[idx[gen]] |= cnt[gen]
    h[idx[h[idx] == 0]] = 1                                          # every chosen entry is seen
    if kind == 3:
        h[idx[0]] = (h[idx[0]] & PR.PROMPT_BIT) | np.uint32(SAT)
    return h


def _bias_for(rng, V, logits):
    """Ban the row's largest finite logit, push two others."""
    with np.errstate(invalid="ignore"):
        top = int(np.argmax(np.where(np.isfinite(logits), logits, -np.inf)))
    lb = {top: float("-inf")}
    for t in rng.choice(V, size=min(2, V - 1), replace=False):
        if int(t) != top:
            lb[int(t)] = float(np.float32(rng.uniform(-4, 4)))
    return lb


# (temperature, top_k, top_p, min_p, repetition, presence, frequency, bias?)
REQUESTS = [
    (0.8, 0, 1.0, 0.0, 1.3, 0.0, 0.0, False),        # each penalty alone
    (0.8, 0, 1.0, 0.0, 1.0, 0.7, 0.0, False),
    (1.0, 0, 1.0, 0.0, 1.0, 0.0, 0.4, False),
    (0.8, 0, 1.0, 0.0, 1.0, 0.0, 0.0, True),
    (0.9, 0, 1.0, 0.0, 1.2, 0.5, 0.25, True),        # all together
    (0.0, 0, 1.0, 0.0, 1.5, 0.6, 0.3, True),         # greedy with penalties
    (0.0, 0, 1.0, 0.0, 1.3, 0.0, 0.0, False),
    (0.7, 40, 1.0, 0.0, 1.3, 0.0, 0.2, False),       # with top-k, top-p, min-p on
    (0.9, 0, 0.9, 0.0, 1.0, 0.4, 0.0, True),
    (1.1, 0, 1.0, 0.05, 1.4, 0.0, 0.0, False),
    (0.8, 40, 0.8, 0.02, 1.25, 0.3, 0.1, True),
    (0.7, 0, 1.0, 0.0, 0.8, -0.5, -0.1, False),      # the signs the definitions allow: r < 1, negative presence / frequency
]


def _to_dev(dev, a):
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev)


def _run(dev, logits, hist, pos, params, streams, observe=False, penalised=True, cache_len=2 ** 31 - 1):
    """One launch: (tok, kept, logits after, history after).  penalised False: plain mq_sample on the same logits."""
    from mobilequant_amd import ops
    rows, V = logits.shape
    lg, h = _to_dev(dev, logits), _to_dev(dev, hist)
    tok = torch.full((rows,), -7, dtype=torch.int64, device=dev)
    kept = torch.full((rows,), -7, dtype=torch.int32, device=dev)
    ps = torch.tensor(pos, dtype=torch.int32, device=dev)
    if penalised:
        bias = [None if p.logit_bias is None else torch.from_numpy(PR.dense_bias(V, p.logit_bias)).to(dev) for p in params]
        ops.sample(lg, ps, (params, streams), tok, kept=kept, cache_len=cache_len, penalties=params, history=h,
                   bias=bias if any(b is not None for b in bias) else None, observe=observe)
    else:
        ops.sample(lg, ps, (params, streams), tok, kept=kept, cache_len=cache_len)
    torch.cuda.synchronize()
    return tok.cpu().numpy(), kept.cpu().numpy(), lg.cpu().numpy(), h.cpu().numpy().view(np.uint32)


def _transformed(logits, hist, params):
    V = logits.shape[1]
    return np.stack([PR.transform(logits[r], hist[r], p.repetition_penalty, p.presence_penalty, p.frequency_penalty, PR.dense_bias(V, p.logit_bias))
                     for r, p in enumerate(params)])


# ---- 1. the kernel against the reference -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 3, 8])
@pytest.mark.parametrize("V", [4, 4096, 4100, 32768, 32772])
def test_penalised_tokens_are_the_reference_and_the_plain_kernel_on_transformed_logits(dev, V, rows):
    """V: the minimum, both sides of the scan-launch threshold (4 096) and of the LDS-resident limit (32 768).  Every request of REQUESTS
    at every (V, rows), a row per request; histories of the four kinds in turn.  tok == sampling_ref(transform(l, h)) and (tok, kept)
    == mq_sample on the transformed logits uploaded as they are.  Neither the logits nor (observe = 0) the histories change."""
    from mobilequant_amd import SamplingParams
    rng = np.random.default_rng(7000 + 8 * V + rows)
    draw = undecidable = 0
    for start in range(0, len(REQUESTS), rows):
        reqs = [REQUESTS[(start + r) % len(REQUESTS)] for r in range(rows)]
        logits = np.stack([_logits(rng, V, plus_inf=(q[1] == 0 and q[2] == 1.0 and q[3] == 0.0)) for q in reqs])
        hist = np.stack([_history(rng, V, (draw + r) % 4, logits[r]) for r in range(rows)])
        pos = [int(rng.integers(0, 100_000)) for _ in range(rows)]
        seeds = [int(rng.integers(0, 2 ** 63)) for _ in range(rows)]
        streams = [int(rng.integers(0, 2 ** 63)) * 2 + 1 for _ in range(rows)]
        params = [SamplingParams(temperature=t, top_k=k, top_p=p, min_p=m, seed=s, repetition_penalty=rp, presence_penalty=a, frequency_penalty=f,
                                 logit_bias=_bias_for(rng, V, logits[r]) if b else None)
                  for r, ((t, k, p, m, rp, a, f, b), s) in enumerate(zip(reqs, seeds))]
        tok, kept, lg_after, h_after = _run(dev, logits, hist, pos, params, streams)
        assert np.array_equal(lg_after.view(np.uint32), logits.view(np.uint32))
        assert np.array_equal(h_after, hist)
        l3 = _transformed(logits, hist, params)
        plain = [SamplingParams(temperature=p.temperature, top_k=p.top_k, top_p=p.top_p, min_p=p.min_p, seed=p.seed) for p in params]
        tok_t, kept_t, _, _ = _run(dev, l3, hist, pos, plain, streams, penalised=False)
        assert np.array_equal(tok, tok_t) and np.array_equal(kept, kept_t), (V, rows, start, tok, tok_t, kept, kept_t)
        with np.errstate(all="ignore"):
            for r, p in enumerate(params):
                a = R.analyse(l3[r], p.temperature, p.top_k, p.top_p, p.min_p, p.seed, streams[r], pos[r])
                undecidable += not a["decidable"]
                print(f"V={V} rows={rows} request={(start + r) % len(REQUESTS)} tok={int(tok[r])} reference={a['token']} decidable={a['decidable']}")
                assert int(tok[r]) == a["token"], (V, rows, r, reqs[r], int(tok[r]), a["token"], a["decidable"])
        draw += rows
    print(f"V={V} rows={rows}: {draw} draws, {undecidable} inside the reference's own fp32 band")


def test_the_penalties_decide_draws(dev):
    """The inputs of the test above are not vacuous: on the same logits the penalised greedy token differs from the plain one."""
    from mobilequant_amd import SamplingParams
    rng = np.random.default_rng(11)
    V = 4100
    logits = np.stack([_logits(rng, V, False) for _ in range(3)])
    hist = np.stack([_history(rng, V, k, logits[k]) for k in range(3)])
    pen = [SamplingParams(temperature=0.0, repetition_penalty=1.5), SamplingParams(temperature=0.0, presence_penalty=3.0),
           SamplingParams(temperature=0.0, logit_bias=_bias_for(rng, V, logits[2]))]
    tok, _, _, _ = _run(dev, logits, hist, [0, 1, 2], pen, [0, 1, 2])
    base, _, _, _ = _run(dev, logits, hist, [0, 1, 2], [SamplingParams(temperature=0.0)] * 3, [0, 1, 2], penalised=False)
    assert (tok != base).all(), (tok, base)
    assert tok.tolist() == [int(np.argmax(np.nan_to_num(x, nan=-np.inf))) for x in _transformed(logits, hist, pen)]


# ---- 2. a neutral request is mq_sample, bit for bit -------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [4, 4100, 32772])
def test_neutral_rows_draw_what_mq_sample_draws_and_nothing_is_written(dev, V):
    from mobilequant_amd import SamplingParams, ops
    rng = np.random.default_rng(300 + V)
    sps = [SamplingParams(temperature=0.0), SamplingParams(temperature=0.8, seed=3), SamplingParams(temperature=0.7, top_k=40, top_p=0.9, seed=4),
           SamplingParams(temperature=1.2, min_p=0.05, seed=5), SamplingParams(temperature=0.9, top_p=0.5, seed=6)]
    rows = len(sps)
    logits = np.stack([_logits(rng, V, plus_inf=(r == 0)) for r in range(rows)])
    logits[:, V - 1] = -0.0
    hist = np.stack([_history(rng, V, r % 4, logits[r]) for r in range(rows)])
    pos, streams = [5, 6, 7, 8, 9], [1, 2, 3, 4, 5]
    lg, h = _to_dev(dev, logits), _to_dev(dev, hist)
    ps = torch.tensor(pos, dtype=torch.int32, device=dev)
    out = []
    for penalised in (False, True):
        tok = torch.full((rows,), -7, dtype=torch.int64, device=dev)
        kept = torch.full((rows,), -7, dtype=torch.int32, device=dev)
        lp = torch.full((rows,), 7.0, dtype=torch.float32, device=dev)
        kw = dict(penalties=sps, history=h, observe=False) if penalised else {}
        ops.sample(lg, ps, (sps, streams), tok, kept=kept, logprob=lp, **kw)
        out.append((tok.cpu().numpy(), kept.cpu().numpy(), lp.cpu().numpy().view(np.uint32)))
    for a, b in zip(*out):
        assert np.array_equal(a, b), (V, a, b)
    assert lg.cpu().numpy().tobytes() == logits.tobytes()
    assert np.array_equal(h.cpu().numpy().view(np.uint32), hist)
    # a neutral row among penalised ones draws the same token: a row's draw is its own
    mixed = [sps[0], SamplingParams(temperature=0.8, seed=3, repetition_penalty=1.3), sps[2], SamplingParams(temperature=1.2, min_p=0.05, seed=5, presence_penalty=0.5), sps[4]]
    tok_m, kept_m, _, _ = _run(dev, logits, hist, pos, mixed, streams)
    for r in (0, 2, 4):
        assert tok_m[r] == out[0][0][r] and kept_m[r] == out[0][1][r]


# ---- 3. observe and the prompt bits ----------------------------------------------------------------------------------------------------
def test_observe_counts_the_drawn_token_only_saturates_and_spares_idle_rows(dev):
    from mobilequant_amd import SamplingParams
    rng = np.random.default_rng(21)
    V, rows = 4100, 6
    logits = np.stack([_logits(rng, V, False) for _ in range(rows)])
    hist = np.stack([_history(rng, V, r % 4, logits[r]) for r in range(rows)])
    big = float(np.float32(1000.0))
    logits[0, 17] = logits[1, 33] = logits[4, 4099] = 0.5
    hist[0, 17] = SAT | (1 << 31)                                    # row 0 draws token 17 (bias), whose count is saturated
    hist[1, 33] = (1 << 31) | 2                                      # row 1 draws token 33: prompt bit and count 2 -> 3
    hist[4, 4099] = 0                                                # row 4 draws the last entry, never seen -> 1
    sps = [SamplingParams(temperature=0.0, logit_bias={17: big}), SamplingParams(temperature=0.9, top_k=5, seed=2, logit_bias={33: big}),
           SamplingParams(temperature=0.8, seed=3, repetition_penalty=1.3), SamplingParams(temperature=0.8, seed=4, frequency_penalty=0.5),
           SamplingParams(temperature=0.0, logit_bias={4099: big}), SamplingParams(temperature=0.7, seed=5)]     # the last one neutral: counted too
    pos = [3, 9, 16, -1, 15, 0]                                      # cache_len 16: rows 2 and 3 are idle
    tok, _, lg_after, h_after = _run(dev, logits, hist, pos, sps, list(range(rows)), observe=True, cache_len=16)
    assert tok[0] == 17 and tok[1] == 33 and tok[4] == 4099 and tok[2] == -7 and tok[3] == -7
    want = hist.copy()
    for r in (0, 1, 4, 5):
        PR.observe(want[r], int(tok[r]))
    assert want[0, 17] == (SAT | (1 << 31)) and want[1, 33] == ((1 << 31) | 3) and want[4, 4099] == 1
    assert np.array_equal(h_after, want)
    assert np.array_equal(lg_after.view(np.uint32), logits.view(np.uint32))
    # observe = 0 draws the same tokens and leaves the histories alone
    tok0, _, _, h0 = _run(dev, logits, hist, pos, sps, list(range(rows)), observe=False, cache_len=16)
    assert np.array_equal(tok0, tok) and np.array_equal(h0, hist)


def test_history_prompt_marks_ids_like_a_numpy_loop(dev):
    import ctypes
    from mobilequant_amd import _lib, ops
    rng = np.random.default_rng(8)
    V = 4100
    h0 = np.stack([_history(rng, V, 2, rng.standard_normal(V).astype(np.float32)) for _ in range(3)])
    ids = [5, 4099, 0, 5, 5, 77, 4099] + rng.integers(0, V, size=300).tolist()
    for clear in (True, False):
        h = _to_dev(dev, h0)
        ops.sample_history_prompt(h[1], ids, clear=clear)
        torch.cuda.synchronize()
        want = h0.copy()
        if clear:
            want[1] = 0
        PR.prompt_history(V, ids, want[1])
        assert np.array_equal(h.cpu().numpy().view(np.uint32), want), clear             # the rows around it are untouched
    h = _to_dev(dev, h0)
    ops.sample_history_prompt(h[2], [], clear=True)                                     # no ids: the clear alone
    assert not h[2].any() and np.array_equal(h[:2].cpu().numpy().view(np.uint32), h0[:2])
    for bad in ([V], [-1], [3, V + 7]):
        with pytest.raises(ValueError):
            ops.sample_history_prompt(h[0], bad)
    # the C entry takes device ids and checks none of them on the host: ids outside [0, V) are ignored by the kernel
    h = _to_dev(dev, h0)
    raw = torch.tensor([-1, V, 9, V + 5, -(2 ** 40), 2 ** 40, 9], dtype=torch.int64, device=dev)
    _lib.call("mq_sample_history_prompt", h[0].data_ptr(), V, raw.data_ptr(), raw.numel(), 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    want = h0.copy()
    want[0, 9] |= PR.PROMPT_BIT
    assert np.array_equal(h.cpu().numpy().view(np.uint32), want)
    assert ctypes.sizeof(_lib.MqSamplePenaltyRow) == 16


# ---- 4. the engines ------------------------------------------------------------------------------------------------------------------
VOCAB = 4160                                         # above 4 096: the selection runs both of its launches
NEW = 12


def _toy(dev, constant_embedding=False, seed=11):
    """The batched-decode tests' random model (TinyLlama geometry, reduced) through the reference's surgery, with a vocabulary of 4 160.
    lm_head is scaled down for a flat next-token distribution (sampled continuations then differ between seeds).  constant_embedding:
    every token embeds alike, so every step sees the same input and the logits barely move: plain greedy repeats one token for ever."""
    import mobilequant_amd as mq
    from mobilequant_amd.calibration import get_act_range
    from mobilequant_amd.llama import LlamaForCausalLM, LlamaShape
    shape = LlamaShape(layers=2, max_pos=1024, hidden=256, heads=32, kv_heads=4, head_dim=64, ffn=512, vocab=VOCAB)
    m = LlamaForCausalLM(shape)
    m.reset_parameters(seed=seed, std=0.08)
    with torch.no_grad():
        if constant_embedding:
            m.embed_tokens.weight.copy_(m.embed_tokens.weight[:1].expand_as(m.embed_tokens.weight).clone())
        else:
            m.lm_head.weight.mul_(0.05)
    m = m.to(dev).eval().requires_grad_(False)
    g = torch.Generator().manual_seed(5)
    act = get_act_range(m, [torch.randint(0, shape.vocab, (1, 48), generator=g) for _ in range(2)])
    mq.create_sim_qmodel(m, mq.QuantConfig(bitwidth=8, is_per_channel=False), mq.QuantConfig(bitwidth=8))
    for n, mod in m.named_modules():
        if isinstance(mod, mq.QLinear):
            if "w2" in n:
                mod.weight_quantizer.qcfg.is_per_channel = True
                mod.output_quantizer.qcfg.bitwidth = 16
            elif "o_proj" in n:
                mod.output_quantizer.qcfg.bitwidth = 16
        elif isinstance(mod, (mq.QRMSNorm, mq.QLayerNorm)):
            mod.input_quantizer.qcfg.bitwidth = 16
            mod.weight_quantizer.qcfg.bitwidth = 16
            mod.weight_quantizer.qcfg.is_symmetric = False
            mod.weight_quantizer.qcfg.is_per_channel = False
        elif isinstance(mod, mq.QMatMul):
            if "qk_bmm" in n:
                mod.output_quantizer.qcfg.bitwidth = 16
            if "pv_bmm" in n:
                mod.input_quantizer.qcfg.bitwidth = 16
    mq.set_scale_and_offset(m, act, "buffer")
    return m


@pytest.fixture(scope="module")
def toy(dev):
    return _toy(dev)


def _prompts(lens, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, VOCAB, (n,), generator=g).tolist() for n in lens]


def _host_loop(eng, prompt, sp, stream, new):
    """The reference, step by step, on the logits the engine holds in front of every draw, with the history kept on the host."""
    eng.reset()
    if len(prompt) > 1:
        eng.prefill(prompt)
    else:
        eng.step(prompt[0])
    hist = PR.prompt_history(VOCAB, prompt)
    bias = PR.dense_bias(VOCAB, sp.logit_bias)
    seq, undecidable = list(prompt), 0
    for k in range(new):
        l3 = PR.transform(eng.logits.cpu().numpy().reshape(-1), hist, sp.repetition_penalty, sp.presence_penalty, sp.frequency_penalty, bias)
        with np.errstate(all="ignore"):
            a = R.analyse(l3, sp.temperature, sp.top_k, sp.top_p, sp.min_p, sp.seed, stream, len(seq))
        undecidable += not a["decidable"]
        PR.observe(hist, a["token"])
        seq.append(a["token"])
        if k + 1 < new:
            eng.step(a["token"])
    return seq, undecidable


PENALISED = dict(temperature=0.8, top_k=40, repetition_penalty=1.3, presence_penalty=0.2, frequency_penalty=0.1, logit_bias={7: 1.5, 11: float("-inf")}, seed=77)


@pytest.mark.parametrize("launches", [4, 5])
def test_generate_is_the_reference_host_loop_on_the_engines_own_logits(dev, toy, launches):
    from mobilequant_amd import SamplingParams
    from mobilequant_amd.decode import DecodeEngine
    eng = DecodeEngine(toy, cache_len=128, launches=launches)
    assert eng.launches == launches
    prompt = _prompts([9], seed=4)[0] + [11, 7]                       # the banned and the pushed token are in the prompt too
    cases = [(SamplingParams(**PENALISED), 5), (SamplingParams(temperature=0.0, repetition_penalty=1.3, frequency_penalty=0.5), 0),
             (SamplingParams(temperature=0.9, presence_penalty=0.6, seed=3), 2)]
    want = []
    for sp, stream in cases:
        seq, undecidable = _host_loop(eng, prompt, sp, stream, NEW)
        print(f"launches={launches} stream={stream}: {undecidable} of {NEW} draws inside the reference's own fp32 band")
        want.append(seq)
    assert all(11 not in w[len(prompt):] for w in want[:1])
    got = [eng.generate(prompt, NEW, sampling=sp, stream=st) for sp, st in cases]
    assert got == want
    assert eng.logits.shape[-1] == VOCAB
    eng.capture()
    assert [eng.generate(prompt, NEW, sampling=sp, stream=st) for sp, st in cases] == want          # one graph replay per token
    assert eng.generate(prompt, NEW, sampling=cases[0][0], stream=5, prefill=False) == want[0]
    # a caller who drives sample_step() gives the history with observe_history
    eng.reset()
    eng.prefill(prompt)
    eng.set_sampling(cases[0][0], 5).observe_history(prompt)
    seq = list(prompt)
    for _ in range(NEW - 1):
        eng.sample_step()
        seq.append(int(eng.tok.item()))
    eng.sample()
    seq.append(int(eng.tok.item()))
    assert seq == want[0]


def test_a_captured_engine_switches_between_neutral_and_penalised_requests(dev, toy):
    from mobilequant_amd import SamplingParams
    from mobilequant_amd.decode import DecodeEngine
    prompt = _prompts([17], seed=6)[0]
    neutral, pen = SamplingParams(temperature=0.8, top_k=40, seed=77), SamplingParams(**PENALISED)
    eager = DecodeEngine(toy, cache_len=128)
    want_n, want_p = eager.generate(prompt, NEW, sampling=neutral, stream=1), eager.generate(prompt, NEW, sampling=pen, stream=1)
    assert want_n != want_p
    eng = DecodeEngine(toy, cache_len=128).capture()
    for _ in range(2):
        assert eng.generate(prompt, NEW, sampling=neutral, stream=1) == want_n
        assert eng.generate(prompt, NEW, sampling=pen, stream=1) == want_p
    assert sorted(eng._sample_graphs) == [(0, False), (0, True)]      # a second graph was recorded, the first one kept
    assert eager.generate(prompt, NEW, sampling=neutral, stream=1) == want_n


def test_batch_generate_is_the_single_engine_per_sequence_with_penalised_and_neutral_rows_mixed(dev, toy):
    from mobilequant_amd import SamplingParams
    from mobilequant_amd.decode import DecodeEngine
    from mobilequant_amd.decode_batch import BatchDecodeEngine
    prompts = _prompts([1, 5, 17, 64, 65, 30, 9, 33], seed=12)
    sps = [SamplingParams(**PENALISED), SamplingParams(temperature=0.7, top_k=40, top_p=0.9, seed=11),
           SamplingParams(temperature=0.0, repetition_penalty=1.3), SamplingParams(temperature=0.9, seed=5, frequency_penalty=0.4, presence_penalty=0.3),
           SamplingParams(temperature=1.0, top_k=5, seed=9), SamplingParams(temperature=0.8, min_p=0.05, seed=3, logit_bias={prompts[5][0]: float("-inf"), 100: 2.0}),
           SamplingParams(temperature=0.0), SamplingParams(temperature=1.1, top_p=0.8, seed=8, repetition_penalty=1.15)]
    single = DecodeEngine(toy, cache_len=128).capture()
    want = [single.generate(p, NEW, sampling=sp, stream=i) for i, (p, sp) in enumerate(zip(prompts, sps))]
    for B in (1, 3, 8):
        for captured in (False, True):
            be = BatchDecodeEngine(toy, B, cache_len=128)
            if captured:
                be.capture()
            assert be.generate(prompts[:B], NEW, sampling=sps[:B]) == want[:B], (B, captured)
            if B > 1:                                          # permuted across the slots: every slot is reused by another sequence
                perm = [int(i) for i in np.random.default_rng(B).permutation(B)]
                got = be.generate([prompts[i] for i in perm], NEW, sampling=[sps[i] for i in perm], streams=perm)
                assert got == [want[i] for i in perm], (B, captured, perm)
            assert be.generate(prompts[:B], NEW, sampling=sps[:B]) == want[:B], (B, captured)      # a slot reused after release is a fresh one
    # a sequence that leaves at its EOS releases its slot; the others go on unchanged
    be = BatchDecodeEngine(toy, 3, cache_len=128).capture()
    eos = want[0][len(prompts[0]) + 4]
    ref = [single.generate(p, NEW, sampling=sp, stream=i, eos_token_id=eos) for i, (p, sp) in enumerate(zip(prompts[:3], sps[:3]))]
    assert len(ref[0]) < len(want[0])
    assert be.generate(prompts[:3], NEW, sampling=sps[:3], eos_token_id=eos) == ref
    # all rows neutral again: the plain entry, the same ids as before this engine ever saw a penalty
    neutral = [sps[1], sps[4], sps[6]]
    fresh = BatchDecodeEngine(toy, 3, cache_len=128).capture()
    assert be.generate(prompts[:3], NEW, sampling=neutral) == fresh.generate(prompts[:3], NEW, sampling=neutral)
    assert not be._sampler.penalized and fresh._sampler.pargs is None


def test_repetition_penalty_breaks_a_greedy_fixed_point_loop(dev):
    """A model whose tokens all embed alike sees the same input at every step: plain greedy emits one token for ever.  The reference on
    the engine's logits shows both facts -- plain greedy loops, repetition_penalty 1.3 leaves the loop -- and generate() follows it."""
    from mobilequant_amd import SamplingParams
    from mobilequant_amd.decode import DecodeEngine
    m = _toy(dev, constant_embedding=True)
    eng = DecodeEngine(m, cache_len=64)
    prompt = [3, 1000, 4000]
    plain, pen = SamplingParams(temperature=0.0), SamplingParams(temperature=0.0, repetition_penalty=1.3)
    ref_plain, _ = _host_loop(eng, prompt, plain, 0, NEW)
    ref_pen, _ = _host_loop(eng, prompt, pen, 0, NEW)
    loop = ref_plain[len(prompt):]
    assert len(set(loop)) == 1, loop                                  # the fixed point
    assert ref_pen[len(prompt):] != loop and ref_pen[len(prompt)] == loop[0] and ref_pen[len(prompt) + 1] != loop[0]
    assert eng.generate(prompt, NEW) == ref_plain == eng.generate(prompt, NEW, sampling=plain)
    got = eng.generate(prompt, NEW, sampling=pen)
    assert got == ref_pen and got != ref_plain
    eng.capture()
    assert eng.generate(prompt, NEW, sampling=pen) == ref_pen
