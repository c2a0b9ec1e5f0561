"""GPU: speculative decoding under seeded sampling (mq_sample_rows, mq_sample_history_count, DecodeEngine.sample_rows /
step_sample_tokens / generate_speculative; csrc/mq_sample.hip).

Every comparison is exact equality, logprob apart (the kernel header's bound).  Kernel: each row of a multi-row launch against a
single-row mq_sample / mq_sample_penalized call at that row's index, over a history on which the proposals in front of the row were
counted by hand, and at V = 160 against the host reference (tests/test_spec_sample_host.py on sampling_penalty_ref / sampling_ref).
Engines: generate_speculative against plain generate(sampling=...), token for token, for every kind of draft."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sampling_penalty_ref as PR  # noqa: E402
from test_spec_sample_host import count_history, rows_reference  # noqa: E402

pytestmark = pytest.mark.gpu

SAT = 0xFFFF
PROMPT = 1 << 31
STREAM = 0x1234567890
N_BASE, N_OFFSET = 1000, -3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _i32(a):
    return torch.from_numpy(np.asarray(a, dtype=np.uint32).view(np.int32))


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


# (temperature, top_k, top_p, min_p)
REQUESTS = [(0.8, 0, 1.0, 0.0), (0.9, 5, 0.8, 0.05), (0.0, 0, 1.0, 0.0)]


def _request(req, penalised, bias):
    from mobilequant_amd import SamplingParams
    t, k, p, m = req
    if not penalised:
        return SamplingParams(temperature=t, top_k=k, top_p=p, min_p=m, seed=77)
    return SamplingParams(temperature=t, top_k=k, top_p=p, min_p=m, seed=77, repetition_penalty=1.8, presence_penalty=1.5, frequency_penalty=0.7,
                          logit_bias=bias)


def _case(V, T, seed):
    """Logits [T, V], a base history, the proposals and a bias.  Tokens: A (unseen, the rows' largest logit) and S (count 65 534) are
    proposed twice each where the row count allows (d[0] == d[2]); 1 (first 4-entry block, positive logit); V - 2 (last block, negative
    logit, in the prompt only); V + 5 (matches no entry)."""
    rng = np.random.default_rng(seed)
    l = (rng.standard_normal((T, V)) * 2.0).astype(np.float32)
    A, S = 37, V // 2 + 3
    l[:, A], l[:, S], l[:, 1], l[:, V - 2] = 9.0, 8.5, 8.0, -1.5
    h = np.zeros(V, dtype=np.uint32)
    seen = np.flatnonzero(rng.random(V) < 0.05)
    h[seen] = rng.integers(1, 6, size=len(seen)).astype(np.uint32)
    h[seen[::3]] |= np.uint32(PROMPT)
    h[A], h[S], h[1], h[V - 2] = 0, np.uint32(PROMPT | (SAT - 1)), 0, np.uint32(PROMPT)
    d = {1: [], 2: [A], 5: [S, 1, S, V - 2], 8: [A, 1, A, V - 2, S, S, V + 5]}[T]
    ban = int(np.argsort(-l[0])[3])                                   # the largest ordinary logit of row 0
    bias = {ban: float("-inf"), 8: 1.5}
    return l, h, d, bias


def _by_hand(h_dev, d, j, V):
    """The base history plus d[0 .. j-1], with torch integer ops on the int32 tensor."""
    h = h_dev.clone()
    for t in d[:j]:
        if 0 <= t < V and (int(h[t]) & SAT) != SAT:
            h[t] += 1
    return h


def _single_rows(dev, lg, h_dev, d, sp, bias_row, penalised):
    """Row j alone through mq_sample / mq_sample_penalized at its index: (tokens, kept, logprob)."""
    from mobilequant_amd import ops
    T, V = lg.shape
    toks, kept, lps = [], [], []
    for j in range(T):
        tok = torch.full((1,), -7, dtype=torch.int64, device=dev)
        kp = torch.full((1,), -7, dtype=torch.int32, device=dev)
        lp = torch.full((1,), -7.0, device=dev)
        pos = torch.tensor([N_BASE + N_OFFSET + j], dtype=torch.int32, device=dev)
        if penalised:
            ops.sample(lg[j:j + 1], pos, ([sp], [STREAM]), tok, kept=kp, logprob=lp, penalties=[sp], history=_by_hand(h_dev, d, j, V).view(1, -1),
                       bias=[bias_row])
        else:
            ops.sample(lg[j:j + 1], pos, ([sp], [STREAM]), tok, kept=kp, logprob=lp)
        toks.append(int(tok)); kept.append(int(kp)); lps.append(float(lp))
    return toks, kept, lps


def _rows(dev, lg, d, sp, history=None, bias=None, n_base=N_BASE):
    from mobilequant_amd import ops
    T = lg.shape[0]
    tok = torch.full((T,), -7, dtype=torch.int64, device=dev)
    kp = torch.full((T,), -7, dtype=torch.int32, device=dev)
    lp = torch.full((T,), -7.0, device=dev)
    nb = torch.tensor([n_base], dtype=torch.int32, device=dev)
    prop = torch.tensor(d, dtype=torch.int64, device=dev) if T > 1 else None
    ops.sample_rows(lg, nb, N_OFFSET, sp, STREAM, tok, proposals=prop, history=history, bias=bias, kept=kp, logprob=lp)
    return tok.tolist(), kp.tolist(), lp.tolist()


# ---- 1. the kernel against the existing entries -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2, 5, 8])
@pytest.mark.parametrize("V", [160, 8196, 32772, 65540])
def test_every_row_draws_what_the_single_row_entries_draw_at_its_index(dev, V, T):
    l, h, d, bias = _case(V, T, seed=V + T)
    lg, h_dev = torch.from_numpy(l).to(dev), _i32(h).to(dev)
    bias_row = torch.from_numpy(PR.dense_bias(V, bias)).to(dev)
    lp_tol = 2 * (2.0 ** -23 * (2 + math.log(V)) + V / 2.0 ** 32)     # two evaluations, each within the header's bound of the exact value
    for req in REQUESTS:
        # neutral: mq_sample's token, with or without a history (the logit bits are kept)
        sp = _request(req, False, None)
        want = _single_rows(dev, lg, h_dev, d, sp, None, False)
        for hist in (None, h_dev):
            got = _rows(dev, lg, d, sp, history=hist)
            assert got[0] == want[0] and got[1] == want[1], (req, "neutral", hist is not None)
            assert all(abs(a - b) <= lp_tol + 2 * np.spacing(np.float32(abs(b))) for a, b in zip(got[2], want[2])), (req, got[2], want[2])
        # penalised: mq_sample_penalized's token from a history on which d[0 .. j-1] were counted one after the other
        sp = _request(req, True, bias)
        want = _single_rows(dev, lg, h_dev, d, sp, bias_row, True)
        got = _rows(dev, lg, d, sp, history=h_dev, bias=bias_row)
        assert got[0] == want[0] and got[1] == want[1], (req, "penalised", got, want)
        assert all(abs(a - b) <= lp_tol + 2 * np.spacing(np.float32(abs(b))) for a, b in zip(got[2], want[2])), (req, got[2], want[2])
        if V == 160:                                                   # and the host reference
            for a, tk, kp in zip(rows_reference(l, h, d, N_BASE + N_OFFSET, sp, STREAM), got[0], got[1]):
                assert a["kept_lo"] <= kp <= a["kept_hi"] and tk in a["allowed"], (req, tk, kp)
                if a["decidable"]:
                    assert tk == a["token"], (req, tk, a["token"])
    # nothing but the outputs was written
    assert np.array_equal(_u32(h_dev), h) and np.array_equal(lg.cpu().numpy().view(np.uint32), l.view(np.uint32))


def test_the_proposals_reach_the_draws_of_this_case(dev):
    """The case above is sensitive: with the proposals taken away the penalised greedy rows draw other tokens."""
    V, T = 8196, 8
    l, h, d, bias = _case(V, T, seed=V + T)
    lg, h_dev = torch.from_numpy(l).to(dev), _i32(h).to(dev)
    sp = _request(REQUESTS[2], True, None)
    with_d = _rows(dev, lg, d, sp, history=h_dev)[0]
    without = _rows(dev, lg, [V + 5] * (T - 1), sp, history=h_dev)[0]
    assert without == [37] * T and with_d[0] == 37 and with_d[1] != 37 and with_d != without, (with_d, without)


def test_a_captured_launch_follows_n_base(dev):
    from mobilequant_amd import _lib
    from mobilequant_amd._lib import MQ_SAMPLE_SCRATCH_BYTES, MqSampleRowsArgs
    from mobilequant_amd.sampling import pack_penalty_rows, pack_rows
    V, T = 8196, 5
    l, h, d, bias = _case(V, T, seed=3)
    sp = _request(REQUESTS[1], True, bias)
    lg, h_dev = torch.from_numpy(l).to(dev), _i32(h).to(dev)
    bias_row = torch.from_numpy(PR.dense_bias(V, bias)).to(dev)
    pr = torch.from_numpy(pack_rows([sp], [STREAM]).view(np.uint8).reshape(-1)).to(dev)
    pen = torch.from_numpy(pack_penalty_rows([sp]).view(np.uint8).reshape(-1)).to(dev)
    prop = torch.tensor(d, dtype=torch.int64, device=dev)
    nb = torch.tensor([N_BASE], dtype=torch.int32, device=dev)
    tok = torch.full((T,), -7, dtype=torch.int64, device=dev)
    kp = torch.full((T,), -7, dtype=torch.int32, device=dev)
    scratch = torch.zeros(MQ_SAMPLE_SCRATCH_BYTES, dtype=torch.uint8, device=dev)
    a = MqSampleRowsArgs()
    a.logits, a.logits_stride, a.V, a.rows, a.n_base, a.n_offset = lg.data_ptr(), V, V, T, nb.data_ptr(), N_OFFSET
    a.params, a.penalty, a.bias, a.history, a.proposals = pr.data_ptr(), pen.data_ptr(), bias_row.data_ptr(), h_dev.data_ptr(), prop.data_ptr()
    a.tok, a.kept, a.logprob, a.scratch, a.scratch_bytes = tok.data_ptr(), kp.data_ptr(), None, scratch.data_ptr(), MQ_SAMPLE_SCRATCH_BYTES
    launch = lambda: _lib.call("mq_sample_rows", ctypes.byref(a), torch.cuda.current_stream().cuda_stream)      # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()                                                       # outside the capture: the kernel's LDS ceiling
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    seen = []
    for base in (N_BASE, 2000):
        nb.fill_(base)
        tok.fill_(-7)
        g.replay()
        want = _rows(dev, lg, d, sp, history=h_dev, bias=bias_row, n_base=base)
        assert tok.tolist() == want[0] and kp.tolist() == want[1], base
        seen.append(tok.tolist())
    assert seen[0] != seen[1]                                          # the index reached the random numbers


# ---- 2. in-flight counts matter ---------------------------------------------------------------------------------------------------------
def test_in_flight_proposals_move_a_greedy_draw(dev):
    from mobilequant_amd import SamplingParams
    V, T = 160, 4
    a, b, c, e, x = 17, 3, 150, 64, 99
    row = np.zeros(V, dtype=np.float32)
    row[[a, b, c, e]] = [4.0, 3.0, 2.0, 1.0]
    lg = torch.from_numpy(np.tile(row, (T, 1))).to(dev)
    sp = SamplingParams(temperature=0.0, presence_penalty=4.0)
    h = torch.zeros(V, dtype=torch.int32, device=dev)
    assert _rows(dev, lg, [a, b, c], sp, history=h)[0] == [a, b, c, e]
    assert _rows(dev, lg, [a, b, c], sp)[0] == [a, b, c, e]            # no history: all zeros
    assert _rows(dev, lg, [x, x, x], sp, history=h)[0] == [a, a, a, a]
    assert int(h.abs().sum()) == 0


# ---- 3. history_count ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [160, 32772])
def test_history_count_is_the_host_loop(dev, V):
    from mobilequant_amd import ops
    rng = np.random.default_rng(V)
    h = rng.integers(0, 40, size=V).astype(np.uint32)
    h[rng.random(V) < 0.3] |= np.uint32(PROMPT)
    h[5], h[6], h[7], h[9], h[V - 1] = SAT, SAT - 1, PROMPT | SAT, PROMPT, 0
    ids = [t for t in rng.integers(0, V, size=3000).tolist() if t not in (5, 6, 7, 9, V - 1)]      # (the entries stated by hand below)
    ids += [5, 6, 6, 6, 7, 9, 9, V - 1, V - 1, V, V + 7, -1, 1 << 40, 0, 0, 0]
    ids_dev = torch.tensor(ids, dtype=torch.int64, device=dev)
    h_dev = _i32(h).to(dev)
    ops.sample_history_count(h_dev, ids_dev, 1)
    up = count_history(h.copy(), ids, 1)
    assert np.array_equal(_u32(h_dev), up)
    assert up[5] == SAT and up[6] == SAT and up[7] == PROMPT | SAT and up[9] == PROMPT | 2
    ops.sample_history_count(h_dev, ids_dev, -1)
    down = count_history(up.copy(), ids, -1)
    assert np.array_equal(_u32(h_dev), down)
    assert down[9] == PROMPT and down[6] == SAT - 3                    # bit 31 kept; no inverse at the ceiling
    ops.sample_history_count(h_dev, ids_dev, -1)                       # to the floor
    assert np.array_equal(_u32(h_dev), count_history(down.copy(), ids, -1))
    assert _u32(h_dev)[V - 1] == 0 and _u32(h_dev)[9] == PROMPT
    # away from the ceiling, + 1 then - 1 over ids with repeats restores the history bit for bit
    calm = h.copy()
    calm[(calm & SAT) > 40] &= np.uint32(PROMPT)
    c_dev = _i32(calm).to(dev)
    ops.sample_history_count(c_dev, ids_dev, 1)
    assert not np.array_equal(_u32(c_dev), calm)
    ops.sample_history_count(c_dev, ids_dev, -1)
    assert np.array_equal(_u32(c_dev), calm)
    ops.sample_history_count(c_dev, ids_dev[:0], 1)                    # no ids: nothing happens
    assert np.array_equal(_u32(c_dev), calm)


# ---- 4. the ids equal plain sampling ----------------------------------------------------------------------------------------------------
ENGINE_REQUESTS = {
    "temperature": dict(temperature=0.8, seed=5),
    "filtered": dict(temperature=0.9, top_k=12, top_p=0.9, min_p=0.02, seed=6),
    "penalised": dict(temperature=0.8, seed=7, repetition_penalty=1.8, presence_penalty=1.5, frequency_penalty=0.7, logit_bias={3: float("-inf"), 11: 1.5}),
}
CL, NEW = 128, 40


@pytest.fixture(scope="module")
def models(dev):
    from test_gpu_decode_batch import _model
    return _model(dev, "llama", 2, 8), _model(dev, "llama", 1, 8, seed=23)


@pytest.fixture(scope="module")
def engines(dev, models):
    """(target, self-draft, smaller draft) per (launches, captured), built once."""
    from mobilequant_amd.decode import DecodeEngine
    made = {}

    def get(launches, captured):
        if (launches, captured) not in made:
            m, small = models
            trio = [DecodeEngine(m, cache_len=CL, launches=launches), DecodeEngine(m, cache_len=CL, launches=launches), DecodeEngine(small, cache_len=CL)]
            if captured:
                for e in trio:
                    e.capture()
            made[(launches, captured)] = trio
        return made[(launches, captured)]
    return get


def _context(V):
    g = torch.Generator().manual_seed(12)
    base = torch.randint(0, V, (15,), generator=g).tolist()
    return base + base + base[:7]                                      # 37 tokens that repeat themselves: prompt lookup finds something


def _truth(V, ctx, out):
    h = PR.prompt_history(V, ctx)
    for t in out[len(ctx):]:
        PR.observe(h, t)
    return h


@pytest.mark.parametrize("request_name", list(ENGINE_REQUESTS))
@pytest.mark.parametrize("captured", [False, True], ids=["direct", "graph"])
@pytest.mark.parametrize("launches", [4, 5])
def test_speculative_sampling_returns_plain_samplings_ids(dev, engines, launches, captured, request_name):
    from mobilequant_amd import SamplingParams
    from mobilequant_amd.decode import prompt_lookup_draft
    eng, self_draft, small_draft = engines(launches, captured)
    V = eng.shape.vocab
    sp = SamplingParams(**ENGINE_REQUESTS[request_name])
    ctx = _context(V)
    assert len(ctx) == 37
    plain = eng.generate(ctx, NEW, sampling=sp, stream=STREAM)
    assert len(plain) == len(ctx) + NEW
    wrong = lambda ids, k: [(plain[len(ids) + i] + 1) % V if len(ids) + i < len(plain) else 0 for i in range(k)]      # noqa: E731
    fewer = lambda ids, k: plain[len(ids):len(ids) + max(k - 2, 0)]                                                # noqa: E731
    for name, draft, nd in (("self", self_draft, 4), ("small", small_draft, 4), ("wrong", wrong, 4), ("lookup", prompt_lookup_draft(3), 4),
                            ("fewer", fewer, 4), ("none", wrong, 0), ("self7", self_draft, 7)):
        got = eng.generate_speculative(ctx, NEW, draft, sampling=sp, stream=STREAM, num_draft=nd)
        assert got == plain, (name, got[len(ctx):], plain[len(ctx):])
        st = eng.spec_stats
        assert st["target_steps"] == st["rounds"] and st["accepted"] <= st["proposed"]
        assert eng.position() <= len(got)
        if name.startswith("self"):                                    # the draft's step() logits are the target's rows bit for bit, the noise is shared
            assert st["accepted"] == st["proposed"] > 0, st
            assert st["rounds"] == math.ceil((NEW - 1) / (nd + 1)), st
        if name == "wrong":
            assert st["accepted"] == 0 and st["rounds"] == NEW - 1, st
        if name == "none":
            assert st["proposed"] == 0 and st["rounds"] == NEW - 1, st
        if name == "fewer":
            assert st["accepted"] == st["proposed"] > 0, st
        if sp.penalized:
            want = _truth(V, ctx, plain)
            assert np.array_equal(_u32(eng._sampler.history[0]), want), name
            if name in ("self", "small", "self7"):
                assert np.array_equal(_u32(draft._sampler.history[0]), want), name
    # an EOS that cuts a round in the middle
    new = plain[len(ctx):]
    cut = next(i for i in (8, 7, 9, 13, 12, 14, 18) if new[i] not in new[:i])
    plain_eos = eng.generate(ctx, NEW, sampling=sp, stream=STREAM, eos_token_id=new[cut])
    assert plain_eos == plain[:len(ctx) + cut + 1]
    for draft in (self_draft, small_draft, prompt_lookup_draft(3)):
        assert eng.generate_speculative(ctx, NEW, draft, sampling=sp, stream=STREAM, num_draft=4, eos_token_id=new[cut]) == plain_eos
    # another stream is another continuation, and the speculative path follows it
    other = eng.generate(ctx, 12, sampling=sp, stream=STREAM + 1)
    assert eng.generate_speculative(ctx, 12, self_draft, sampling=sp, stream=STREAM + 1) == other


def test_engine_sample_rows_draws_the_rows_of_the_last_step_tokens_call(dev, engines):
    """sample_rows after step_tokens, step_sample_tokens as one captured graph and the functional op on the same rows agree."""
    from mobilequant_amd import SamplingParams, ops
    eng_d, eng_g = engines(4, False)[0], engines(4, True)[0]
    V = eng_d.shape.vocab
    ctx = _context(V)
    toks = [ctx[-1], 5, 9, 5, 77]
    for sp in (SamplingParams(temperature=0.8, seed=9), SamplingParams(temperature=0.8, seed=9, presence_penalty=2.0, repetition_penalty=1.4)):
        got = []
        for eng, fused in ((eng_d, False), (eng_d, True), (eng_g, False), (eng_g, True)):
            eng.set_sampling(sp, STREAM)
            eng._start_sequence(ctx[:-1], True)
            eng.observe_history(ctx)
            if fused:
                got.append(eng.step_sample_tokens(toks).tolist())
            else:
                rows = eng.step_tokens(toks)
                got.append(eng.sample_rows(len(toks)).tolist())
                if eng is eng_d:                                       # the functional op on the same rows
                    tok = torch.zeros(len(toks), dtype=torch.int64, device=dev)
                    hist = eng._sampler.history[0] if sp.penalized else None
                    ops.sample_rows(rows, eng.pos, 1 - len(toks), sp, STREAM, tok, proposals=eng.rtok[1:len(toks)].clone(), history=hist)
                    got.append(tok.tolist())
            assert eng.position() == len(ctx) - 1 + len(toks)
        assert all(g == got[0] for g in got), got
    with pytest.raises(RuntimeError, match="row count"):
        eng_d.sample_rows(3)
    eng_d.rewind(len(ctx))
    with pytest.raises(RuntimeError, match="row count"):
        eng_d.sample_rows(len(toks))
