"""GPU: speculative decoding under seeded sampling in the batched engine (mq_sample_ragged, mq_sample_history_count_ragged,
BatchDecodeEngine.sample_rows / step_sample_tokens / generate_speculative; csrc/mq_sample.hip).

Every comparison is exact equality, logprob apart (the kernel header's bound, the formula of tests/test_gpu_spec_sample.py).  The
existing entries are the oracle, and they are themselves pinned.  Kernel: every run of a ragged launch against mq_sample_rows given that
run alone (its sequence's request, history and bias, the run's first index, its proposals), and every row against a single-row
mq_sample / mq_sample_penalized call over a history on which the proposals in front of the row were counted by hand.  Engine: each
slot's rows against DecodeEngine.step_sample_tokens for that sequence alone, and generate_speculative against DecodeEngine.generate(
sampling=, stream=) per prompt and the batched generate(sampling=, streams=), token for token, for every kind of draft."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sampling_penalty_ref as PR  # noqa: E402
from test_spec_sample_host import count_history  # noqa: E402

pytestmark = pytest.mark.gpu

SAT = 0xFFFF
PROMPT = 1 << 31
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
B, CL, N_OFFSET = 4, 64, 1
STREAMS = [0x1234567890, 7, 2 ** 63 + 5, 99]
F, A = 21, 37                                                     # a run's first token; the rows' largest logit


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _i32(a):
    return torch.from_numpy(np.asarray(a, dtype=np.uint32).view(np.int32))


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _requests(V):
    """One launch mixes: 0 neutral sampled; 1 filtered (top-k / top-p / min-p) with penalties and a bias; 2 greedy with penalties;
    3 penalised with a NULL bias pointer.  Different seeds and streams per slot."""
    from mobilequant_amd import SamplingParams
    pen = dict(repetition_penalty=1.8, presence_penalty=1.5, frequency_penalty=0.7)
    return [SamplingParams(temperature=0.8, seed=11),
            SamplingParams(temperature=0.9, top_k=5, top_p=0.8, min_p=0.05, seed=12, logit_bias={8: 1.5, V - 7: float("-inf")}, **pen),
            SamplingParams(temperature=0.0, seed=13, **pen),
            SamplingParams(temperature=0.8, seed=14, **pen)]


def _proposals(V, T):
    """Behind a run's first token (tests/test_gpu_spec_sample.py's _case): A (unseen, the largest logit) and S (count 65 534) proposed
    twice each where the run is long enough; 1 (first 4-entry block); V - 2 (last block, in the prompt only); V + 5 (matches no entry)."""
    S = V // 2 + 3
    return {1: [], 2: [A], 3: [A, 1], 4: [S, 1, S], 5: [S, 1, S, V - 2], 8: [A, 1, A, V - 2, S, S, V + 5]}[T]


def _runs(table):
    """The launch's rule restated on the host: [(first row, row count)] of the live runs of a table of (sequence, position) rows."""
    runs, r = [], 0
    while r < len(table):
        s, p = table[r]
        if not (0 <= s < B and 0 <= p < CL):
            r += 1
            continue
        n = 1
        while r + n < len(table) and table[r + n] == (s, p + n) and p + n < CL:
            n += 1
        runs.append((r, n))
        r += n
    return runs


class Case:
    """Logits [R, V], the batch's histories, biases and requests, and the tokens of a table's rows."""

    def __init__(self, dev, V, table, seed=0, toks=None):
        rng = np.random.default_rng(1000 * V + seed)
        self.dev, self.V, self.table, self.R = dev, V, list(table), len(table)
        S = V // 2 + 3
        l = (rng.standard_normal((self.R, V)) * 2.0).astype(np.float32)
        l[:, A], l[:, F], l[:, S], l[:, 1], l[:, V - 2] = 9.0, 8.9, 8.5, 8.0, -1.5
        h = np.zeros((B, V), dtype=np.uint32)
        for s in range(B):
            seen = np.flatnonzero(rng.random(V) < 0.05)
            h[s, seen] = rng.integers(1, 6, size=len(seen)).astype(np.uint32)
            h[s, seen[::3]] |= np.uint32(PROMPT)
            h[s, A], h[s, F], h[s, S], h[s, 1], h[s, V - 2] = 0, 0, np.uint32(PROMPT | (SAT - 1)), 0, np.uint32(PROMPT)
        self.sp = _requests(V)
        self.l, self.h = l, h
        tok = np.full(self.R, A, dtype=np.int64)                   # idle rows and single-row runs: a token that would matter if counted
        for r0, n in _runs(self.table):
            if n > 1:
                tok[r0:r0 + n] = [F] + _proposals(V, n)
        self.tok = tok if toks is None else np.asarray(toks, dtype=np.int64)
        self.lg, self.hd = torch.from_numpy(l).to(dev), _i32(h).to(dev)
        self.bias = [torch.from_numpy(PR.dense_bias(V, p.logit_bias)).to(dev) if p.logit_bias is not None else None for p in self.sp]
        self.rt = torch.from_numpy(self.tok).to(dev)

    def tables(self, table=None):
        t = self.table if table is None else table
        return (torch.tensor([s for s, _ in t], dtype=torch.int32, device=self.dev), torch.tensor([p for _, p in t], dtype=torch.int32, device=self.dev))

    def ragged(self, table=None):
        from mobilequant_amd import ops
        seq, pos = self.tables(table)
        out = (torch.full((self.R,), -7, dtype=torch.int64, device=self.dev), torch.full((self.R,), -7, dtype=torch.int32, device=self.dev),
               torch.full((self.R,), -7.0, device=self.dev))
        snap = [t.clone() for t in (self.lg, self.hd, seq, pos, self.rt)]
        ops.sample_ragged(self.lg, seq, pos, self.rt, N_OFFSET, (self.sp, STREAMS), out[0], cache_len=CL, history=self.hd, bias=self.bias,
                          kept=out[1], logprob=out[2])
        for a, b in zip(snap, (self.lg, self.hd, seq, pos, self.rt)):
            assert torch.equal(a, b)                               # nothing but the outputs was written
        return out[0].tolist(), out[1].tolist(), out[2].tolist()

    def run_alone(self, r0, n, proposals=None):
        """mq_sample_rows given the run alone: (tokens, kept, logprob)."""
        from mobilequant_amd import ops
        s, p = self.table[r0]
        sp = self.sp[s]
        tok = torch.full((n,), -7, dtype=torch.int64, device=self.dev)
        kp = torch.full((n,), -7, dtype=torch.int32, device=self.dev)
        lp = torch.full((n,), -7.0, device=self.dev)
        prop = (self.rt[r0 + 1:r0 + n].clone() if proposals is None else torch.tensor(proposals, dtype=torch.int64, device=self.dev)) if n > 1 else None
        ops.sample_rows(self.lg[r0:r0 + n], torch.tensor([p], dtype=torch.int32, device=self.dev), N_OFFSET, sp, STREAMS[s], tok, proposals=prop,
                        history=self.hd[s], bias=self.bias[s], kept=kp, logprob=lp)
        return tok.tolist(), kp.tolist(), lp.tolist()

    def row_alone(self, r, j):
        """Row r (at distance j from its run's first row) through mq_sample / mq_sample_penalized from the history counted by hand."""
        from mobilequant_amd import ops
        s, p = self.table[r]
        sp = self.sp[s]
        tok = torch.full((1,), -7, dtype=torch.int64, device=self.dev)
        kp = torch.full((1,), -7, dtype=torch.int32, device=self.dev)
        lp = torch.full((1,), -7.0, device=self.dev)
        pos = torch.tensor([p + N_OFFSET], dtype=torch.int32, device=self.dev)
        if not sp.penalized:
            ops.sample(self.lg[r:r + 1], pos, ([sp], [STREAMS[s]]), tok, kept=kp, logprob=lp)
        else:
            h = self.hd[s].clone()
            for t in self.tok[r - j + 1:r + 1].tolist():
                if 0 <= t < self.V and (int(h[t]) & SAT) != SAT:
                    h[t] += 1
            ops.sample(self.lg[r:r + 1], pos, ([sp], [STREAMS[s]]), tok, kept=kp, logprob=lp, penalties=[sp], history=h.view(1, -1), bias=[self.bias[s]])
        return int(tok), int(kp)


def _run(s, p, n):
    return [(s, p + i) for i in range(n)]


IDLE = (-1, CL)
PLANS = {
    "8x1": [(0, 5), (1, 9), (2, 3), (3, 20), (0, 30), (1, 31), (2, 40), (3, 50)],
    "1x8": _run(2, 10, 8),
    "1x8 filtered": _run(1, 3, 8),
    "1+2+5": [(0, 4)] + _run(3, 8, 2) + _run(1, 20, 5),
    "1+2+5 greedy": [(3, 4)] + _run(0, 8, 2) + _run(2, 20, 5),
    "idle before, between and after": [IDLE] + _run(2, 10, 3) + [IDLE] + _run(1, 30, 2) + [IDLE],
    "equal positions on different slots": [(1, 7), (2, 7), (3, 7), (2, 8), (1, 8), (0, 7)],
    "rising positions on different slots": [(1, 10), (2, 11), (3, 12), (1, 13), (2, 14)],
    "a run ends at the cache end": _run(2, CL - 3, 3) + [(2, CL)],
    "sequences and positions out of range": [(-1, 5), (B, 6), (INT_MIN, 7), (INT_MAX, 8), (1, -1), (1, CL), (1, 0), (1, 1)],
    "out of range inside a run": _run(3, 30, 2) + [(3, INT_MAX)] + _run(3, 33, 2) + [(B, 35), (3, 36)],
}


# ---- 1. the kernel against mq_sample_rows per run, and against the single-row entries ---------------------------------------------
@pytest.mark.parametrize("V", [160, 4096, 4100])      # the one-launch form, its boundary, the two-launch form
def test_every_run_draws_what_mq_sample_rows_draws_for_it_alone(dev, V):
    lp_tol = 2 * (2.0 ** -23 * (2 + math.log(V)) + V / 2.0 ** 32)     # two evaluations, each within the header's bound of the exact value
    for name, table in PLANS.items():
        c = Case(dev, V, table)
        tok, kept, lp = c.ragged()
        live = set()
        for r0, n in _runs(table):
            want = c.run_alone(r0, n)
            assert tok[r0:r0 + n] == want[0] and kept[r0:r0 + n] == want[1], (name, r0, n, tok, want)
            assert all(abs(a - b) <= lp_tol + 2 * np.spacing(np.float32(abs(b))) for a, b in zip(lp[r0:r0 + n], want[2])), (name, r0, lp, want[2])
            live.update(range(r0, r0 + n))
            if name.startswith("1+2+5") or V == 160:
                for j in range(n):
                    assert (tok[r0 + j], kept[r0 + j]) == c.row_alone(r0 + j, j), (name, r0, j)
        for r in range(c.R):
            if r not in live:                                      # idle rows keep their bytes
                assert (tok[r], kept[r], lp[r]) == (-7, -7, -7.0), (name, r)
    # the plans are what their names say
    assert _runs(PLANS["sequences and positions out of range"]) == [(6, 2)] and _runs(PLANS["a run ends at the cache end"]) == [(0, 3)]
    assert _runs(PLANS["out of range inside a run"]) == [(0, 2), (3, 2), (6, 1)] and len(_runs(PLANS["rising positions on different slots"])) == 5


def test_the_case_is_sensitive_to_runs_slots_and_the_first_token(dev):
    """Otherwise the equalities above show nothing: the greedy penalised slot's draws follow what is counted."""
    from mobilequant_amd import ops
    V = 160
    table = PLANS["1+2+5 greedy"]                                  # slot 3 alone, a run of slot 0, a run of 5 of slot 2 (greedy, penalised)
    toks = [A, F, A, F, A, 1, A, V - 2]
    c = Case(dev, V, table, toks=toks)
    tok = c.ragged()[0]
    run = tok[3:8]
    assert run[0] == A and run[1] == F, run                        # A until it is counted; F, the run's first token, is never counted
    assert run == c.run_alone(3, 5)[0]
    # the run's rows presented as single-row runs (falling positions): the same indices, no proposal counted
    back = table[:3] + table[3:][::-1]
    c2 = Case(dev, V, back, toks=toks[:3] + toks[3:][::-1])
    c2.lg = torch.cat([c.lg[:3], c.lg[3:].flip(0)]).contiguous()
    broken = c2.ragged()[0]
    assert _runs(back) == [(0, 1), (1, 2)] + [(r, 1) for r in range(3, 8)]
    assert broken[:3] == tok[:3] and broken[3:] == [A] * 5 and broken[3:][::-1] != run, (broken, tok)
    # two slots swapped in row_seq: other requests, other histories; slot 0's rows stay
    swap = {2: 3, 3: 2}
    swapped = c.ragged(table=[(swap.get(s, s), p) for s, p in table])[0]
    assert swapped != tok and swapped[1:3] == tok[1:3], (swapped, tok)
    # the run's first token counted as a proposal (mq_sample_rows over the run behind one more row): another draw
    shifted = torch.cat([c.lg[3:4], c.lg[3:8]]).contiguous()
    out = torch.full((6,), -7, dtype=torch.int64, device=dev)
    ops.sample_rows(shifted, torch.tensor([table[3][1] - 1], dtype=torch.int32, device=dev), N_OFFSET, c.sp[2], STREAMS[2], out,
                    proposals=c.rt[3:8].clone(), history=c.hd[2])
    assert out.tolist()[1:] != run and out.tolist()[2] != F, (out.tolist(), run)
    # a neutral sequence keeps the bits of its logits: its rows do not see the proposals at all
    neutral = Case(dev, V, _run(0, 10, 8))
    assert neutral.ragged()[0] == [neutral.row_alone(r, 0)[0] for r in range(8)]


def test_a_captured_launch_follows_the_table_the_tokens_and_the_requests(dev):
    from mobilequant_amd import _lib
    from mobilequant_amd._lib import MQ_SAMPLE_SCRATCH_BYTES, MqSampleRaggedArgs
    from mobilequant_amd.sampling import pack_penalty_rows, pack_rows
    V, R = 4100, 5
    first, second = [(0, 4)] + _run(2, 8, 4), _run(1, 40, 3) + [IDLE, (3, 9)]
    c = Case(dev, V, first)
    seq, pos = c.tables()
    rt = c.rt.clone()
    pr = torch.from_numpy(pack_rows(c.sp, STREAMS).view(np.uint8).reshape(-1)).to(dev)
    pen = torch.from_numpy(pack_penalty_rows(c.sp).view(np.uint8).reshape(-1)).to(dev)
    bias_ptr = torch.tensor([0 if b is None else b.data_ptr() for b in c.bias], dtype=torch.int64, device=dev)
    tok = torch.full((R,), -7, dtype=torch.int64, device=dev)
    kp = torch.full((R,), -7, dtype=torch.int32, device=dev)
    scratch = torch.zeros(MQ_SAMPLE_SCRATCH_BYTES, dtype=torch.uint8, device=dev)
    a = MqSampleRaggedArgs()
    a.logits, a.logits_stride, a.V, a.rows, a.batch, a.cache_len = c.lg.data_ptr(), V, V, R, B, CL
    a.row_seq, a.row_pos, a.n_offset, a.row_tok, a.params = seq.data_ptr(), pos.data_ptr(), N_OFFSET, rt.data_ptr(), pr.data_ptr()
    a.penalty, a.history, a.history_stride, a.bias = pen.data_ptr(), c.hd.data_ptr(), V, bias_ptr.data_ptr()
    a.tok, a.kept, a.logprob, a.scratch, a.scratch_bytes = tok.data_ptr(), kp.data_ptr(), None, scratch.data_ptr(), MQ_SAMPLE_SCRATCH_BYTES
    launch = lambda: _lib.call("mq_sample_ragged", ctypes.byref(a), torch.cuda.current_stream().cuda_stream)      # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()                                                   # outside the capture: the kernel's LDS ceiling
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    tok.fill_(-7)
    g.replay()
    want = c.ragged()
    assert tok.tolist() == want[0] and kp.tolist() == want[1]
    # another plan, other tokens and the requests of slots 1 and 3 exchanged, all rewritten in device memory
    c2 = Case(dev, V, second)
    c2.lg, c2.hd, c2.bias = c.lg, c.hd, [c.bias[0], None, c.bias[2], c.bias[1]]
    c2.sp = [c.sp[0], c.sp[3], c.sp[2], c.sp[1]]
    s2, p2 = c2.tables()
    seq.copy_(s2), pos.copy_(p2), rt.copy_(c2.rt)
    pr.copy_(torch.from_numpy(pack_rows(c2.sp, STREAMS).view(np.uint8).reshape(-1)))
    pen.copy_(torch.from_numpy(pack_penalty_rows(c2.sp).view(np.uint8).reshape(-1)))
    bias_ptr.copy_(torch.tensor([0 if b is None else b.data_ptr() for b in c2.bias], dtype=torch.int64))
    tok.fill_(-7), kp.fill_(-7)
    g.replay()
    want2 = c2.ragged()
    assert tok.tolist() == want2[0] and kp.tolist() == want2[1] and want2[0] != want[0]
    assert tok.tolist()[3] == -7                                   # the idle row of the new plan


# ---- 2. history_count_ragged ----------------------------------------------------------------------------------------------------------
def test_history_count_ragged_is_the_host_loop(dev):
    from mobilequant_amd import ops
    V, NB = 160, 3
    rng = np.random.default_rng(5)
    h = rng.integers(0, 40, size=(NB, V)).astype(np.uint32)
    h[rng.random((NB, V)) < 0.3] |= np.uint32(PROMPT)
    h[1, 5], h[1, 6], h[1, 7], h[1, 9], h[2, V - 1], h[0, 5] = SAT, SAT - 1, PROMPT | SAT, PROMPT, 0, 3
    stated = {(1, 5), (1, 6), (1, 7), (1, 9), (2, V - 1), (0, 5)}
    pairs = [(int(s), int(t)) for s, t in zip(rng.integers(0, NB, size=2000), rng.integers(0, V, size=2000)) if (int(s), int(t)) not in stated]
    pairs += [(1, 5), (1, 6), (1, 6), (1, 6), (1, 7), (1, 9), (1, 9), (2, V - 1), (2, V - 1), (0, 5),
              (0, V), (1, V + 7), (2, -1), (0, 1 << 40), (-1, 5), (NB, 5), (1 << 40, 5), (INT_MIN, 0), (INT_MAX, 0)]
    pd = torch.tensor(pairs, dtype=torch.int64, device=dev)
    hd = _i32(h).to(dev)

    def host(hh, delta):
        for s in range(NB):
            count_history(hh[s], [t for q, t in pairs if q == s], delta)
        return hh
    assert ops.sample_history_count_ragged(hd, pd, 1) is hd
    up = host(h.copy(), 1)
    assert np.array_equal(_u32(hd), up)
    assert up[1, 5] == SAT and up[1, 6] == SAT and up[1, 7] == PROMPT | SAT and up[1, 9] == PROMPT | 2 and up[0, 5] == 4 and up[2, V - 1] == 2
    ops.sample_history_count_ragged(hd, pd, -1)
    down = host(up.copy(), -1)
    assert np.array_equal(_u32(hd), down)
    assert down[1, 9] == PROMPT and down[1, 6] == SAT - 3 and down[0, 5] == 3      # bit 31 kept; no inverse at the ceiling
    ops.sample_history_count_ragged(hd, pd, -1)                    # to the floor
    assert np.array_equal(_u32(hd), host(down.copy(), -1))
    assert _u32(hd)[2, V - 1] == 0 and _u32(hd)[1, 9] == PROMPT
    before = _u32(hd).copy()
    ops.sample_history_count_ragged(hd, pd[:0], 1)                 # n = 0: nothing happens
    assert np.array_equal(_u32(hd), before)
    for bad in (0, 2, -2):
        with pytest.raises(ValueError, match="delta"):
            ops.sample_history_count_ragged(hd, pd, bad)
    assert np.array_equal(_u32(hd), before)


# ---- 3. the engine ------------------------------------------------------------------------------------------------------------------------
ENGINE_REQUESTS = {
    "neutral": [dict(temperature=0.8, seed=5), dict(temperature=0.9, top_k=12, top_p=0.9, min_p=0.02, seed=6), dict(temperature=1.1, seed=7)],
    "penalised": [dict(temperature=0.8, seed=7, repetition_penalty=1.8, presence_penalty=1.5, frequency_penalty=0.7, logit_bias={3: float("-inf"), 11: 1.5}),
                  dict(temperature=0.0, presence_penalty=2.0, repetition_penalty=1.4),
                  dict(temperature=0.9, top_k=12, seed=8, frequency_penalty=0.9)],
    "mixed": [dict(temperature=0.8, seed=5), dict(temperature=0.8, seed=7, repetition_penalty=1.8, presence_penalty=1.5, logit_bias={3: float("-inf")}),
              dict(temperature=0.0)],
}
EB = 3                                                            # the engine's batch


@pytest.fixture(scope="module")
def model(dev):
    from test_gpu_decode_batch import _model
    return _model(dev, "llama", 2, 8)


@pytest.fixture(scope="module")
def engines(dev, model):
    """(single-sequence reference, batched engine) per captured, built once."""
    from mobilequant_amd.decode import DecodeEngine
    from mobilequant_amd.decode_batch import BatchDecodeEngine
    made = {}

    def get(captured):
        if captured not in made:
            pair = (DecodeEngine(model, cache_len=CL), BatchDecodeEngine(model, EB, cache_len=CL))
            if captured:
                pair[0].capture(), pair[1].capture()
            made[captured] = pair
        return made[captured]
    return get


def _prompts(V, n):
    g = torch.Generator().manual_seed(12)
    base = torch.randint(0, V, (9,), generator=g).tolist()
    return [((base[i:] + base[:i]) * 4)[:ln] for i, ln in enumerate([19, 1, 30][:n])]      # they repeat themselves: prompt lookup finds something


def _sp(name, n):
    from mobilequant_amd import SamplingParams
    return [SamplingParams(**kw) for kw in ENGINE_REQUESTS[name][:n]]


@pytest.mark.parametrize("captured", [False, True], ids=["direct", "graph"])
def test_engine_rows_are_the_single_engines_rows(dev, engines, captured):
    """sample_rows behind step_tokens and step_sample_tokens: each slot's rows are DecodeEngine.step_sample_tokens for that sequence
    alone; slots not named do not move; a foreign step takes the rows away."""
    ref, eng = engines(captured)
    V = eng.shape.vocab
    prompts = _prompts(V, 3)
    g = torch.Generator().manual_seed(3)
    for name in ("penalised", "mixed"):
        sps = _sp(name, 3)
        for b in range(EB):
            eng.release(b)
        eng.start(1)
        eng.step([0, prompts[1][0], 0])                            # the one-token prompt, alone
        for b in (0, 2):
            eng.prefill(b, prompts[b])
        stepped = [[], [], []]                                     # per slot: the tokens stepped behind its prompt
        eng.set_sampling(sps, STREAMS[:3])
        for plan, fused in (({0: 3, 2: 4}, False), ({1: 5, 2: 1}, True), ({0: 8}, True), ({0: 1, 1: 1, 2: 1}, False)):
            for b in range(EB):
                eng.observe_history(b, prompts[b] + stepped[b])
            toks = {b: torch.randint(0, V, (n,), generator=g).tolist() for b, n in plan.items()}
            if 2 in toks:
                toks[2][1:] = [toks[2][0]] * (len(toks[2]) - 1)     # slot 2 proposes one token again and again
            still = [b for b in range(EB) if b not in plan]
            snap = [(eng.logits[b].clone(), eng.position(b), _u32(eng._sampler.history[b]).copy()) for b in still]
            if fused:
                got = eng.step_sample_tokens(toks).tolist()
            else:
                eng.step_tokens(toks)
                got = eng.sample_rows(sum(plan.values())).tolist()
            for (lg, p, h), b in zip(snap, still):
                assert torch.equal(eng.logits[b], lg) and eng.position(b) == p and int(eng.pos[b]) == p, (name, plan, b)
                assert np.array_equal(_u32(eng._sampler.history[b]), h), (name, plan, b)
            r0 = 0
            for b in sorted(plan):                                 # the sequence alone, along the same path: prefill (or a step), then steps
                ref.set_sampling(sps[b], STREAMS[b])
                ref._start_sequence(prompts[b], True)
                ref.extend(stepped[b])
                ref.observe_history(prompts[b] + stepped[b])
                want = ref.step_sample_tokens(toks[b]).tolist()
                assert got[r0:r0 + plan[b]] == want, (name, plan, b, got, want)
                assert torch.equal(eng.logits[b], ref.logits.view(-1)), (name, plan, b)
                r0 += plan[b]
                stepped[b] = stepped[b] + toks[b]                  # (every row's token stays in the cache)
        with pytest.raises(RuntimeError, match="row count"):
            eng.sample_rows(2)                                     # not the last call's rows
        eng.step([1, 2, 3])
        with pytest.raises(RuntimeError, match="row count"):
            eng.sample_rows(3)                                     # a foreign step stands between
    if captured:
        assert set(eng._row_sample_graphs) == {(6, True), (8, True)}      # one graph per (total rows, penalised), whatever the plan
    else:
        assert eng._row_sample_graphs == {}


def _truth(V, ctx, out):
    h = PR.prompt_history(V, ctx)
    for t in out[len(ctx):]:
        PR.observe(h, t)
    return h


@pytest.mark.parametrize("request_name", list(ENGINE_REQUESTS))
@pytest.mark.parametrize("captured", [False, True], ids=["direct", "graph"])
def test_batch_speculative_sampling_returns_plain_samplings_ids(dev, engines, captured, request_name):
    from mobilequant_amd.decode import prompt_lookup_draft
    ref, eng = engines(captured)
    V, NEW = eng.shape.vocab, 24
    for n in (1, 3, 2):
        prompts, sps, streams = _prompts(V, n), _sp(request_name, n), STREAMS[:n]
        alone = [ref.generate(p, NEW, sampling=sp, stream=st) for p, sp, st in zip(prompts, sps, streams)]
        plain = eng.generate(prompts, NEW, sampling=sps, streams=streams)
        assert plain == alone and all(len(o) == len(p) + NEW for o, p in zip(plain, prompts))
        oracle = [(lambda ids, k, t=t: t[len(ids):len(ids) + k]) for t in plain]
        wrong = [(lambda ids, k, t=t: [(v + 1) % V for v in t[len(ids):len(ids) + k]]) for t in plain]
        # every release is preceded by the slot's history as the loop left it
        seen, release = {}, eng.release

        def spy(slot):
            if eng.active(slot) and eng._sampler is not None and eng._sampler.pargs is not None:
                seen[slot] = _u32(eng._sampler.history[slot]).copy()
            release(slot)
        eng.release = spy
        try:
            for name, drafts, nd in (("oracle", oracle, 4), ("wrong", wrong, 4), ("lookup", prompt_lookup_draft(2), 3), ("oracle7", oracle, 7)):
                seen.clear()
                got = eng.generate_speculative(prompts, NEW, drafts, sampling=sps, streams=streams, num_draft=nd)
                assert got == plain, (n, name, got, plain)
                st = eng.spec_stats
                assert st["target_steps"] == st["rounds"] >= 1 and st["accepted"] <= st["proposed"]
                if name.startswith("oracle"):
                    assert st["accepted"] == st["proposed"] > 0, st
                    k = min(nd, eng.max_rows // n - 1)
                    assert st["rounds"] == math.ceil((NEW - 1) / (k + 1)), st
                if name == "wrong":
                    assert st["accepted"] == 0 and st["rounds"] == NEW - 1, st
                assert all(not eng.active(b) for b in range(EB))
                for i, sp in enumerate(sps):
                    if sp.penalized:                               # the history rebuilt from the output: the prompt marked, every new token counted
                        assert np.array_equal(seen[i], _truth(V, prompts[i], plain[i])), (n, name, i)
            # an EOS that cuts a round in the middle
            new = plain[0][len(prompts[0]):]
            cut = next(i for i in (8, 7, 9, 13, 12, 14, 18) if new[i] not in new[:i])
            plain_eos = eng.generate(prompts, NEW, sampling=sps, streams=streams, eos_token_id=new[cut])
            assert plain_eos[0] == plain[0][:len(prompts[0]) + cut + 1]
            for drafts in (oracle, prompt_lookup_draft(2)):
                assert eng.generate_speculative(prompts, NEW, drafts, sampling=sps, streams=streams, eos_token_id=new[cut]) == plain_eos, n
        finally:
            del eng.release
    # a sequence's ids do not depend on its slot or on its neighbours
    prompts, sps = _prompts(V, 3), _sp(request_name, 3)
    got = eng.generate_speculative(prompts[::-1], 12, prompt_lookup_draft(2), sampling=sps[::-1], streams=STREAMS[:3][::-1])
    assert got == [ref.generate(p, 12, sampling=sp, stream=st) for p, sp, st in zip(prompts, sps, STREAMS[:3])][::-1]
