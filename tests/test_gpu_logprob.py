"""GPU: per-token log-probabilities and top-n alternatives (csrc/mq_logprob.hip).

Kernel level: ids and ranks exactly, log-probabilities within the kernel header's bound (tests/logprob_ref.py evaluates it per entry;
nothing is left out of the comparison but -inf entries, which must match exactly), on Gaussian rows and on rows built to break ties,
at every size where the launches take another path (one slice, a tail slice, more than 64 slices, the 2^20 limit).  The bit contract:
a row's four outputs do not depend on the row count, its index, its neighbours, the stride, the index form or eager / replayed.
Engine level: generate(logprobs=...) leaves the ids alone and its records are ops.logprob_top of the raw logits, eager and captured,
single and batched, plain and speculative."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import logprob_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

INF = float("inf")
SL = R.SLICE


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _run(dev, rows, toks, n_top, stride=None):
    """ops.logprob_top on host rows [R, V]: the four outputs as numpy arrays."""
    from mobilequant_amd import ops
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    n, V = rows.shape
    buf = torch.full((n, stride or V), 7.5, dtype=torch.float32, device=dev)
    buf[:, :V] = torch.from_numpy(rows).to(dev)
    out = ops.logprob_top(buf[:, :V], torch.tensor([int(t) for t in toks], dtype=torch.int64, device=dev), n_top)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def _check_row(l, t, n_top, lp, rank, ids, tl, tag):
    """One row of outputs against the reference: ids and rank exactly, every log-probability within the header's bound."""
    V = l.size
    w_lp, w_rank, w_ids, w_tl = R.logprob_ref(l, t, n_top)
    assert rank == w_rank, (tag, rank, w_rank)
    assert ids.tolist() == w_ids.tolist(), (tag, ids.tolist(), w_ids.tolist())
    got = np.concatenate([[lp], tl]).astype(np.float64)
    want = np.concatenate([[w_lp], w_tl])
    worst = 0.0
    for g, w in zip(got, want):
        if np.isnan(w) or np.isinf(w):
            assert (np.isnan(g) and np.isnan(w)) or g == w, (tag, g, w)
        else:
            err, cap = abs(g - w), float(R.bound(V, w))
            assert cap <= 1e-5 and err <= cap, (tag, g, w, err, cap)
            worst = max(worst, err)
    return worst


def _check(dev, rows, toks, n_top, tag, stride=None):
    lp, rank, ids, tl = _run(dev, rows, toks, n_top, stride)
    worst = max(_check_row(np.asarray(rows[r], dtype=np.float32), toks[r], n_top, lp[r], rank[r], ids[r], tl[r], (tag, r)) for r in range(len(toks)))
    print(f"{tag}: max |logprob - float64 reference| = {worst:.3e}")
    return lp, rank, ids, tl


def _gauss(V, n, seed):
    return (np.random.default_rng(seed).standard_normal((n, V)) * 3).astype(np.float32)


# ---- the rule, at every size where the launches take another path ------------------------------------------------------------------
@pytest.mark.parametrize("n_top", [0, 1, 5, 20])
@pytest.mark.parametrize("V", [4, SL, SL + 4, 3 * SL + 8, 64 * SL + 4])
def test_gaussian_rows_match_the_reference(dev, V, n_top):
    rows = _gauss(V, 3, 100 + V % 97)
    toks = [int(rows[0].argmax()), int(rows[1].argmin()), V - 1]
    _check(dev, rows, toks, n_top, f"gauss V={V} n_top={n_top}", stride=V + 8)


def test_the_vocabulary_limit(dev):
    V = 1 << 20
    rows = _gauss(V, 2, 5)
    _check(dev, rows, [int(rows[0].argmin()), 777777], 20, "gauss V=2^20")


@pytest.mark.parametrize("n", [1, 3, 8])
def test_row_counts(dev, n):
    V = 2 * SL + 4
    rows = _gauss(V, n, 40 + n)
    _check(dev, rows, [(1237 * r) % V for r in range(n)], 5, f"rows={n}")


def _edge(V):
    """A slice boundary inside the row (rows of one slice: any index that leaves room behind it)."""
    return SL if V > 2 * SL else V // 4


def _tie_rows(V):
    """Rows built to break ties and corner the selection; (row, token, what)."""
    rng = np.random.default_rng(9)
    out = []
    B = _edge(V)
    half = np.round(rng.standard_normal(V) * 3 * 2) / 2               # multiples of 0.5: hundreds tie
    top = np.flatnonzero(half == half.max())
    mid = np.flatnonzero(half == 0.0)
    out += [(half, int(top[-1]), "halves, t the last of the maximal tie"), (half, int(mid[len(mid) // 2]), "halves, t inside a tie"),
            (half, int(half.argmin()), "halves, t the minimum"), (half, V - 1, "halves, t = V - 1")]
    base = rng.standard_normal(V) * 3 - 20
    cut = base.copy()
    cut[[5, 900, B - 1, B, B + 1, V - 1, 17]] = 4.0                   # 7 tie for the top: the n_top = 5 cut falls inside the tie
    out.append((cut, B + 1, "a tie across the n_top cut"))
    edge = base.copy()
    edge[B - 2:B + 2] = 6.0                                           # a tie across a slice boundary
    edge[2 * B - 1:2 * B + 1] = 5.5
    out.append((edge, 2 * B, "a tie across a slice boundary"))
    one = base.copy()
    one[B + 40:B + 60] = 3.0 + np.arange(20)[::-1] * 0.25            # the 20 largest inside one slice, 16 of them one thread's neighbours
    out.append((one, B + 59, "the 20 largest in one slice"))
    last = base.copy()
    last[V - 4:] = [9.0, 9.5, 9.0, 9.5]                                 # the largest on the last 4-entry block (the tail slice when V % SLICE == 4)
    last[100:116] = 8.0
    out.append((last, V - 2, "the largest on the last block"))
    zero = -np.abs(base) - 1
    zero[10], zero[3] = -0.0, 0.0                                       # +0 / -0: equal, the lower index first
    zero[B + 7] = -0.0
    out.append((zero, 10, "+0 / -0"))
    odd = base.copy()
    odd[[0, 77, B, V - 3]] = np.nan
    odd[[1, 78, B + 1, V - 2]] = -INF
    out += [(odd, 77, "NaN and -inf entries, t a NaN"), (odd, V - 2, "NaN and -inf entries, t a -inf")]
    dead = np.full(V, -INF)
    dead[50] = np.nan
    out += [(dead, 0, "all -inf, t = 0"), (dead, V - 1, "all -inf, t = V - 1")]
    one_inf = base.copy()
    one_inf[B + 3] = INF
    two_inf = one_inf.copy()
    two_inf[9] = INF
    out += [(one_inf, B + 3, "one +inf, t on it"), (one_inf, 4, "one +inf, t elsewhere"), (two_inf, B + 3, "two +inf, t the second"),
            (two_inf, 4, "two +inf, t elsewhere")]
    g = _gauss(V, 1, 77)[0]
    out += [(g, -1, "t = -1"), (g, V, "t = V"), (g, 1 << 40, "t = 2^40"), (g, -(1 << 40), "t = -2^40")]
    return out


@pytest.mark.parametrize("n_top", [5, 20])
@pytest.mark.parametrize("V", [SL, 2 * SL + 4])
def test_rows_built_to_break_ties(dev, V, n_top):
    cases, B = _tie_rows(V), _edge(V)
    for i in range(0, len(cases), 8):
        chunk = cases[i:i + 8]
        rows = np.stack([c[0] for c in chunk]).astype(np.float32)
        lp, rank, ids, tl = _check(dev, rows, [c[1] for c in chunk], n_top, f"ties V={V} n_top={n_top} [{i}:{i + 8}]")
        for r, (_, t, what) in enumerate(chunk):
            # the stated values of the special rows, apart from the reference
            if what.startswith("all -inf"):
                assert lp[r] == -INF and rank[r] == t + 1 and ids[r].tolist() == list(range(n_top)) and np.all(tl[r] == -INF), what
            if what == "one +inf, t on it":
                assert lp[r] == 0.0 and rank[r] == 1 and tl[r][0] == 0.0 and np.all(tl[r][1:] == -INF), what
            if what == "two +inf, t the second":
                assert rank[r] == 2 and ids[r][:2].tolist() == [9, B + 3] and lp[r] == tl[r][0] == tl[r][1] and np.all(tl[r][2:] == -INF), what
                assert abs(float(lp[r]) + np.log(2)) < 1e-6
            if what.endswith("t elsewhere"):
                assert lp[r] == -INF, what
            if what.startswith("t = "):
                assert np.isnan(lp[r]) and rank[r] == 0, what
            if what == "+0 / -0":
                assert ids[r][:3].tolist() == [3, 10, B + 7] and rank[r] == 2 and tl[r][0] == tl[r][1] == tl[r][2] == lp[r], what


def test_alternatives_past_the_vocabulary_are_padded(dev):
    rows = np.array([[1.0, 2.0, 2.0, 1.0], [0.0, -INF, np.nan, 3.0]], dtype=np.float32)
    lp, rank, ids, tl = _check(dev, rows, [3, 1], 20, "V=4 n_top=20")
    assert ids[0].tolist() == [1, 2, 0, 3] + [-1] * 16 and np.all(tl[:, 4:] == -INF) and rank.tolist() == [4, 3]


# ---- the bit contract ------------------------------------------------------------------------------------------------------------------
def _same(a, b, tag=""):
    for x, y in zip(a, b):
        x, y = (np.asarray(x).view(np.int32) if np.asarray(x).dtype == np.float32 else np.asarray(x)), \
               (np.asarray(y).view(np.int32) if np.asarray(y).dtype == np.float32 else np.asarray(y))
        assert x.shape == y.shape and np.array_equal(x, y), tag


@pytest.mark.parametrize("V", [SL, 2 * SL + 4, 65 * SL])
def test_a_row_does_not_depend_on_its_neighbours_its_index_or_the_stride(dev, V):
    row, t = _gauss(V, 1, 3)[0], 1234 % V
    row[[7, V - 9]] = row.max()                                         # a tie for the top
    alone = _run(dev, row[None], [t], 20)
    among = _gauss(V, 8, 4)
    among[5] = row
    eight = _run(dev, among, [0, 1, 2, 3, 4, t, 6, 7], 20, stride=V + 260)
    _same([o[0] for o in alone], [o[5] for o in eight], "row 5 of 8")
    wide = _run(dev, row[None], [t], 20, stride=2 * V)
    _same(alone, wide, "another stride")


def test_top_logprob_carries_the_bits_of_logprob(dev):
    V = 2 * SL + 4
    row = np.round(_gauss(V, 1, 8)[0] * 2) / 2
    lp, rank, ids, tl = _run(dev, row[None], [0], 20)
    again = []
    for i in range(0, 20, 8):
        k = ids[0][i:i + 8]
        o = _run(dev, np.repeat(row[None], len(k), 0), k.tolist(), 0)
        again += list(zip(o[0], o[1]))
    assert [int(np.float32(a).view(np.int32)) for a, _ in again] == tl[0].view(np.int32).tolist()
    assert [int(r) for _, r in again] == list(range(1, 21))


PAT_F, PAT_I = -123.25, 0x5A5A5A5A


def _form(dev, lg, tok, n_top, batch, record_len, cache_len=64, **index):
    """mq_logprob_top through the C ABI into pattern-filled record arrays [batch, record_len]; index: device tensors / n_offset."""
    from mobilequant_amd import _lib
    from mobilequant_amd._lib import MQ_LOGPROB_SCRATCH_BYTES, MqLogprobTopArgs
    rec = [torch.full((batch, record_len), PAT_F, dtype=torch.float32, device=dev), torch.full((batch, record_len), PAT_I, dtype=torch.int32, device=dev),
           torch.full((batch, record_len, n_top), PAT_I, dtype=torch.int32, device=dev), torch.full((batch, record_len, n_top), PAT_F, dtype=torch.float32, device=dev)]
    scratch = torch.empty(MQ_LOGPROB_SCRATCH_BYTES, dtype=torch.uint8, device=dev)
    a = MqLogprobTopArgs()
    a.logits, a.logits_stride, a.V, a.rows, a.n_top, a.tok = lg.data_ptr(), lg.stride(0), lg.shape[1], lg.shape[0], n_top, tok.data_ptr()
    a.batch, a.cache_len, a.record_len = batch, cache_len, record_len
    a.logprob, a.rank, a.top_id, a.top_logprob = (r.data_ptr() for r in rec)
    a.scratch, a.scratch_bytes = scratch.data_ptr(), MQ_LOGPROB_SCRATCH_BYTES
    for k, v in index.items():
        setattr(a, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    _lib.call("mq_logprob_top", ctypes.byref(a), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return a, rec, scratch


def _records_are(rec, want, where, tag):
    """rec holds row r of `want` at where[r] = (sequence, n) (None: the row wrote nothing) and the pattern everywhere else."""
    exp = [np.full(tuple(r.shape), PAT_F if r.dtype == torch.float32 else PAT_I, dtype=np.float32 if r.dtype == torch.float32 else np.int32) for r in rec]
    for r, at in enumerate(where):
        if at is not None:
            for e, w in zip(exp, want):
                e[at] = w[r]
    _same([r.cpu().numpy() for r in rec], exp, tag)


@pytest.mark.parametrize("V", [160, 2 * SL + 4])
def test_the_three_index_forms_write_the_same_bits_and_idle_rows_write_nothing(dev, V):
    n_top, L = 5, 64
    rows = _gauss(V, 6, 21)
    toks = [3, V - 1, 17, 0, V, 5]
    want = _run(dev, rows, toks, n_top)
    lg = torch.from_numpy(rows).to(dev)
    tok = torch.tensor(toks, dtype=torch.int64, device=dev)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)      # noqa: E731
    # (a) row r is sequence r at pos[r]; outside [0, cache_len): idle
    pos = [5, 63, L, -1, 0, 64 + 7]
    _, rec, _ = _form(dev, lg, tok, n_top, 6, L, cache_len=L, pos=i32(pos))
    _records_are(rec, want, [(0, 5), (1, 63), None, None, (4, 0), None], "form a")
    # (a) with a record shorter than the cache: n outside [0, record_len) writes nothing
    _, rec, _ = _form(dev, lg, tok, n_top, 6, 8, cache_len=L, pos=i32([5, 63, 8, 7, 0, 9]))
    _records_are(rec, want, [(0, 5), None, None, (3, 7), (4, 0), None], "form a, short record")
    # (b) every row is sequence 0 at *n_base + n_offset + j
    _, rec, _ = _form(dev, lg, tok, n_top, 1, L, n_base=i32([40]), n_offset=-5)
    _records_are(rec, want, [(0, 35 + j) for j in range(6)], "form b")
    _, rec, _ = _form(dev, lg, tok, n_top, 1, L, n_base=i32([62]), n_offset=-1)      # rows 3.. fall off the record's end
    _records_are(rec, want, [(0, 61), (0, 62), (0, 63), None, None, None], "form b, the record's end")
    _, rec, _ = _form(dev, lg, tok, n_top, 1, L, n_base=i32([1]), n_offset=-3)       # rows 0, 1 in front of its start
    _records_are(rec, want, [None, None, (0, 0), (0, 1), (0, 2), (0, 3)], "form b, the record's start")
    # (c) a permuted, partly idle table; entries out of range in both columns
    seq = [2, 0, 9, 1, -1, 2]
    rp = [10, 62, 3, L, 4, 63]
    _, rec, _ = _form(dev, lg, tok, n_top, 3, L, cache_len=L, row_seq=i32(seq), row_pos=i32(rp), n_offset=1)
    _records_are(rec, want, [(2, 11), (0, 63), None, None, None, None], "form c")        # (row 5: position 63 + 1 is past the record)
    _, rec, _ = _form(dev, lg, tok, n_top, 3, L, cache_len=L, row_seq=i32([1, 1, 1, 0, 2, 2]), row_pos=i32([0, 1, 2, 7, -3, 1 << 30]), n_offset=0)
    _records_are(rec, want, [(1, 0), (1, 1), (1, 2), (0, 7), None, None], "form c, a run")
    # no form: row r at [r][0]
    _, rec, _ = _form(dev, lg, tok, n_top, 6, 1)
    _records_are(rec, want, [(r, 0) for r in range(6)], "no form")


@pytest.mark.parametrize("V", [160, 2 * SL + 4])
def test_a_captured_launch_follows_the_position_and_equals_the_eager_one(dev, V):
    from mobilequant_amd import _lib
    n_top, L = 5, 16
    rows = _gauss(V, 4, 31)
    lg = torch.from_numpy(rows[:2]).to(dev)
    tok = torch.tensor([1, 2], dtype=torch.int64, device=dev)
    pos = torch.tensor([3, L], dtype=torch.int32, device=dev)
    a, rec, keep = _form(dev, lg, tok, n_top, 2, L, cache_len=L, pos=pos)           # eager, and the kernels are loaded
    first = _run(dev, rows[:2], [1, 2], n_top)
    _records_are(rec, first, [(0, 3), None], "eager")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _lib.call("mq_logprob_top", ctypes.byref(a), torch.cuda.current_stream().cuda_stream)
    for r in rec:
        r.fill_(PAT_F if r.dtype == torch.float32 else PAT_I)
    g.replay()
    torch.cuda.synchronize()
    _records_are(rec, first, [(0, 3), None], "replay 1")
    lg.copy_(torch.from_numpy(rows[2:]))                                # the next step: new logits, new tokens, positions moved on the device
    tok.copy_(torch.tensor([V - 1, 0]))
    pos.copy_(torch.tensor([4, 9], dtype=torch.int32))
    g.replay()
    torch.cuda.synchronize()
    second = _run(dev, rows[2:], [V - 1, 0], n_top)
    exp = [np.full(tuple(r.shape), PAT_F if r.dtype == torch.float32 else PAT_I, dtype=np.float32 if r.dtype == torch.float32 else np.int32) for r in rec]
    for e, w1, w2 in zip(exp, first, second):
        e[0, 3], e[0, 4], e[1, 9] = w1[0], w2[0], w2[1]
    _same([r.cpu().numpy() for r in rec], exp, "replay 2")


# ---- the engines -----------------------------------------------------------------------------------------------------------------------
CL, NEW, STREAM = 64, 12, 5
REQUESTS = {
    "neutral": dict(temperature=0.9, seed=11),
    "filtered": dict(temperature=0.8, top_k=12, top_p=0.9, min_p=0.02, seed=12),
    "penalised": dict(temperature=0.9, seed=13, repetition_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.25),
}


@pytest.fixture(scope="module")
def model(dev):
    from test_gpu_decode_batch import _model
    return _model(dev, "llama", 2, 8)


@pytest.fixture(scope="module")
def engines(dev, model):
    """captured -> (DecodeEngine, a second one as a self-draft, BatchDecodeEngine of 4 slots), built once."""
    from mobilequant_amd import BatchDecodeEngine, DecodeEngine
    made = {}

    def get(captured):
        if captured not in made:
            trio = [DecodeEngine(model, cache_len=CL), DecodeEngine(model, cache_len=CL), BatchDecodeEngine(model, batch=4, cache_len=CL)]
            if captured:
                for e in trio:
                    e.capture()
            made[captured] = trio
        return made[captured]
    return get


def _ctx(V, n=20, seed=12):
    from test_gpu_decode_batch import _prompts
    base = _prompts(V, [n // 2], seed)[0]
    return (base + base)[:n]                                            # repeats itself: prompt lookup finds something


def _same_records(a, b, tag=""):
    _same([t.numpy() for t in a], [t.numpy() for t in b], tag)


@pytest.mark.parametrize("captured", [False, True], ids=["direct", "graph"])
def test_logprobs_leave_the_ids_alone_and_eager_equals_captured(dev, engines, captured):
    from mobilequant_amd import SamplingParams, TokenLogprobs
    eng = engines(captured)[0]
    ctx = _ctx(eng.shape.vocab)
    for name, req in REQUESTS.items():
        sp = SamplingParams(**req)
        plain = eng.generate(ctx, NEW, sampling=sp, stream=STREAM)
        ids, rec = eng.generate(ctx, NEW, sampling=sp, stream=STREAM, logprobs=5)
        assert ids == plain and isinstance(rec, TokenLogprobs), name
        assert rec.logprob.shape == (NEW,) and rec.rank.shape == (NEW,) and rec.top_id.shape == (NEW, 5) and rec.top_logprob.shape == (NEW, 5)
        assert bool(torch.all(rec.logprob <= 0)) and bool(torch.all(rec.rank >= 1)) and bool(torch.all(rec.top_logprob[:, :-1] >= rec.top_logprob[:, 1:]))
        other = engines(not captured)[0].generate(ctx, NEW, sampling=sp, stream=STREAM, logprobs=5)
        assert other[0] == ids, name
        _same_records(rec, other[1], name)
        ids0, rec0 = eng.generate(ctx, NEW, sampling=sp, stream=STREAM, logprobs=0)
        assert ids0 == plain and rec0.top_id.shape == (NEW, 0)
        _same([rec0.logprob.numpy(), rec0.rank.numpy()], [rec.logprob.numpy(), rec.rank.numpy()], name)


@pytest.mark.parametrize("captured", [False, True], ids=["direct", "graph"])
def test_records_are_the_op_on_the_raw_logits(dev, engines, captured):
    """A hand-driven loop: sample(), clone the logits, step().  Under a penalised and biased request the records are still those of the
    raw row: a banned token keeps its raw rank."""
    from mobilequant_amd import SamplingParams, ops
    eng = engines(captured)[0]
    V = eng.shape.vocab
    ctx = _ctx(V)
    eng._start_sequence(ctx, True)
    banned = int(torch.argmax(eng.logits))                              # the raw favourite behind the context
    requests = dict(REQUESTS, penalised=dict(REQUESTS["penalised"], logit_bias={banned: -INF, 7: 1.5}))
    for name, req in requests.items():
        sp = SamplingParams(**req)
        eng.set_sampling(sp, STREAM)
        eng.set_logprobs(5)
        eng._start_sequence(ctx, True)
        eng.observe_history(ctx)
        rows, toks = [], []
        for i in range(8):
            if i < 7:
                eng.sample()
                rows.append(eng.logits.clone())
                toks.append(eng.tok.clone())
                eng.step()
            else:
                rows.append(eng.logits.clone())
                eng.sample_step()                                       # one graph after capture(): the record is written before the step
                toks.append(eng.tok.clone())
        rec = eng.logprob_records(len(ctx), len(ctx) + 8)
        want = ops.logprob_top(torch.stack(rows), torch.cat(toks), 5)
        _same([t.numpy() for t in rec], [w.cpu().numpy() for w in want], name)
        if name == "penalised":
            assert int(toks[0]) != banned and int(rec.top_id[0, 0]) == banned and int(rec.rank[0]) > 1
    eng.set_logprobs(None)
    with pytest.raises(RuntimeError, match="set_logprobs"):
        eng.logprob_records(0, 1)


@pytest.mark.parametrize("captured", [False, True], ids=["direct", "graph"])
def test_a_slot_of_the_batched_engine_equals_the_sequence_alone(dev, engines, captured):
    from mobilequant_amd import SamplingParams
    eng, _, be = engines(captured)
    V = eng.shape.vocab
    prompts = [_ctx(V, 20, 1), _ctx(V, 7, 2), _ctx(V, 33, 3)]
    sps = [SamplingParams(**REQUESTS[k]) for k in ("neutral", "filtered", "penalised")]
    alone = [eng.generate(p, NEW, sampling=s, stream=10 + i, logprobs=5) for i, (p, s) in enumerate(zip(prompts, sps))]
    for perm in ([0, 1, 2], [2, 0, 1], [1, 2, 0]):                      # every prompt in every slot; the slots are released and used again
        outs, recs = be.generate([prompts[i] for i in perm], NEW, sampling=[sps[i] for i in perm], streams=[10 + i for i in perm], logprobs=5)
        for slot, i in enumerate(perm):
            assert outs[slot] == alone[i][0], (perm, slot)
            _same_records(recs[slot], alone[i][1], (perm, slot))
    plain = be.generate(prompts, NEW, sampling=sps, streams=[10, 11, 12])
    assert plain == [a[0] for a in alone]


@pytest.mark.parametrize("captured", [False, True], ids=["direct", "graph"])
def test_speculative_generation_returns_plain_generations_records(dev, engines, captured):
    from mobilequant_amd import SamplingParams
    from mobilequant_amd.decode import prompt_lookup_draft
    eng, self_draft, be = engines(captured)
    V = eng.shape.vocab
    for name in ("neutral", "penalised"):
        sp = SamplingParams(**REQUESTS[name])
        for ctx, new, what in ((_ctx(V), NEW, "max_new_tokens"), (_ctx(V, CL - 8), 8, "the cache end")):
            ids, rec = eng.generate(ctx, new, sampling=sp, stream=STREAM, logprobs=5)
            wrong = lambda p, k: [(ids[len(p) + i] + 1) % V if len(p) + i < len(ids) else 0 for i in range(k)]      # noqa: E731
            for dname, draft in (("self", self_draft), ("wrong", wrong), ("lookup", prompt_lookup_draft(3))):
                got, grec = eng.generate_speculative(ctx, new, draft, sampling=sp, stream=STREAM, logprobs=5)
                assert got == ids, (name, what, dname)
                _same_records(grec, rec, (name, what, dname))
                st = eng.spec_stats
                if dname == "self":
                    assert st["accepted"] == st["proposed"] > 0, st
                    assert self_draft._lp is None                       # a draft engine computes no log-probabilities
                if dname == "wrong":
                    assert st["accepted"] == 0 and st["proposed"] > 0, st       # every record behind row 0 was written once and overwritten
            outs, recs = be.generate_speculative([ctx, ctx[:9]], new, [wrong, prompt_lookup_draft(3)], sampling=sp, streams=[STREAM, STREAM + 1], logprobs=5)
            assert outs[0] == ids, (name, what)
            _same_records(recs[0], rec, (name, what, "batch"))
            one = eng.generate(ctx[:9], new, sampling=sp, stream=STREAM + 1, logprobs=5)
            assert outs[1] == one[0]
            _same_records(recs[1], one[1], (name, what, "batch slot 1"))
        # a stop by EOS in the middle of a round
        ctx = _ctx(V)
        ids, _ = eng.generate(ctx, NEW, sampling=sp, stream=STREAM, logprobs=5)
        new_ids = ids[len(ctx):]
        cut = next(i for i in (5, 4, 6, 7, 3) if new_ids[i] not in new_ids[:i])
        want = eng.generate(ctx, NEW, sampling=sp, stream=STREAM, logprobs=5, eos_token_id=new_ids[cut])
        assert want[0] == ids[:len(ctx) + cut + 1] and want[1].logprob.shape == (cut + 1,)
        for draft in (self_draft, prompt_lookup_draft(3)):
            got = eng.generate_speculative(ctx, NEW, draft, sampling=sp, stream=STREAM, logprobs=5, eos_token_id=new_ids[cut])
            assert got[0] == want[0]
            _same_records(got[1], want[1], (name, "eos"))
        outs, recs = be.generate_speculative([ctx], NEW, prompt_lookup_draft(3), sampling=sp, streams=[STREAM], logprobs=5, eos_token_id=new_ids[cut])
        assert outs[0] == want[0]
        _same_records(recs[0], want[1], (name, "eos, batch"))


@pytest.mark.parametrize("captured", [False, True], ids=["direct", "graph"])
def test_records_follow_the_row_buffers_of_a_fresh_lowering(dev, model, captured):
    """refresh_grids() lowers the row chain again: new row logits, token and table buffers, a new selection launch.  The logprob
    launch kept for this n_top must follow them (its row blocks belong to the selection launch they were made for)."""
    from mobilequant_amd import BatchDecodeEngine, DecodeEngine, SamplingParams
    from mobilequant_amd.decode import prompt_lookup_draft
    sp = SamplingParams(**REQUESTS["filtered"])
    eng, be = DecodeEngine(model, cache_len=CL), BatchDecodeEngine(model, batch=2, cache_len=CL)
    if captured:
        eng.capture(), be.capture()
    ctx = _ctx(eng.shape.vocab)
    wrong = lambda p, k: [1] * k      # noqa: E731
    for e, run in ((eng, lambda d: eng.generate_speculative(ctx, NEW, d, sampling=sp, stream=STREAM, num_draft=3, logprobs=5)),
                   (be, lambda d: tuple(x[0] for x in be.generate_speculative([ctx], NEW, d, sampling=sp, streams=[STREAM], num_draft=3, logprobs=5)))):
        want = eng.generate(ctx, NEW, sampling=sp, stream=STREAM, logprobs=5)
        first = run(wrong)
        old = (e.rlogits, e.rsel, e._row_sel, e._lp_launches[5])
        e.refresh_grids()
        old[0].fill_(3.0e38), old[1].fill_(-7)                          # the old row buffers, kept alive here: a launch still bound to them reads this
        for draft in (wrong, prompt_lookup_draft(3)):
            again = run(draft)
            assert again[0] == first[0] == want[0]
            _same_records(again[1], want[1], (type(e).__name__, "after refresh_grids"))
            _same_records(first[1], want[1], (type(e).__name__, "before refresh_grids"))
        assert e._row_sel is not old[2] and e.rlogits is not old[0] and e._lp_launches[5] is old[3]
        held = [sel for sel, _ in old[3]._row_args.values()]
        assert held and all(sel is e._row_sel for sel in held)          # every cached block was made again for the new selection launch
        assert all(l.scratch is old[3].scratch for l in e.set_logprobs(2)._lp_launches.values())      # one scratch for every n_top
        e.set_logprobs(None)


def test_generate_leaves_a_switch_set_by_hand_as_it_found_it(dev, engines):
    from mobilequant_amd import SamplingParams
    eng, _, be = engines(False)
    sp = SamplingParams(**REQUESTS["neutral"])
    ctx = _ctx(eng.shape.vocab)
    for e, plain, with_lp in ((eng, lambda: eng.generate(ctx, 4, sampling=sp), lambda: eng.generate(ctx, 4, sampling=sp, logprobs=5)),
                              (be, lambda: be.generate([ctx], 4, sampling=sp), lambda: be.generate([ctx], 4, sampling=sp, logprobs=5))):
        e.set_logprobs(None)
        with_lp()
        assert e._lp is None
        e.set_logprobs(3)
        mine = e._lp
        ids = plain()
        assert e._lp is mine and with_lp()[0] == ids and e._lp is mine
        e.set_logprobs(None)


def test_switching_off_replays_the_graphs_without_the_launch(dev, model):
    from mobilequant_amd import BatchDecodeEngine, DecodeEngine, SamplingParams
    sp = SamplingParams(**REQUESTS["neutral"])
    eng = DecodeEngine(model, cache_len=CL).capture()
    ctx = _ctx(eng.shape.vocab)
    plain = eng.generate(ctx, NEW, sampling=sp, stream=STREAM)
    wrong = lambda p, k: [0] * k      # noqa: E731
    spec = eng.generate_speculative(ctx, NEW, wrong, sampling=sp, stream=STREAM, num_draft=3)
    assert spec == plain
    keys, row_keys = dict(eng._sample_graphs), dict(eng._row_sample_graphs)
    assert keys and all(len(k) == 2 for k in keys) and row_keys and all(len(k) == 2 for k in row_keys)
    assert eng.generate(ctx, NEW, sampling=sp, stream=STREAM, logprobs=5)[0] == plain
    assert eng.generate_speculative(ctx, NEW, wrong, sampling=sp, stream=STREAM, num_draft=3, logprobs=5)[0] == plain
    on, row_on = set(eng._sample_graphs) - set(keys), set(eng._row_sample_graphs) - set(row_keys)
    assert on == {k + (5,) for k in keys} and row_on == {k + (5,) for k in row_keys}     # one more key component; the first graphs are kept
    assert eng.generate(ctx, NEW, sampling=sp, stream=STREAM) == plain and eng._lp is None
    assert eng.generate_speculative(ctx, NEW, wrong, sampling=sp, stream=STREAM, num_draft=3) == plain
    assert set(eng._sample_graphs) == set(keys) | on and all(eng._sample_graphs[k] is g for k, g in keys.items())      # nothing new was recorded:
    assert set(eng._row_sample_graphs) == set(row_keys) | row_on and all(eng._row_sample_graphs[k] is g for k, g in row_keys.items())      # the old graphs replayed
    be = BatchDecodeEngine(model, batch=2, cache_len=CL).capture()
    base = be.generate([ctx, ctx[:5]], NEW, sampling=sp)
    assert set(be._sample_graphs) == {False}
    assert be.generate([ctx, ctx[:5]], NEW, sampling=sp, logprobs=5)[0] == base
    assert set(be._sample_graphs) == {False, (False, 5)}
    first = be._sample_graphs[False]
    assert be.generate([ctx, ctx[:5]], NEW, sampling=sp) == base and be._lp is None
    assert set(be._sample_graphs) == {False, (False, 5)} and be._sample_graphs[False] is first
