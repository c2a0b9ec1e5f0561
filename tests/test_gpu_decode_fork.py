"""Forking cached sequences on the device: mq_decode_cache_fork against a torch restatement of its rule -- caches
filled with random bytes and compared WHOLE, so every untouched byte counts -- and BatchDecodeEngine.fork / generate(n=) /
generate_speculative(n=) against slots that encoded the same prompt themselves.  Every comparison is an equality of bytes, bits or ids.
The fork / step / append cases run the toy model of tests/test_gpu_prefill_append.py (head_dim 64).  Its vocabulary of 97 entries is no
multiple of 4, which every mq_sample launch requires, so the cases that draw tokens (generate(n=), generate_speculative(n=), the sampler
history) run the TinyLlama-geometry toy of tests/test_gpu_decode_batch.py (head_dim 64, vocabulary 160) that the other sampling tests use."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_gpu_prefill_append import CACHE_LEN, _ids, _model  # noqa: E402

pytestmark = pytest.mark.gpu

INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
POS = [0, 1, 15, 16, 63, 79, 80, 40]                               # cache_len 80: slot 6 is idle
POS_B = [40, 80, 79, 63, 16, 15, 1, 5]                             # the same tables with other slots live
IDENT = list(range(8))
TABLES = {
    "fan_out_1": [0, 1, 2, 4, 4, 5, 6, 7],
    "fan_out_7": [5, 5, 5, 5, 5, 5, 5, 5],
    "two_sources": [0, 0, 0, 3, 5, 5, 5, 5],                       # 0 -> 1, 2 and 5 -> 4, 6, 7
    "source_at_0": [0, 0, 2, 3, 4, 5, 6, 7],                       # POS[0] == 0: nothing to copy
    "idle_source": [6, 1, 2, 3, 4, 5, 6, 6],                       # POS[6] == cache_len
    "chain": [0, 2, 3, 3, 4, 5, 6, 7],                             # 1 -> 2 -> 3: slot 1 is a no-op, slot 2 takes slot 3
    "out_of_range": [-1, 8, INT_MIN, INT_MAX, 4, 4, 6, 7],         # only 5 <- 4 is live
    "identity": IDENT,
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _i32(v, dev):
    return torch.tensor(v, dtype=torch.int32).to(dev)


def _random_caches(n, B, H, L, D, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(-128, 128, (B, H, L, D), generator=g, dtype=torch.int8).to(dev) for _ in range(n)]


def _rule(caches, pos, parent, L):
    """The rule, restated with torch indexing on copies: slot d takes [0, pos[p]) of every head from p = parent[d] iff p is in range,
    p != d, parent[p] == p and 0 <= pos[p] < L.  Everything else keeps its bytes."""
    out = [c.clone() for c in caches]
    B = len(pos)
    for d in range(B):
        p = parent[d]
        if not 0 <= p < B or p == d or parent[p] != p or not 0 <= pos[p] < L:
            continue
        for o, c in zip(out, caches):
            o[d, :, :pos[p]] = c[p, :, :pos[p]]
    return out


def _run_and_compare(caches, pos, parent, L, dev, **kw):
    import mobilequant_amd as mq
    want = _rule(caches, pos, parent, L)
    dpos, dpar = _i32(pos, dev), _i32(parent, dev)
    mq.ops.decode_cache_fork(caches, dpos, dpar, **kw)
    torch.cuda.synchronize()
    assert dpos.tolist() == pos and dpar.tolist() == parent
    for i, (got, w) in enumerate(zip(caches, want)):
        assert torch.equal(got, w), (i, (got != w).nonzero()[:4].tolist())
    return want


# ---- the kernel ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [16, 64, 128, 256])
def test_kernel_copies_what_the_rule_says_and_nothing_else(dev, D):
    L = 80
    for name, parent in TABLES.items():
        for pos in (POS, POS_B):
            caches = _random_caches(3, 8, 2, L, D, dev, seed=D)
            before = [c.clone() for c in caches]
            want = _run_and_compare(caches, pos, parent, L, dev)
            changed = any(not torch.equal(w, b) for w, b in zip(want, before))
            if name == "identity" or (pos is POS and name in ("source_at_0", "idle_source")):
                assert not changed, name                           # these tables write nothing at all
            if name in ("fan_out_1", "fan_out_7", "two_sources", "chain", "out_of_range"):
                assert changed, name                               # (the reference itself moves bytes: the comparison is not vacuous)


def test_kernel_goes_round_its_chunk_loop(dev):
    """2 MiB per head: more chunks than one round of the grid covers.  The source stops one position short of the cache's end."""
    L = 8192
    caches = _random_caches(2, 2, 1, L, 256, dev, seed=5)
    want = _run_and_compare(caches, [L - 1, L], [0, 0], L, dev)
    assert torch.equal(want[0][1, :, :L - 1], want[0][0, :, :L - 1]) and not torch.equal(want[0][1, :, L - 1], want[0][0, :, L - 1])


def test_registered_operator_runs_the_same_launch(dev):
    import mobilequant_amd.torch_ops  # noqa: F401
    L = 80
    caches = _random_caches(3, 8, 2, L, 64, dev, seed=4)
    want = _rule(caches, POS_B, TABLES["two_sources"], L)
    assert torch.ops.mobilequant_amd.decode_cache_fork(caches, _i32(POS_B, dev), _i32(TABLES["two_sources"], dev)) is None
    torch.cuda.synchronize()
    assert all(torch.equal(c, w) for c, w in zip(caches, want))


def test_batch_one_has_no_destination(dev):
    caches = _random_caches(2, 1, 2, 32, 64, dev, seed=6)
    for parent in ([0], [-1], [1], [INT_MAX]):
        _run_and_compare(caches, [17], parent, 32, dev)


def test_one_captured_launch_serves_later_tables(dev):
    import mobilequant_amd as mq
    L = 80
    caches = _random_caches(3, 8, 2, L, 64, dev, seed=9)
    fill = [c.clone() for c in caches]
    table = mq.ops.decode_cache_table(caches)
    dpos, dpar = _i32(POS, dev), _i32(IDENT, dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                      # no warm-up launch in front: there is no launch attribute to set
        mq.ops.decode_cache_fork(caches, dpos, dpar, table=table)
    for pos, parent in ((POS, TABLES["fan_out_7"]), (POS_B, TABLES["two_sources"]), (POS, TABLES["out_of_range"])):
        eager = [c.clone() for c in fill]
        mq.ops.decode_cache_fork(eager, _i32(pos, dev), _i32(parent, dev))
        for c, f in zip(caches, fill):
            c.copy_(f)
        dpos.copy_(_i32(pos, dev))
        dpar.copy_(_i32(parent, dev))
        g.replay()
        torch.cuda.synchronize()
        want = _rule(fill, pos, parent, L)
        for got, e, w in zip(caches, eager, want):
            assert torch.equal(got, e) and torch.equal(got, w)


def test_op_refusals_on_device_tensors(dev):
    import mobilequant_amd as mq
    caches = _random_caches(2, 2, 1, 8, 16, dev)
    pos, par = _i32([3, 8], dev), _i32([0, 0], dev)
    for bad in (torch.zeros(2, dtype=torch.int32, device=dev), torch.zeros(3, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int64)):
        with pytest.raises(RuntimeError, match="table|no CPU path"):
            mq.ops.decode_cache_fork(caches, pos, par, table=bad)
    odd = torch.zeros(2 * 8 * 16 + 8, dtype=torch.int8, device=dev)[8:].view(2, 1, 8, 16)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        mq.ops.decode_cache_fork([odd], pos, par)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mq.ops.decode_cache_fork(caches, pos.cpu(), par)


# ---- the engine ------------------------------------------------------------------------------------------------------------------------
B = 4
_ENGINES, _MODELS = {}, {}


def _engines(dev, captured):
    """Two batched engines on the toy model, built once per `captured`; every slot released."""
    from mobilequant_amd.decode_batch import BatchDecodeEngine
    if captured not in _ENGINES:
        m = _model(dev, 64)
        made = (BatchDecodeEngine(m, B, cache_len=CACHE_LEN), BatchDecodeEngine(m, B, cache_len=CACHE_LEN))
        if captured:
            for e in made:
                e.capture()
        _ENGINES[captured] = made
    a, b = _ENGINES[captured]
    for e in (a, b):
        for s in range(B):
            e.release(s)
    return a, b


def _sampling_engines(dev, captured):
    """(single-sequence reference, batched engine) on a model whose vocabulary the samplers take, built once per `captured`."""
    from test_gpu_decode_batch import _model as _llama
    from mobilequant_amd.decode import DecodeEngine
    from mobilequant_amd.decode_batch import BatchDecodeEngine
    key = ("sampling", captured)
    if key not in _ENGINES:
        m = _MODELS.get("llama") or _MODELS.setdefault("llama", _llama(dev, "llama", 2, 8))
        made = (DecodeEngine(m, cache_len=CACHE_LEN), BatchDecodeEngine(m, B, cache_len=CACHE_LEN))
        if captured:
            for e in made:
                e.capture()
        _ENGINES[key] = made
    ref, eng = _ENGINES[key]
    for s in range(B):
        eng.release(s)
    return ref, eng


def _same_slots(a, b, slots):
    """Slots `slots` of the two engines hold the same sequence: position, logits row, caches below the position."""
    torch.cuda.synchronize()
    for s in slots:
        n = a.position(s)
        assert n == b.position(s) and a.active(s) and b.active(s) and a.pos[s].item() == b.pos[s].item() == n
        assert torch.equal(a.logits[s], b.logits[s]), s
        for li in range(len(a.k_cache)):
            assert torch.equal(a.cached_keys(s, li), b.cached_keys(s, li)) and torch.equal(a.cached_values(s, li), b.cached_values(s, li)), (s, li)


def _step_both(a, b, slots):
    """Several steps with different tokens per slot keep the two engines' logits and caches equal."""
    for toks in ([3, 4, 5, 6], [90, 0, 17, 17]):
        assert torch.equal(a.step(toks)[slots], b.step(toks)[slots])
    ragged = {s: [7 + s, 8, 9 + s][:1 + (i % 3)] for i, s in enumerate(slots)}
    ra, rb = a.step_tokens(ragged), b.step_tokens(ragged)
    for s in slots:
        assert torch.equal(ra[s], rb[s]), s
    assert torch.equal(a.step([1, 2, 3, 4])[slots], b.step([1, 2, 3, 4])[slots])
    _same_slots(a, b, slots)


CAPTURED = pytest.mark.parametrize("captured", [False, True], ids=["direct", "graph"])


@CAPTURED
def test_forked_slots_are_slots_that_prefilled_the_prompt_themselves(dev, captured):
    a, b = _engines(dev, captured)
    m = a.model
    p, q = _ids(m, 37, seed=11), _ids(m, 50, seed=12)
    a.prefill(0, p)
    a.prefill(2, q)
    for s in (0, 1, 3):
        b.prefill(s, p)
    b.prefill(2, q)
    a.tok[0], b.tok[0] = 9, 9
    for s in (1, 3):
        b.tok[s] = 9
    keep = [(a.k_cache[li][2].clone(), a.v_cache[li][2].clone()) for li in range(2)]
    row2, tok2 = a.logits[2].clone(), a.tok[2].item()
    src = [(a.k_cache[li][0].clone(), a.v_cache[li][0].clone()) for li in range(2)]
    a._rows_at = (1, list(a._host_pos))
    assert a.fork({0: [1, 3]}) is a
    torch.cuda.synchronize()
    assert a.fork_stats == {"sources": 1, "destinations": 2, "positions": 74, "bytes": 74 * 64 * 2 * 4}
    assert a._rows_at is None
    assert a.pos.tolist() == [37, 37, 50, 37] and [a.position(s) for s in range(B)] == [37, 37, 50, 37] and all(a.active(s) for s in range(B))
    assert a.tok.tolist() == [9, 9, tok2, 9] and a.tok.tolist() == b.tok.tolist()
    for li in range(2):                                            # the bystander and the source keep every byte
        assert torch.equal(a.k_cache[li][2], keep[li][0]) and torch.equal(a.v_cache[li][2], keep[li][1])
        assert torch.equal(a.k_cache[li][0], src[li][0]) and torch.equal(a.v_cache[li][0], src[li][1])
    assert torch.equal(a.logits[2], row2)
    _same_slots(a, b, [0, 1, 2, 3])
    _step_both(a, b, [0, 1, 2, 3])


@CAPTURED
def test_fork_behind_steps_and_over_a_longer_active_slot(dev, captured):
    a, b = _engines(dev, captured)
    m = a.model
    p, longer = _ids(m, 37, seed=11), _ids(m, 90, seed=13)
    a.prefill(0, p)
    a.prefill(1, longer)                                           # an active destination at a LONGER position
    a.prefill(3, longer[:20])
    for s in (0, 1, 2):
        b.prefill(s, p)
    b.prefill(3, longer[:20])
    a.release(1), a.release(3)                                     # the source steps alone: its position is no prefill boundary
    for t in (5, 6):
        a.step([t, 0, 0, 0])
    a.set_position(1, 90), a.set_position(3, 20)
    b.release(3)
    for t in (5, 6):
        b.step([t, t, t, 0])
    b.set_position(3, 20)
    tail = [(a.k_cache[li][1, :, 39:].clone(), a.v_cache[li][1, :, 39:].clone()) for li in range(2)]
    a.fork({0: (1, 2)})
    torch.cuda.synchronize()
    assert a.fork_stats == {"sources": 1, "destinations": 2, "positions": 78, "bytes": 78 * 64 * 2 * 4}
    assert a.pos.tolist() == [39, 39, 39, 20] and [a.position(s) for s in range(B)] == [39, 39, 39, 20]
    for li in range(2):                                            # nothing at or past the source's position is written
        assert torch.equal(a.k_cache[li][1, :, 39:], tail[li][0]) and torch.equal(a.v_cache[li][1, :, 39:], tail[li][1])
    _same_slots(a, b, [0, 1, 2, 3])
    _step_both(a, b, [0, 1, 2, 3])


@CAPTURED
def test_fork_then_append_is_the_append_of_a_slot_that_prefilled_the_prefix(dev, captured):
    """The shared-system-prompt recipe: fork, then prefill(slot, suffix, append=True) on a destination."""
    a, b = _engines(dev, captured)
    ids = _ids(a.model)
    a.prefill(0, ids[:70])
    b.prefill(0, ids[:70])
    b.prefill(1, ids[:70])
    a.fork({0: [1]})
    got = a.prefill(1, ids[70:200], append=True).clone()
    want = b.prefill(1, ids[70:200], append=True).clone()
    assert a.append_stats == b.append_stats and a.append_stats["prefilled"] > 0 and a.append_stats["stepped"] + a.append_stats["prefilled"] == 130
    assert torch.equal(got, want) and a.position(1) == 200 and a.position(0) == 70
    _same_slots(a, b, [0, 1])
    a.prefill(2, ids[:5]), a.prefill(3, ids[:5]), b.prefill(2, ids[:5]), b.prefill(3, ids[:5])
    _step_both(a, b, [0, 1])


def test_fork_copies_the_sampler_history_once_it_exists(dev):
    from mobilequant_amd import SamplingParams
    _, a = _sampling_engines(dev, False)
    a.prefill(0, [3, 4, 5, 4])
    a.prefill(1, [9, 9])
    a.set_sampling(SamplingParams(temperature=0.7, repetition_penalty=1.3))
    a.observe_history(0, [3, 4, 5, 4])
    a.observe_history(1, [9, 9])
    a.fork({0: [2]})
    h = a._sampler.history.cpu()
    assert torch.equal(h[2], h[0]) and h[0].ne(0).sum().item() == 3 and not torch.equal(h[1], h[0]) and h[3].eq(0).all()


def _spied(eng, name):
    calls, orig = [], getattr(eng, name)

    def spy(*args, **kw):
        calls.append(args)
        return orig(*args, **kw)
    setattr(eng, name, spy)
    return calls


def _generate_n(ref, eng, prompts, k, sps, streams, new, **kw):
    """generate(n=k) against the single engine per stream AND against generate with every prompt repeated k times; the prompt is
    encoded len(prompts) times, not len(prompts) * k.  Returns the nested ids."""
    per_prompt = sps if isinstance(sps, list) else [sps] * len(prompts)
    st = list(range(len(prompts) * k)) if streams is None else streams
    fills, starts = _spied(eng, "_prefill_fill"), _spied(eng, "start")
    try:
        got = eng.generate(prompts, new, sampling=sps, streams=streams, n=k, **kw)
    finally:
        del eng._prefill_fill, eng.start
    long = sum(len(p) > 1 for p in prompts)
    assert len(fills) == long and len(starts) == len(prompts) - long, (len(fills), len(starts))
    if k > 1:
        assert eng.fork_stats["sources"] == len(prompts) and eng.fork_stats["destinations"] == len(prompts) * (k - 1)
    flat = eng.generate([p for p in prompts for _ in range(k)], new, sampling=[s for s in per_prompt for _ in range(k)], streams=st, **kw)
    alone = [[ref.generate(p, new, sampling=per_prompt[i], stream=st[i * k + j], **kw) for j in range(k)] for i, p in enumerate(prompts)]
    if "logprobs" in kw:
        (got, recs), (flat, frecs) = got, flat
        for i in range(len(prompts)):
            for j in range(k):
                one, two, three = recs[i][j], frecs[i * k + j], alone[i][j][1]
                assert len(one.logprob) == len(got[i][j]) - len(prompts[i])
                for f in one._fields:
                    x, y, z = getattr(one, f), getattr(two, f), getattr(three, f)
                    assert x.dtype == y.dtype and torch.equal(x.view(torch.int32), y.view(torch.int32)), (i, j, f)
                    assert torch.equal(x.view(torch.int32), z.view(torch.int32)), (i, j, f)
        alone = [[o[0] for o in row] for row in alone]
    assert len(got) == len(prompts) and all(len(row) == k for row in got)
    assert got == [flat[i * k:(i + 1) * k] for i in range(len(prompts))]
    assert got == alone
    assert all(not eng.active(s) for s in range(B))
    return got


@CAPTURED
def test_generate_n_draws_every_sample_from_one_encoding(dev, captured):
    from mobilequant_amd import SamplingParams
    ref, eng = _sampling_engines(dev, captured)
    m = eng.model
    p, q = _ids(m, 37, seed=11), _ids(m, 21, seed=14)
    sp = SamplingParams(temperature=1.0, top_k=30, seed=5)
    sq = SamplingParams(temperature=0.9, top_p=0.95, seed=6)
    NEW = 16
    four = _generate_n(ref, eng, [p], 4, sp, None, NEW)[0]
    assert len({tuple(o) for o in four}) > 1                       # different streams: different continuations of one prompt
    _generate_n(ref, eng, [p, q], 2, [sp, sq], [11, 12, 2 ** 63 + 5, 14], NEW)
    _generate_n(ref, eng, [p], 1, sp, [3], NEW)
    # log-probability records nest the same way, bit for bit
    _generate_n(ref, eng, [p, q], 2, [sp, sq], None, NEW, logprobs=2)
    # one-token prompts go through the step path, once per prompt
    _generate_n(ref, eng, [[7]], 4, sp, None, NEW)
    _generate_n(ref, eng, [[7], q], 2, [sq, sp], None, NEW)
    # a penalised request with a logit bias: every slot's prompt history is written by generate itself
    pen = SamplingParams(temperature=0.9, seed=3, repetition_penalty=1.3, presence_penalty=0.2, frequency_penalty=0.1,
                         logit_bias={5: 2.0, 9: float("-inf")})
    _generate_n(ref, eng, [p], 4, pen, None, NEW)
    _generate_n(ref, eng, [q, p], 2, [pen, sp], None, NEW, logprobs=0)
    # an EOS that some samples hit and others do not
    new = [o[len(p):] for o in four]
    eos = next(t for t in new[0][:-1] if any(t not in other for other in new[1:]))
    cut = _generate_n(ref, eng, [p], 4, sp, None, NEW, eos_token_id=eos)[0]
    lens = [len(o) - len(p) for o in cut]
    assert min(lens) < NEW and max(lens) == NEW and cut[0][-1] == eos and cut[0] == four[0][:len(cut[0])]
    # nothing to draw: the prompts come back nested
    assert eng.generate([p, q], 0, sampling=sp, n=2) == [[p, p], [q, q]]


@CAPTURED
def test_generate_speculative_n_returns_plain_samplings_ids(dev, captured):
    from mobilequant_amd import SamplingParams
    from mobilequant_amd.decode import prompt_lookup_draft
    _, eng = _sampling_engines(dev, captured)
    V = eng.shape.vocab
    base = _ids(eng.model, 9, seed=12)
    p, q = ((base * 4)[:19]), ((base[3:] + base[:3]) * 4)[:30]     # they repeat themselves: prompt lookup finds something
    sps = [SamplingParams(temperature=0.8, seed=5), SamplingParams(temperature=0.8, seed=7, repetition_penalty=1.8, logit_bias={3: float("-inf")})]
    streams, NEW = [21, 22, 23, 24], 16
    plain = eng.generate([p, p, q, q], NEW, sampling=[sps[0], sps[0], sps[1], sps[1]], streams=streams)
    fills = _spied(eng, "_prefill_fill")
    try:
        got = eng.generate_speculative([p, q], NEW, prompt_lookup_draft(2), sampling=sps, streams=streams, n=2)
        assert len(fills) == 2
        assert got == [plain[:2], plain[2:]]
        assert eng.spec_stats["rounds"] >= 1 and eng.fork_stats["destinations"] == 2
        # drafts per prompt and per sample; an oracle per sample is accepted whole
        assert eng.generate_speculative([p, q], NEW, [prompt_lookup_draft(2), prompt_lookup_draft(3)], sampling=sps, streams=streams, n=2) == got
        oracle = [(lambda ids, k, t=t: t[len(ids):len(ids) + k]) for t in plain]
        assert eng.generate_speculative([p, q], NEW, oracle, sampling=sps, streams=streams, n=2) == got
        assert eng.spec_stats["accepted"] == eng.spec_stats["proposed"] > 0
        out, recs = eng.generate_speculative([p, q], NEW, prompt_lookup_draft(2), sampling=sps, streams=streams, n=2, logprobs=1)
        want, wrecs = eng.generate([p, q], NEW, sampling=sps, streams=streams, n=2, logprobs=1)
        assert out == want == got
        for i in range(2):
            for j in range(2):
                for f in recs[i][j]._fields:
                    assert torch.equal(getattr(recs[i][j], f).view(torch.int32), getattr(wrecs[i][j], f).view(torch.int32)), (i, j, f)
    finally:
        del eng._prefill_fill
    assert all(0 <= t < V for row in got for o in row for t in o)
