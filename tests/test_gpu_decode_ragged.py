"""GPU: ragged decode steps of the batched engine (csrc/mq_decode_rows.hip, BatchDecodeEngine.step_tokens / extend / rewind /
generate(draft=...)).

The single-token path is the oracle and the bar is bit identity.  Kernel: one mq_decode_attention_ragged launch against sequential
mq_decode_attention_batch launches at batch 1 over the named slots' caches (its out_q rows and every cache byte of every slot).
Engine: every step_tokens row against the logits of DecodeEngine.step() calls on that sequence alone, the caches against theirs, and
the slots a call does not name against their own bytes before it.  Speculative generation: the returned ids against plain greedy
generate, token for token, for every kind of draft."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_gpu_decode_batch import _model  # noqa: E402
from test_gpu_decode_grouped import _model as _grouped_model  # noqa: E402

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _clone_struct(s):
    c = type(s)()
    ctypes.pointer(c)[0] = s
    return c


# ---- kernel ---------------------------------------------------------------------------------------------------------------------
def _run(slot, p, n):
    return [(slot, p + i) for i in range(n)]


def _check_ragged_launch(eng, table, gen, tail=()):
    """One mq_decode_attention_ragged launch over random caches / q|k|v rows against sequential mq_decode_attention_batch launches at
    batch 1, row by row in table order (a run's rows each append their own position in front of the next).  table: (sequence,
    position) per row, any of them idle; tail: table entries behind `rows`, which the launch must not look at."""
    from mobilequant_amd import _lib
    from mobilequant_amd._lib import MqDecodeAttentionBatchArgs
    if eng._rows is None:
        eng._lower_rows()
    ra = next(a for k, a in eng._rows[0] if k == "attn_ragged")          # layer 0
    R, B, s, CL, dev = len(table), eng.batch, eng.shape, eng.cache_len, eng.dev
    assert 1 <= R and R + len(tail) <= eng.max_rows
    ra.rows = R
    HD = s.heads * s.head_dim
    full = list(table) + list(tail)
    eng.row_seq.fill_(-1)
    eng.row_pos.fill_(CL)
    eng.row_seq[:len(full)] = torch.tensor([q for q, _ in full], dtype=torch.int32)
    eng.row_pos[:len(full)] = torch.tensor([p for _, p in full], dtype=torch.int32)
    eng.rqkv.copy_(torch.randn(eng.rqkv.shape, generator=gen).to(dev) * 2)
    kc = torch.randint(-128, 128, eng.k_cache[0].shape, generator=gen, dtype=torch.int8).to(dev)
    vc = torch.randint(-128, 128, eng.v_cache[0].shape, generator=gen, dtype=torch.int8).to(dev)
    eng.k_cache[0].copy_(kc)
    eng.v_cache[0].copy_(vc)
    eng.rattn_q.fill_(85)
    _lib.call("mq_decode_attention_ragged", ctypes.byref(ra), _st())
    torch.cuda.synchronize()
    got_q, got_k, got_v = eng.rattn_q.clone(), eng.k_cache[0].clone(), eng.v_cache[0].clone()
    k1, v1 = kc.clone(), vc.clone()
    part = torch.zeros(eng.LONG_SPLITS, HD, dtype=torch.int64, device=dev)
    ticket = torch.zeros(s.heads, dtype=torch.int32, device=dev)
    for r, (q, p) in enumerate(table):
        oq = torch.full((HD,), 85, dtype=torch.int8, device=dev)      # an idle row keeps the sentinel
        if 0 <= q < B and 0 <= p < CL:
            a = _clone_struct(ra.a)
            pos_t = torch.tensor([p], dtype=torch.int32, device=dev)
            a.qkv, a.k_cache, a.v_cache, a.out_q, a.pos = eng.rqkv[r].data_ptr(), k1[q].data_ptr(), v1[q].data_ptr(), oq.data_ptr(), pos_t.data_ptr()
            a.part, a.ticket = part.data_ptr(), ticket.data_ptr()
            b = MqDecodeAttentionBatchArgs()
            b.a, b.batch, b.split_from, b.qkv_stride = a, 1, ra.split_from, ra.qkv_stride
            _lib.call("mq_decode_attention_batch", ctypes.byref(b), _st())
            torch.cuda.synchronize()
        assert torch.equal(got_q[r], oq), (table, r)
    assert torch.equal(got_k, k1), table                           # every slot, named or not
    assert torch.equal(got_v, v1), table
    assert bool((got_q[R:] == 85).all()), table                     # no row behind `rows` was written
    assert bool((eng.rticket == 0).all()), table                    # the tickets are ready for the next launch


@pytest.mark.parametrize("geom", ["llama", "stablelm", "gemma"])
def test_attention_ragged_launch_is_sequential_single_launches(dev, geom):
    """Runs of 1..8 rows from positions on both sides of a 16-position chunk, a 64-position block and the split threshold (768) and
    up to past cache_len; two to four runs on different slots (equal positions included); idle rows (sequence -1, = batch, a position
    outside the cache) at the start, between runs and at the end: the output images and every cache byte of every slot equal
    sequential batch-1 launches."""
    from mobilequant_amd.decode_batch import BatchDecodeEngine
    m = _model(dev, geom, 1, 8)
    CL, B = 1024, 4
    eng = BatchDecodeEngine(m, B, cache_len=CL)
    assert eng.max_rows == 8
    gen = torch.Generator().manual_seed(7)
    for i, p in enumerate((0, 1, 15, 16, 17, 63, 64, 65, 760, 767, 768, 769, CL - 9, CL - 1)):
        for n in range(1, 9):
            _check_ragged_launch(eng, _run((i + n) % B, p, n), gen)      # (from CL - 9 / CL - 1 on: rows that run past the cache)
    idle_lo, idle_hi, idle_pos = (-1, 5), (B, 5), (2, -1)
    tables = [
        _run(0, 63, 3) + _run(1, 63, 1) + _run(3, 766, 4),             # equal positions on two slots; across a block and the threshold
        [idle_lo] + _run(1, 15, 3) + [idle_hi] + _run(2, 0, 2) + [idle_lo],
        _run(0, CL - 2, 4) + _run(2, 760, 4),                          # a run that runs past cache_len
        _run(0, 5, 1) + _run(1, 5, 2) + _run(2, 768, 2) + _run(3, 1, 3),      # four runs
        _run(2, 17, 1) + [idle_pos] + _run(3, 17, 2) + [idle_hi],
        [(0, 10), (1, 11), (2, 12), (3, 13)],                          # positions rising by one on DIFFERENT slots: four runs of one row
        [(1, 64), (0, 65), (2, 66)],
        _run(3, 765, 5) + [idle_lo] + _run(0, 767, 2),
        [idle_hi, idle_lo, idle_pos] + _run(1, 62, 5),
        _run(0, 64, 2) + _run(1, 64, 2) + _run(2, 64, 2) + _run(3, 64, 2),
        [idle_lo] * 8,
    ]
    for t in tables:
        assert len(t) <= 8
        _check_ragged_launch(eng, t, gen)
    # fewer rows than the table holds: the entries behind `rows` are not looked at (their positions keep their cache bytes)
    _check_ragged_launch(eng, _run(1, 100, 3), gen, tail=_run(1, 103, 2) + _run(0, 7, 1))
    _check_ragged_launch(eng, _run(2, 766, 1), gen, tail=_run(2, 767, 3))


# ---- engine ---------------------------------------------------------------------------------------------------------------------
RECIPES = {"w8a8": lambda dev, geom, layers: _model(dev, geom, layers, 8),
           "w4a8": lambda dev, geom, layers: _model(dev, geom, layers, 4),
           "w4g128": lambda dev, geom, layers: _grouped_model(dev, geom, layers, 4, 128)}


def _oracle(ref, prompt, toks):
    """The single-sequence oracle: prefill, then one DecodeEngine.step() per token -> ([logits after each token], caches)."""
    ref.reset()
    ref.prefill(prompt)
    out = [ref.step(t).clone() for t in toks]
    n = ref.position()
    return out, [(ref.k_cache[li][:, :n].clone(), ref.cached_values(li, n).clone()) for li in range(len(ref.k_cache))]


def _snapshot(eng):
    return eng.logits.clone(), [c.clone() for c in eng.k_cache], [c.clone() for c in eng.v_cache]


def _unchanged(eng, snap, slots, tag):
    lg, ks, vs = snap
    for b in slots:
        assert torch.equal(eng.logits[b], lg[b]), (tag, b)
        for li in range(len(ks)):
            assert torch.equal(eng.k_cache[li][b], ks[li][b]) and torch.equal(eng.v_cache[li][b], vs[li][b]), (tag, b, li)


def _same_caches(eng, slot, want, tag):
    for li, (k, v) in enumerate(want):
        n = k.shape[1]
        assert eng.position(slot) == n, (tag, slot)
        assert torch.equal(eng.cached_keys(slot, li, n), k) and torch.equal(eng.cached_values(slot, li, n), v), (tag, slot, li)


PLANS = [{0: 3, 1: 1, 3: 4}, "step", {1: 8}, {0: 1, 1: 1, 2: 1, 3: 1}, "step", {2: 7, 0: 1}]


def _run_plans(dev, m, captured, tag):
    from mobilequant_amd.decode import DecodeEngine
    from mobilequant_amd.decode_batch import BatchDecodeEngine
    B, CL, V = 4, 848, m.shape.vocab
    g = torch.Generator().manual_seed(4)
    ref = DecodeEngine(m, cache_len=CL)
    eng = BatchDecodeEngine(m, B, cache_len=CL)
    assert eng.max_rows == 8
    need = [sum(1 if p == "step" else p.get(b, 0) for p in PLANS) for b in range(B)]
    prompts = [torch.randint(0, V, (n,), generator=g).tolist() for n in (9, 700, 700, 9)]      # both split variants in one step
    toks = [torch.randint(0, V, (need[b],), generator=g).tolist() for b in range(B)]
    want = [_oracle(ref, prompts[b], toks[b]) for b in range(B)]
    for b in range(B):
        eng.prefill(b, prompts[b])
    if captured:
        eng.capture()
    used, counts, graphs_seen = [0] * B, set(), {}
    for plan in PLANS:
        snap, pos0 = _snapshot(eng), [eng.position(b) for b in range(B)]
        if plan == "step":
            named = {b: 1 for b in range(B)}
            lg = eng.step([toks[b][used[b]] for b in range(B)])
            rows = {b: lg[b:b + 1] for b in range(B)}
        else:
            named = plan
            rows = eng.step_tokens({b: toks[b][used[b]:used[b] + n] for b, n in plan.items()})
            assert sorted(rows) == sorted(plan)
            R = sum(plan.values())
            if captured:
                if R in counts:
                    assert eng._row_graphs[R] is graphs_seen[R], (tag, plan)      # a row count seen before records nothing new
                counts.add(R)
                assert set(eng._row_graphs) == counts, (tag, plan)
                graphs_seen[R] = eng._row_graphs[R]
        for b, n in named.items():
            assert rows[b].shape == (n, V)
            for r in range(n):
                assert torch.equal(rows[b][r], want[b][0][used[b] + r]), (tag, plan, b, r)
            assert torch.equal(eng.logits[b], want[b][0][used[b] + n - 1]), (tag, plan, b)
            used[b] += n
        assert [eng.position(b) for b in range(B)] == [pos0[b] + named.get(b, 0) for b in range(B)], (tag, plan)
        assert eng.pos.tolist() == [eng.position(b) for b in range(B)], (tag, plan)
        _unchanged(eng, snap, [b for b in range(B) if b not in named], (tag, plan))
    assert used == need
    for b in range(B):
        _same_caches(eng, b, want[b][1], tag)
    if not captured:
        assert eng._row_graphs == {}


@pytest.mark.parametrize("recipe", list(RECIPES))
@pytest.mark.parametrize("captured", [False, True], ids=["direct", "graph"])
def test_step_tokens_rows_are_single_steps_bit_for_bit(dev, recipe, captured):
    _run_plans(dev, RECIPES[recipe](dev, "llama", 2), captured, (recipe, captured))


@pytest.mark.parametrize("geom,recipe,captured", [("stablelm", "w8a8", True), ("gemma", "w4a8", False)])
def test_step_tokens_other_geometries(dev, geom, recipe, captured):
    _run_plans(dev, RECIPES[recipe](dev, geom, 1), captured, (geom, recipe, captured))


def test_extend_is_n_steps(dev):
    from mobilequant_amd.decode import DecodeEngine
    from mobilequant_amd.decode_batch import BatchDecodeEngine
    m = _model(dev, "llama", 2, 8)
    V, CL = m.shape.vocab, 128
    g = torch.Generator().manual_seed(6)
    ref, eng = DecodeEngine(m, cache_len=CL), BatchDecodeEngine(m, 3, cache_len=CL)
    prompts = [torch.randint(0, V, (n,), generator=g).tolist() for n in (13, 60, 5)]
    for b in range(3):
        eng.prefill(b, prompts[b])
    stepped = [[], [], []]
    for counts in ({0: 1}, {0: 13, 2: 5}, {1: 8, 2: 9}, {0: 3, 1: 30, 2: 2}):
        toks = {b: torch.randint(0, V, (n,), generator=g).tolist() for b, n in counts.items()}
        snap = _snapshot(eng)
        got = eng.extend(toks)
        assert got is eng.logits
        for b in counts:
            stepped[b] += toks[b]
            want, caches = _oracle(ref, prompts[b], stepped[b])
            assert torch.equal(got[b], want[-1]), (counts, b)
            _same_caches(eng, b, caches, (counts, b))
        _unchanged(eng, snap, [b for b in range(3) if b not in counts], counts)
    # the engine goes on with plain steps from there
    nxt = [1, 2, 3]
    lg = eng.step(nxt).clone()
    for b in range(3):
        want, _ = _oracle(ref, prompts[b], stepped[b] + [nxt[b]])
        assert torch.equal(lg[b], want[-1]), b


@pytest.mark.parametrize("captured", [False, True], ids=["direct", "graph"])
def test_rewind_forgets_the_dropped_positions(dev, captured):
    """Garbage tokens on one slot, rewind, then more steps (ragged and plain): the same bits as an engine that never saw the garbage --
    rewinds into the middle of a 16-position chunk and across a 64-position block included -- and the other slots bit-unchanged."""
    from mobilequant_amd.decode import DecodeEngine
    from mobilequant_amd.decode_batch import BatchDecodeEngine
    m = _model(dev, "llama", 2, 8)
    V, CL = m.shape.vocab, 256
    g = torch.Generator().manual_seed(9)
    ref, eng = DecodeEngine(m, cache_len=CL), BatchDecodeEngine(m, 3, cache_len=CL)
    prompts = [torch.randint(0, V, (n,), generator=g).tolist() for n in (58, 20, 70)]
    toks = [torch.randint(0, V, (24,), generator=g).tolist() for _ in range(3)]
    want = [_oracle(ref, prompts[b], toks[b]) for b in range(3)]
    for b in range(3):
        eng.prefill(b, prompts[b])
    if captured:
        eng.capture()
    junk = lambda n: torch.randint(0, V, (n,), generator=g).tolist()      # noqa: E731
    eng.step_tokens({0: junk(8)})                              # slot 0: 58 .. 65, across the 64-block, then dropped
    snap, pos = _snapshot(eng), eng.pos.clone()
    assert eng.rewind(0, 58) is eng
    assert eng.position(0) == 58 and eng.pos.tolist() == [58, 20, 70]
    _unchanged(eng, snap, [0, 1, 2], "rewind")                  # only the position moves
    assert torch.equal(eng.pos[1:], pos[1:])
    rows = eng.step_tokens({0: toks[0][:3] + junk(5)})         # 3 kept, 5 dropped (61 .. 65): inside a 16-position chunk
    for r in range(3):
        assert torch.equal(rows[0][r], want[0][0][r])
    eng.rewind(0, 61)
    used = [3, 0, 0]
    for _ in range(7):                                          # plain steps of all slots over the dropped bytes
        lg = eng.step([toks[b][used[b]] for b in range(3)])
        for b in range(3):
            assert torch.equal(lg[b], want[b][0][used[b]]), (b, used)
            used[b] += 1
    eng.step_tokens({0: junk(1), 2: junk(4)})
    eng.rewind(0, 68).rewind(2, 77)
    rows = eng.step_tokens({0: toks[0][10:14], 2: toks[2][7:11]})
    for r in range(4):
        assert torch.equal(rows[0][r], want[0][0][10 + r]) and torch.equal(rows[2][r], want[2][0][7 + r])
    eng.extend({0: toks[0][14:], 1: toks[1][7:], 2: toks[2][11:]})
    for b in range(3):
        assert torch.equal(eng.logits[b], want[b][0][-1]), b
        _same_caches(eng, b, want[b][1], (captured, b))
    with pytest.raises(ValueError):
        eng.rewind(0, eng.position(0) + 1)
    with pytest.raises(ValueError):
        eng.rewind(0, -1)
    with pytest.raises(IndexError):
        eng.rewind(3, 0)
    eng.release(1)
    with pytest.raises(RuntimeError, match="idle"):
        eng.rewind(1, 0)


def test_step_tokens_limits(dev):
    from mobilequant_amd.decode_batch import BatchDecodeEngine
    m = _model(dev, "llama", 1, 8)
    eng = BatchDecodeEngine(m, 3, cache_len=32)
    eng.start(0)
    eng.start(2)
    eng.extend({0: list(range(28))})
    assert eng.position(0) == 28 and eng.position(2) == 0
    snap = _snapshot(eng)
    with pytest.raises(RuntimeError, match="overflow"):
        eng.step_tokens({0: [1] * 5})
    with pytest.raises(RuntimeError, match="overflow"):
        eng.extend({2: [1] * 33})
    with pytest.raises(RuntimeError, match="idle"):
        eng.step_tokens({1: [1]})
    with pytest.raises(ValueError, match="outside 1..8"):
        eng.step_tokens({0: [1] * 4, 2: [1] * 5})
    with pytest.raises(ValueError, match="outside 1..8"):
        eng.step_tokens({})
    with pytest.raises(ValueError, match="no tokens"):
        eng.step_tokens({0: [1], 2: []})
    for bad in (3, -1):
        with pytest.raises(ValueError, match="outside 0..2"):
            eng.step_tokens({bad: [1]})
    _unchanged(eng, snap, [0, 1, 2], "refused")                 # a refused call has run nothing
    assert eng.pos.tolist() == [28, 32, 0]
    eng.step_tokens({0: [1] * 4, 2: [5]})
    assert eng.position(0) == 32 and eng.position(2) == 1
    small = BatchDecodeEngine(m, 2, cache_len=32, max_rows=3)
    assert small.max_rows == 3
    small.start(0)
    with pytest.raises(ValueError, match="outside 1..3"):
        small.step_tokens({0: [1] * 4})
    with pytest.raises(ValueError):
        BatchDecodeEngine(m, 2, cache_len=32, max_rows=0)


# ---- speculative ----------------------------------------------------------------------------------------------------------------
def _oracle_draft(ref_ids):
    """Proposes exactly what plain greedy returned: everything is accepted."""
    return lambda ids, k: ref_ids[len(ids):len(ids) + k]


def _always_wrong(ref_ids, vocab):
    return lambda ids, k: [(ref_ids[len(ids) + i] + 1) % vocab if len(ids) + i < len(ref_ids) else 0 for i in range(k)]


@pytest.mark.parametrize("n", [1, 3, 8])
def test_batch_speculative_greedy_is_plain_greedy(dev, n):
    """1, 3 and 8 prompts of different lengths: an EOS that occurs, max_new_tokens and the cache end cutting in the middle of a round."""
    from mobilequant_amd.decode import prompt_lookup_draft
    from mobilequant_amd.decode_batch import BatchDecodeEngine
    m = _model(dev, "llama", 2, 8)
    V, CL, N = m.shape.vocab, 96, 30
    g = torch.Generator().manual_seed(12)
    eng = BatchDecodeEngine(m, 8, cache_len=CL)
    base = torch.randint(0, V, (12,), generator=g).tolist()
    lens = [19, 1, 75, 40, 7, 90, 33, 64][:n]                   # 75 / 90 + 30 new tokens pass the cache end (96); a one-token prompt
    prompts = [((base[i:] + base[:i]) * 8)[:ln] for i, ln in enumerate(lens)]      # they repeat themselves: prompt lookup finds something
    plain = eng.generate(prompts, N)
    for i, ln in enumerate(lens):
        assert len(plain[i]) == min(ln + N, CL + 1), (i, ln)
    eos = plain[0][lens[0] + 6]
    plain_eos = eng.generate(prompts, N, eos_token_id=eos)
    assert len(plain_eos[0]) < len(plain[0])                    # the EOS occurs
    for captured in (False, True):
        if captured:
            eng.capture()
        for nd in ((3,) if captured else (1, 3, 7)):
            for name, drafts in (("oracle", [_oracle_draft(p) for p in plain]), ("wrong", [_always_wrong(p, V) for p in plain]),
                                 ("lookup", prompt_lookup_draft(3))):
                got = eng.generate(prompts, N, draft=drafts, num_draft=nd)
                assert got == plain, (n, captured, nd, name)
                st = eng.spec_stats
                assert st["target_steps"] == st["rounds"] >= 1 and st["accepted"] <= st["proposed"]
                if name == "oracle":
                    assert st["accepted"] == st["proposed"], st
                    if n < 8:                                   # (eight live slots leave no spare rows: plain steps)
                        assert st["proposed"] > 0, st
                if name == "wrong":
                    assert st["accepted"] == 0, st
                assert all(not eng.active(b) for b in range(8))
            drafts_eos = [_oracle_draft(p) for p in plain]      # the oracle of the run WITHOUT an EOS: accepted up to the EOS, cut there
            assert eng.generate(prompts, N, eos_token_id=eos, draft=drafts_eos, num_draft=nd) == plain_eos, (n, captured, nd, "eos")
            assert eng.generate(prompts, N, eos_token_id=eos, draft=prompt_lookup_draft(2), num_draft=nd) == plain_eos, (n, captured, nd, "eos lookup")
        # max_new_tokens in the middle of a round (rounds of nd + 1 tokens behind the first one)
        for N2 in (2, 11):
            want = eng.generate(prompts, N2)
            assert eng.generate(prompts, N2, draft=[_oracle_draft(p) for p in plain], num_draft=3) == want, (n, captured, N2)


def test_batch_speculative_refusals(dev):
    from mobilequant_amd.decode import DecodeEngine
    from mobilequant_amd.decode_batch import BatchDecodeEngine
    from mobilequant_amd.sampling import SamplingParams
    m = _model(dev, "llama", 1, 8)
    eng = BatchDecodeEngine(m, 2, cache_len=64)
    d = lambda ids, k: []      # noqa: E731
    with pytest.raises(ValueError, match="greedy"):
        eng.generate([[1, 2, 3]], 4, do_sample=True, draft=d)
    with pytest.raises(ValueError, match="greedy"):
        eng.generate([[1, 2, 3]], 4, sampling=SamplingParams(temperature=0.7, seed=1), draft=d)
    with pytest.raises(TypeError, match="callable drafts"):
        eng.generate([[1, 2, 3]], 4, draft=DecodeEngine(m, cache_len=64))
    with pytest.raises(TypeError, match="callable drafts"):
        eng.generate([[1, 2, 3], [4]], 4, draft=[d, eng])
    with pytest.raises(TypeError):
        eng.generate([[1, 2, 3]], 4, draft=5)
    with pytest.raises(ValueError, match="drafts for"):
        eng.generate([[1, 2, 3], [4]], 4, draft=[d])
    with pytest.raises(ValueError, match="num_draft"):
        eng.generate([[1, 2, 3]], 4, draft=d, num_draft=-1)
    assert eng.generate([[1, 2, 3], [4]], 4, draft=[d, d]) == eng.generate([[1, 2, 3], [4]], 4)
