"""The speculative generation loops of DecodeEngine (generate(draft=...), generate_speculative) without a GPU and without the library:
a stand-in engine whose "model" is a deterministic function prefix -> logits row over 32 tokens runs the real loops on CPU tensors.
The reference is the plain loop on the same stand-in (generate(...), generate(sampling=...)); the speculative ids must equal it token
for token whatever the draft proposes, and afterwards the caches (here: a Python list) must hold out[:position()].

The stand-in's "sampled" selection is argmax(row + noise[index]) over one fixed noise table: token n is a function of its logits row
and n alone, which is the property of mq_sample's rule that the loop relies on.  A row at or past cache_len is idle (the token stays),
as in the kernels.

Not covered here: the history bookkeeping under a penalised request (history_count on device tensors).  tests/test_gpu_spec_sample.py
pins it; the stand-in's _sampler says penalized = False."""
import math
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mobilequant_amd import SamplingParams  # noqa: E402
from mobilequant_amd.decode import DecodeEngine, prompt_lookup_draft  # noqa: E402

V = 32
NOISE = 3.0 * torch.randn(256, V, generator=torch.Generator().manual_seed(1234))      # one table for every stand-in: shared "Gumbel noise"
SP = SamplingParams(temperature=0.8, seed=5)
CTX = [3, 1, 4, 1, 5]
LOOP_CTX = [1, 2, 3, 4] * 3 + [1, 2, 3]
_ROWS = {}


def model_row(seed: int, mix: float, loop: bool, prefix) -> torch.Tensor:
    """Logits after `prefix` (all of it: a stale cached position anywhere changes the row): a base row every model shares plus `mix` of
    the model's own (mix 0: the target's model).  loop: the row also favours the token behind the last one in the cycle 1 2 3 4, so that
    the sequence repeats itself."""
    key = (seed, mix, loop, tuple(prefix))
    if key not in _ROWS:
        row = torch.randn(V, generator=torch.Generator().manual_seed(hash(key[2:]) & (2 ** 62 - 1)))
        if mix:
            row = row + mix * torch.randn(V, generator=torch.Generator().manual_seed(hash(key) & (2 ** 62 - 1)))
        if loop:
            row[prefix[-1] % 4 + 1] += 8.0
        _ROWS[key] = row
    return _ROWS[key]


class ToyEngine(DecodeEngine):
    """What the generation loops touch of an engine, on CPU tensors; the cache is the list `prefix`."""

    def __init__(self, cache_len: int = 64, max_rows: int = 8, seed: int = 0, mix: float = 0.0, loop: bool = False, shrink_to=None):
        self.model_key = (seed, mix, loop)
        self.cache_len, self.max_rows, self.shrink_to = cache_len, max_rows, shrink_to
        self.shape, self.dev = types.SimpleNamespace(vocab=V), torch.device("cpu")
        self.logits, self.tok = torch.zeros(V), torch.zeros(1, dtype=torch.int64)
        self.rlogits, self.rsel = torch.zeros(max_rows, V), torch.zeros(max_rows, dtype=torch.int64)
        self._sampler, self._host_pos, self.prefix, self.spec_stats = None, 0, [], None

    def _push(self, token: int) -> torch.Tensor:
        assert len(self.prefix) == self._host_pos < self.cache_len
        self.prefix.append(int(token))
        self._host_pos += 1
        return model_row(*self.model_key, self.prefix)

    def set_sampling(self, sampling, stream: int = 0):
        assert isinstance(sampling, SamplingParams)
        self._sampler = types.SimpleNamespace(penalized=False)
        return self

    def _start_sequence(self, ids, prefill):
        if self.shrink_to is not None:
            # generate asserts that the request fits the cache, so the loops' cache-end stops are reachable only where that assert
            # is off; the stand-in's cache shrinks behind the assert to reach them
            self.cache_len = self.shrink_to
        self.prefix, self._host_pos = [], 0
        for t in ids:
            self.logits.copy_(self._push(t))

    def step(self, token=None):
        if self._host_pos >= self.cache_len:
            raise RuntimeError("ToyEngine.step: the KV cache is full")
        self.logits.copy_(self._push(int(self.tok) if token is None else token))
        return self.logits

    def step_tokens(self, tokens):
        t = [int(v) for v in tokens]
        if not 1 <= len(t) <= self.max_rows:
            raise ValueError(f"ToyEngine.step_tokens: {len(t)} tokens outside 1..{self.max_rows}")
        if self._host_pos + len(t) > self.cache_len:
            raise RuntimeError("ToyEngine.step_tokens: overflow")
        for j, v in enumerate(t):
            self.rlogits[j].copy_(self._push(v))
        self.logits.copy_(self.rlogits[len(t) - 1])
        return self.rlogits[:len(t)]

    def extend(self, tokens):
        t = [int(v) for v in tokens]
        if self._host_pos + len(t) > self.cache_len:
            raise RuntimeError("ToyEngine.extend: overflow")
        for i in range(0, len(t), self.max_rows):
            self.step_tokens(t[i:i + self.max_rows])
        return self.logits

    def rewind(self, n):
        if not 0 <= int(n) <= self._host_pos:
            raise ValueError(f"ToyEngine.rewind: n={n} outside 0..{self._host_pos}")
        del self.prefix[int(n):]
        self._host_pos = int(n)
        return self

    def _draw(self, row: torch.Tensor, index: int, out: torch.Tensor):
        if index < self.cache_len:                                 # (an idle row keeps its token)
            out.fill_(int(torch.argmax(row + NOISE[index])))

    def sample(self):
        assert self._sampler is not None and self._host_pos < self.cache_len      # (the loops never draw a token from an idle row)
        self._draw(self.logits, self._host_pos, self.tok)
        return self.tok

    def sample_step(self):
        if self._host_pos >= self.cache_len:
            raise RuntimeError("ToyEngine.sample_step: the KV cache is full")
        self.sample()
        return self.step()

    def step_sample_tokens(self, tokens):
        P = self._host_pos
        rows = self.step_tokens(tokens)
        for j in range(rows.shape[0]):
            self._draw(rows[j], P + 1 + j, self.rsel[j:j + 1])
        return self.rsel[:rows.shape[0]]


def plain(sampled: bool, ctx, new: int, eos=None, **kw):
    eng = ToyEngine(**kw)
    out = eng.generate(ctx, new, eos_token_id=eos, sampling=SP if sampled else None)
    assert eng.prefix == out[:eng.position()]
    return out


def speculate(sampled: bool, eng: ToyEngine, ctx, new: int, draft, num_draft: int, eos=None):
    if sampled:
        return eng.generate_speculative(ctx, new, draft, sampling=SP, num_draft=num_draft, eos_token_id=eos)
    return eng.generate(ctx, new, eos_token_id=eos, draft=draft, num_draft=num_draft)


def make_draft(kind: str, truth):
    """truth: the plain ids far past every request (context included)."""
    right = lambda ids, k: truth[len(ids):len(ids) + k]      # noqa: E731
    if kind == "right":
        return right
    if kind == "wrong":
        return (lambda ids, k: [(t + 1) % V for t in right(ids, k)])
    if kind == "two_fewer":
        return (lambda ids, k: right(ids, max(0, k - 2)))
    if kind == "empty":
        return (lambda ids, k: [])
    if kind == "lookup":
        return prompt_lookup_draft(3)
    if kind == "engine_same":
        return ToyEngine()
    if kind == "engine_other":
        return ToyEngine(mix=0.7, seed=9, max_rows=3)
    if kind == "engine_short":
        return ToyEngine(cache_len=len(CTX) + 4)      # its cache ends inside the generation: both kd bounds
    raise KeyError(kind)


def check(eng, out, want, draft, num_draft):
    assert out == want
    st = eng.spec_stats
    assert set(st) == {"rounds", "proposed", "accepted", "target_steps"}
    assert st["target_steps"] == st["rounds"] and 0 <= st["accepted"] <= st["proposed"] <= st["rounds"] * max(0, min(num_draft, eng.max_rows - 1))
    assert eng.prefix == out[:eng.position()] and len(eng.prefix) == eng.position()
    if isinstance(draft, ToyEngine):
        assert draft.prefix == out[:len(draft.prefix)] and len(draft.prefix) == draft.position()


KINDS = ["right", "wrong", "two_fewer", "empty", "lookup", "engine_same", "engine_other", "engine_short"]


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
@pytest.mark.parametrize("kind", KINDS)
def test_speculative_ids_are_the_plain_ids(kind, sampled):
    loop = kind == "lookup"                                        # a self-repeating context under a model that goes on repeating it
    ctx = LOOP_CTX if loop else CTX
    truth = plain(sampled, ctx, 24, loop=loop)
    # an EOS in the middle of a round: the third new token (first token, then the second of round 1's rows), if it is new there
    eos_at = next(i for i in range(len(ctx) + 2, len(truth)) if truth[i] not in truth[len(ctx):i])
    accepted_some = False
    for max_rows in (3, 8):
        for num_draft in (0, 1, 4, 7):
            for new in (0, 1, 2, 9):
                for eos in (None, truth[eos_at]):
                    draft = make_draft(kind, truth)
                    eng = ToyEngine(max_rows=max_rows, loop=loop)
                    want = plain(sampled, ctx, new, eos, max_rows=max_rows, loop=loop)
                    out = speculate(sampled, eng, ctx, new, draft, num_draft, eos)
                    check(eng, out, want, draft, num_draft)
                    assert want == truth[:len(want)] and len(want) <= len(ctx) + new
                    st, made = eng.spec_stats, len(out) - len(ctx)
                    accepted_some |= st["accepted"] > 0
                    if new <= 1:
                        assert st["rounds"] == 0
                    if kind in ("right", "engine_same"):
                        kk = min(num_draft, max_rows - 1)          # (== num_draft wherever the step has the rows for it)
                        assert st["rounds"] == math.ceil(max(0, made - 1) / (kk + 1))
                        if eos is None:                            # (an EOS may cut a round's last proposals)
                            assert st["accepted"] == st["proposed"] == max(0, made - 1) - st["rounds"]
                    if kind in ("wrong", "empty"):
                        assert st["accepted"] == 0 and st["rounds"] == max(0, made - 1)
    if kind in ("two_fewer", "lookup", "engine_other", "engine_short"):
        assert accepted_some                                       # (the case is not vacuous)


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
@pytest.mark.parametrize("kind", ["right", "wrong", "two_fewer", "engine_same", "engine_other"])
def test_the_cache_end_stops_the_sequence_where_plain_generate_stops(kind, sampled):
    """A target whose cache ends before max_new_tokens: every position is cached and one more token is returned.  Greedy: the ids of
    the plain loop on the same short cache.  Sampled: the plain loop has no cache-end stop (sample_step refuses), so the reference is
    the plain ids of a long cache up to the cache's end; the one token behind it would be drawn at index cache_len, an idle row."""
    truth = plain(sampled, CTX, 24)
    end = len(CTX) + 5
    for max_rows in (3, 8):
        for num_draft in (0, 1, 4, 7):
            draft = make_draft(kind, truth)
            eng = ToyEngine(max_rows=max_rows, shrink_to=end)
            out = speculate(sampled, eng, CTX, 9, draft, num_draft)
            assert len(out) == end + 1 < len(CTX) + 9
            # sampled: out[end] comes from an idle row, so its value is unspecified and deliberately not compared: only that ONE token is returned
            want = truth[:end] + out[end:] if sampled else plain(False, CTX, 9, shrink_to=end, max_rows=max_rows)
            check(eng, out, want, draft, num_draft)
            assert eng.position() == end


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
def test_a_draft_that_is_no_decode_engine_is_refused_before_the_target_moves(sampled):
    """Only a DecodeEngine drafts as an engine: a BatchDecodeEngine (not callable) is refused like any other object, a negative
    num_draft and the target itself too, and the target has not started a sequence or taken a sampling request by then."""
    from mobilequant_amd.decode_batch import BatchDecodeEngine
    eng = ToyEngine()
    eng._start_sequence([7, 8], True)
    for bad in (object.__new__(BatchDecodeEngine), 5, "lookup"):
        with pytest.raises(TypeError, match="draft must be a DecodeEngine or a callable"):
            speculate(sampled, eng, CTX, 4, bad, 4)
    with pytest.raises(ValueError, match="num_draft"):
        speculate(sampled, eng, CTX, 4, lambda ids, k: [], -1)
    with pytest.raises(ValueError, match="another engine"):
        speculate(sampled, eng, CTX, 4, eng, 4)
    assert eng.prefix == [7, 8] and eng.position() == 2 and eng._sampler is None and eng.spec_stats is None


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
def test_a_bool_num_draft_is_refused_by_both_entry_points(sampled):
    """One validator serves generate(draft=...), generate_speculative and BatchDecodeEngine.generate.  The last two always refused a
    bool num_draft; generate(draft=...) used to read True as 1 and refuses it with them since the validator is shared."""
    eng = ToyEngine()
    for bad in (True, False):
        with pytest.raises(ValueError, match="num_draft"):
            speculate(sampled, eng, CTX, 4, lambda ids, k: [], bad)
    assert eng.prefix == [] and eng._sampler is None


def test_the_stand_in_samples_differently_from_greedy_and_drafts_disagree():
    """The cases above are not vacuous: sampled ids differ from greedy ones, and the other model's greedy ids differ from the target's."""
    assert plain(False, CTX, 12) != plain(True, CTX, 12)
    assert plain(False, CTX, 12) != plain(False, CTX, 12, mix=0.7, seed=9)
