"""Speculative decoding under seeded sampling in the batched engine (mq_sample_ragged, mq_sample_history_count_ragged,
BatchDecodeEngine.generate_speculative) without a GPU: the ABI (declared, bound, struct layout, every refusal before
any HIP call; pointers are fake and never read), the refusals of the Python surface, and the batch round itself on a stand-in engine.

The stand-in runs the real generate / generate_speculative / _generate_speculative of BatchDecodeEngine on CPU tensors.  Every slot's
"model" is test_spec_host.model_row, a deterministic function prefix -> logits row; "sampling" is argmax(row + NOISE[stream][index]):
token n of a sequence is a function of its logits row, its stream and n alone, which is the property of mq_sample's rule that the round
relies on.  The reference is the plain per-prompt loop written out below; the speculative ids must equal it token for token whatever
the drafts propose and whatever else is in the batch, and afterwards every slot's cache (a Python list) must hold out[:position].

Not covered here: the history bookkeeping under a penalised request (device tensors; tests/test_gpu_spec_sample_batch.py pins it)."""
import ctypes
import math
import os
import re
import subprocess
import sys
import tempfile
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_spec_host import V, model_row  # noqa: E402

from mobilequant_amd import SamplingParams  # noqa: E402
from mobilequant_amd.decode import prompt_lookup_draft  # noqa: E402
from mobilequant_amd.decode_batch import BatchDecodeEngine  # noqa: E402

P = 0x10000
SP = SamplingParams(temperature=0.8, seed=5)
STREAMS = [11, 3, 7, 0, 5, 2, 9, 4]
NOISE = 3.0 * torch.randn(12, 96, V, generator=torch.Generator().manual_seed(4321))      # [stream][index]: the shared "Gumbel noise"


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from mobilequant_amd import _lib, build
    build.build()
    return _lib.load()


def _args(**kw):
    from mobilequant_amd._lib import MQ_SAMPLE_SCRATCH_BYTES, MqSampleRaggedArgs
    a = MqSampleRaggedArgs()
    a.logits, a.row_seq, a.row_pos, a.row_tok, a.params, a.tok, a.scratch = P, P, P, P, P, P, P
    a.logits_stride, a.V, a.rows, a.batch, a.cache_len, a.n_offset, a.scratch_bytes = 32000, 32000, 5, 4, 64, 1, MQ_SAMPLE_SCRATCH_BYTES
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _rejects(lib, a, text):
    rc = lib.mq_sample_ragged(ctypes.byref(a), None)
    msg = lib.mq_last_error()
    assert rc == 1 and text.encode() in msg and b"mq_sample_ragged" in msg, (rc, msg, text)


def test_entries_are_declared_exported_and_the_struct_matches_the_header(lib):
    from mobilequant_amd import _lib
    from mobilequant_amd._lib import MqSampleRaggedArgs
    for name in ("mq_sample_ragged", "mq_sample_history_count_ragged"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    hdr = open(os.path.join(ROOT, "include", "mobilequant_amd.h")).read()
    assert re.search(r"int mq_sample_ragged\(const mq_sample_ragged_args\* args, mq_stream_t stream\);", hdr)
    assert re.search(r"int mq_sample_history_count_ragged\(uint32_t\* history, int64_t history_stride, int64_t V, int batch, const int64_t\* pairs, "
                     r"int64_t n, int delta,\s+mq_stream_t stream\);", hdr)
    ver = int(re.search(r"#define MQ_VERSION (\d+)", hdr).group(1))
    assert ver // 100 == _lib.HEADER_MAJOR == lib.mq_version() // 100                       # additive entries: the major stays
    af = [f for f, _ in MqSampleRaggedArgs._fields_]
    assert af == ["logits", "logits_stride", "V", "rows", "batch", "cache_len", "row_seq", "row_pos", "n_offset", "row_tok", "params", "penalty",
                  "history", "history_stride", "bias", "tok", "kept", "logprob", "scratch", "scratch_bytes"]
    src = "\n".join(["#include <stddef.h>", "#include <stdio.h>", '#include "mobilequant_amd.h"', "int main(void) {",
                     '  printf("%zu' + " %zu" * len(af) + '\\n", sizeof(mq_sample_ragged_args), ' + ", ".join(f"offsetof(mq_sample_ragged_args, {f})" for f in af) + ");",
                     "  return 0;", "}"])
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        open(c, "w").write(src)
        cc = next((x for x in ("cc", "gcc", "clang") if subprocess.run(["which", x], stdout=subprocess.PIPE).returncode == 0), None)
        if cc is None:
            cc = "/opt/rocm/llvm/bin/clang"
        subprocess.run([cc, "-I" + os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        out = subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")
    assert [int(v) for v in out[0].split()] == [ctypes.sizeof(MqSampleRaggedArgs)] + [getattr(MqSampleRaggedArgs, f).offset for f in af]


def test_rejects_argument_blocks_outside_the_limits(lib):
    assert lib.mq_sample_ragged(None, None) == 1 and b"null argument block" in lib.mq_last_error()
    for f in ("row_seq", "row_pos", "row_tok"):
        _rejects(lib, _args(**{f: None}), "the row table row_seq / row_pos and row_tok are required")
    for f in ("logits", "params", "tok", "scratch"):
        _rejects(lib, _args(**{f: None}), "null pointer")
    for r in (0, 9, -1):
        _rejects(lib, _args(rows=r), "rows=%d outside 1..8" % r)
        _rejects(lib, _args(batch=r), "batch=%d outside 1..8" % r)
    _rejects(lib, _args(V=31999), "V=31999")
    _rejects(lib, _args(V=(1 << 20) + 4, logits_stride=(1 << 20) + 4), "multiple of 4 in [4, 2^20]")
    _rejects(lib, _args(V=0), "V=0")
    _rejects(lib, _args(logits_stride=31996), "logits_stride=31996")
    _rejects(lib, _args(logits_stride=32002), "logits_stride=32002")
    _rejects(lib, _args(cache_len=0), "cache_len=0")
    _rejects(lib, _args(logits=P + 8), "16-byte aligned")
    _rejects(lib, _args(params=P + 8), "16-byte aligned")
    _rejects(lib, _args(tok=P + 4), "8-byte")
    _rejects(lib, _args(row_pos=P + 2), "4-byte aligned")
    _rejects(lib, _args(kept=P + 2), "4-byte aligned")
    _rejects(lib, _args(scratch_bytes=4096), "scratch_bytes=4096")
    for bad in ((1 << 30) + 1, -(1 << 30) - 1):
        _rejects(lib, _args(n_offset=bad), "n_offset=%d" % bad)
    for stride in (0, 31996, 32002):
        _rejects(lib, _args(penalty=P, history_stride=stride), "history_stride=%d" % stride)
        _rejects(lib, _args(history=P, history_stride=stride), "history_stride=%d" % stride)
    for f in ("penalty", "history"):
        _rejects(lib, _args(**{f: P + 8}, history_stride=32000), "16-byte aligned")
    _rejects(lib, _args(bias=P + 4), "bias 8-byte")
    _rejects(lib, _args(row_tok=P + 4), "row_tok and bias 8-byte")
    _rejects(lib, _args(row_seq=P + 2), "row_seq 4-byte")
    hc = lib.mq_sample_history_count_ragged
    who = b"mq_sample_history_count_ragged"
    assert hc(None, 32000, 32000, 4, P, 4, 1, None) == 1 and who + b": history" in lib.mq_last_error()
    assert hc(P + 4, 32000, 32000, 4, P, 4, 1, None) == 1 and b"16-byte aligned" in lib.mq_last_error()
    assert hc(P, 32000, 31999, 4, P, 4, 1, None) == 1 and b"V=31999" in lib.mq_last_error()
    for stride in (31996, 32002):
        assert hc(P, stride, 32000, 4, P, 4, 1, None) == 1 and f"history_stride={stride}".encode() in lib.mq_last_error()
    for b in (0, 9):
        assert hc(P, 32000, 32000, b, P, 4, 1, None) == 1 and f"batch={b}".encode() in lib.mq_last_error()
    assert hc(P, 32000, 32000, 4, P, -1, 1, None) == 1 and b"n=-1" in lib.mq_last_error()
    assert hc(P, 32000, 32000, 4, None, 4, 1, None) == 1 and b"pairs must be" in lib.mq_last_error()
    assert hc(P, 32000, 32000, 4, P + 4, 4, 1, None) == 1 and b"pairs must be" in lib.mq_last_error()
    for bad in (0, 2, -2):
        assert hc(P, 32000, 32000, 4, P, 4, bad, None) == 1 and f"delta={bad}".encode() in lib.mq_last_error() and who in lib.mq_last_error()
    assert hc(P, 32000, 32000, 4, None, 0, -1, None) == 0                                   # nothing to count: no launch


def test_the_ragged_kernels_keep_no_scratch_memory_and_no_static_lds(tmp_path):
    """The ragged instantiations hold their run and their proposals in registers: no private segment, nothing new in LDS."""
    from mobilequant_amd import build
    flags = [f for f in build.FLAGS if f != "-fPIC"]
    asm = str(tmp_path / "mq_sample.s")
    cmd = [build.HIPCC, *flags, "-w", "--cuda-device-only", "-S", os.path.join(ROOT, "mobilequant_amd", "csrc", "mq_sample.hip"), "-o", asm]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    text = open(asm).read()
    for k in (r"sample_scan_kernelINS\S*6Ragged", r"sample_select_kernelINS\S*6Ragged", "history_count_ragged_kernel"):
        m = re.search(r"\.amdhsa_kernel \S*" + k + r"\S*\n(.*?)\.end_amdhsa_kernel", text, flags=re.S)
        assert m, k
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", m.group(1)), k
    m = re.search(r"\.amdhsa_kernel \S*sample_select_kernelINS\S*6Ragged\S*\n(.*?)\.end_amdhsa_kernel", text, flags=re.S)
    assert re.search(r"\.amdhsa_group_segment_fixed_size 0\b", m.group(1))


# ---- the Python surface ---------------------------------------------------------------------------------------------------------------
def test_sample_ragged_and_history_count_ragged_refuse_before_touching_a_device():
    from mobilequant_amd import ops, sampling
    assert ops.sample_ragged is sampling.sample_ragged and ops.sample_history_count_ragged is sampling.history_count_ragged
    lg = torch.zeros(4, 160)
    seq, pos = torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    rt, tok = torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.int64)
    req = ([SP, SP], [0, 1])
    with pytest.raises(RuntimeError, match="ROCm device tensor"):
        ops.sample_ragged(lg, seq, pos, rt, 1, req, tok)
    with pytest.raises(RuntimeError, match="fp32"):
        ops.sample_ragged(lg.double(), seq, pos, rt, 1, req, tok)
    for rows in (0, 9):
        with pytest.raises(RuntimeError, match="rows=%d outside 1..8" % rows):
            ops.sample_ragged(torch.zeros(rows, 160), seq, pos, rt, 1, req, tok)
    with pytest.raises(RuntimeError, match="batch=9 outside 1..8"):
        ops.sample_ragged(lg, seq, pos, rt, 1, ([SP] * 9, list(range(9))), tok)
    with pytest.raises(RuntimeError, match="batch=0 outside 1..8"):
        ops.sample_ragged(lg, seq, pos, rt, 1, ([], []), tok)
    with pytest.raises(TypeError, match="SamplingParams"):
        ops.sample_ragged(lg, seq, pos, rt, 1, ([(0.8, 0, 1.0, 0.0)], [0]), tok)
    with pytest.raises(ValueError, match="streams"):
        ops.sample_ragged(lg, seq, pos, rt, 1, ([SP, SP], [0]), tok)
    with pytest.raises(ValueError, match="stream"):
        ops.sample_ragged(lg, seq, pos, rt, 1, ([SP], [-1]), tok)
    for bad in (1.5, True, 2 ** 30 + 1):
        with pytest.raises(ValueError, match="n_offset"):
            ops.sample_ragged(lg, seq, pos, rt, bad, req, tok)
    h = torch.zeros(3, 160, dtype=torch.int32)
    pairs = torch.zeros(5, 2, dtype=torch.int64)
    for delta in (0, 2, -2, True, 1.5):
        with pytest.raises(ValueError, match="delta"):
            ops.sample_history_count_ragged(h, pairs, delta)
    with pytest.raises(RuntimeError, match="ROCm device tensor"):
        ops.sample_history_count_ragged(h, pairs, 1)
    with pytest.raises(RuntimeError, match="int32"):
        ops.sample_history_count_ragged(h.long(), pairs, 1)
    with pytest.raises(RuntimeError, match="int32"):
        ops.sample_history_count_ragged(h[0], pairs, -1)
    with pytest.raises(RuntimeError, match="int32"):
        ops.sample_history_count_ragged(torch.zeros(9, 160, dtype=torch.int32), pairs, 1)


# ---- the stand-in ---------------------------------------------------------------------------------------------------------------------
class ToyBatchEngine(BatchDecodeEngine):
    """What the batch generation loops touch of an engine, on CPU tensors; slot b's cache is the list prefix[b].  release() keeps what
    the slot held in `final` (the loops release every slot they finish)."""

    def __init__(self, batch: int = 8, cache_len: int = 64, max_rows: int = 8, loop: bool = False):
        self.batch, self.cache_len, self.max_rows, self.loop = batch, cache_len, max_rows, loop
        self.shape, self.dev = types.SimpleNamespace(vocab=V), torch.device("cpu")
        self.logits, self.tok = torch.zeros(batch, V), torch.zeros(batch, dtype=torch.int64)
        self.rlogits, self.rsel = torch.zeros(max_rows, V), torch.zeros(max_rows, dtype=torch.int64)
        self._host_pos, self._active, self.prefix = [cache_len] * batch, [False] * batch, [[] for _ in range(batch)]
        self._sampler, self.streams, self.spec_stats, self.final = None, list(range(batch)), None, {}
        self.row_steps = self.plain_steps = 0

    def _push(self, slot: int, token: int) -> torch.Tensor:
        assert self._active[slot] and len(self.prefix[slot]) == self._host_pos[slot] < self.cache_len
        self.prefix[slot].append(int(token))
        self._host_pos[slot] += 1
        return model_row(0, 0.0, self.loop, self.prefix[slot])

    def set_sampling(self, sampling, streams=None):
        rows = [sampling] * self.batch if isinstance(sampling, SamplingParams) else list(sampling)
        assert len(rows) == self.batch and all(isinstance(r, SamplingParams) for r in rows)
        self.streams = list(range(self.batch)) if streams is None else list(streams)
        self._sampler = types.SimpleNamespace(penalized=False)
        return self

    def release(self, slot):
        if self._active[slot]:
            self.final[slot] = (list(self.prefix[slot]), self._host_pos[slot])
        self._active[slot], self._host_pos[slot], self.prefix[slot] = False, self.cache_len, []

    def start(self, slot):
        self._active[slot], self._host_pos[slot], self.prefix[slot] = True, 0, []

    def prefill(self, slot, ids, append=False):
        self.start(slot)
        for t in ids:
            self.logits[slot].copy_(self._push(slot, t))
        return self.logits[slot]

    def step(self, tokens=None):
        if tokens is not None:
            self.tok.copy_(torch.tensor([int(v) for v in tokens], dtype=torch.int64))
        self.plain_steps += 1
        for b in range(self.batch):
            if self._active[b]:
                if self._host_pos[b] >= self.cache_len:
                    raise RuntimeError("ToyBatchEngine.step: a full cache")
                self.logits[b].copy_(self._push(b, int(self.tok[b])))
        return self.logits

    def step_tokens(self, tokens):
        total = sum(len(t) for t in tokens.values())
        if not 1 <= total <= self.max_rows:
            raise ValueError(f"ToyBatchEngine.step_tokens: {total} rows outside 1..{self.max_rows}")
        self.row_steps += 1
        out, r = {}, 0
        for slot in sorted(tokens):
            assert self._active[slot] and len(tokens[slot]) > 0 and self._host_pos[slot] + len(tokens[slot]) <= self.cache_len
            r0 = r
            for t in tokens[slot]:
                self.rlogits[r].copy_(self._push(slot, t))
                r += 1
            self.logits[slot].copy_(self.rlogits[r - 1])
            out[slot] = self.rlogits[r0:r]
        return out

    def rewind(self, slot, n):
        assert self._active[slot] and 0 <= int(n) <= self._host_pos[slot]
        del self.prefix[slot][int(n):]
        self._host_pos[slot] = int(n)
        return self

    def _draw(self, row, slot, index, out):
        if index < self.cache_len:                                 # (an idle row keeps its token)
            out.fill_(int(torch.argmax(row + NOISE[self.streams[slot]][index])))

    def sample(self):
        assert self._sampler is not None
        for b in range(self.batch):
            if self._active[b]:
                self._draw(self.logits[b], b, self._host_pos[b], self.tok[b:b + 1])
        return self.tok

    def sample_step(self):
        self.sample()
        return self.step()

    def step_sample_tokens(self, tokens):
        before = {slot: self._host_pos[slot] for slot in tokens}
        views = self.step_tokens(tokens)
        r = 0
        for slot in sorted(tokens):
            for j in range(views[slot].shape[0]):                  # the row cached at position p predicts index p + 1
                self._draw(views[slot][j], slot, before[slot] + j + 1, self.rsel[r:r + 1])
                r += 1
        return self.rsel[:r]


def plain_ids(prompt, new, stream=None, eos=(), loop=False):
    """The plain per-prompt loop: greedy (stream None) or argmax(row + NOISE[stream][index])."""
    out = list(prompt)
    for _ in range(new):
        row = model_row(0, 0.0, loop, out)
        out.append(int(torch.argmax(row if stream is None else row + NOISE[stream][len(out)])))
        if out[-1] in eos:
            break
    return out


def _prompts(n, loop=False):
    if loop:
        return [([1, 2, 3, 4] * 6)[i:i + 9 + 2 * i] for i in range(n)]
    lens = [5, 1, 12, 3, 9, 2, 7, 4][:n]
    return [[(3 * i + 7 * j) % V for j in range(ln)] for i, ln in enumerate(lens)]


def _draft(kind, truth):
    right = lambda ids, k: truth[len(ids):len(ids) + k]      # noqa: E731
    return {"oracle": right, "wrong": lambda ids, k: [(t + 1) % V for t in right(ids, k)],
            "two_then_wrong": lambda ids, k: [t if j < 2 else (t + 1) % V for j, t in enumerate(right(ids, k))],
            "empty": lambda ids, k: [], "lookup": prompt_lookup_draft(3)}[kind]


def _check_caches(eng, outs):
    assert not any(eng._active)
    for i, out in enumerate(outs):
        prefix, pos = eng.final[i]
        assert prefix == out[:pos] and pos == len(prefix) == len(out) - 1, (i, prefix, out)      # all but the last token is cached


KINDS = ["oracle", "wrong", "two_then_wrong", "empty", "lookup", "mixed"]


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [1, 3, 8])
def test_batch_speculative_ids_are_the_plain_ids(n, kind, sampled):
    loop = kind == "lookup"
    prompts = _prompts(n, loop)
    streams = STREAMS[:n]
    far = [plain_ids(p, 30, s if sampled else None, loop=loop) for p, s in zip(prompts, streams)]
    accepted = 0
    for max_rows, num_draft, new in ((8, 4, 11), (8, 7, 9), (8, 1, 2), (8, 0, 5), (3, 4, 9), (8, 4, 1), (8, 4, 0)):
        for eos_at in (None, 4):
            eos = None if eos_at is None or new < 6 else far[0][len(prompts[0]) + eos_at]      # inside an accepted run of prompt 0
            want = [plain_ids(p, new, s if sampled else None, () if eos is None else (eos,), loop) for p, s in zip(prompts, streams)]
            if kind == "mixed":
                drafts = [_draft(KINDS[i % 4], far[i]) for i in range(n)]
            else:
                drafts = [_draft(kind, far[i]) for i in range(n)] if kind != "lookup" else _draft(kind, None)
            eng = ToyBatchEngine(max_rows=max_rows, loop=loop)
            if sampled:
                got = eng.generate_speculative(prompts, new, drafts, sampling=[SP] * n, streams=streams, num_draft=num_draft, eos_token_id=eos)
            else:
                got = eng.generate(prompts, new, eos_token_id=eos, draft=drafts, num_draft=num_draft)
            assert got == want, (max_rows, num_draft, new, eos)
            if new == 0:
                continue
            _check_caches(eng, got)
            st = eng.spec_stats
            assert set(st) == {"rounds", "proposed", "accepted", "target_steps"}
            short = 1 if any(len(p) == 1 for p in prompts) else 0      # (the one-token prompts' own step)
            assert st["rounds"] == st["target_steps"] == eng.row_steps + eng.plain_steps - short
            assert 0 <= st["accepted"] <= st["proposed"] <= eng.row_steps * max_rows
            accepted += st["accepted"]
            if n > max_rows and new > 1:
                assert eng.plain_steps - short >= 1                # more live slots than rows: plain steps
            if new <= 1:
                assert st["rounds"] == 0
            if kind in ("wrong", "empty"):
                assert st["accepted"] == 0
            if kind == "oracle" and eos is None:
                assert st["accepted"] == st["proposed"]
                if n == 1:
                    kk = min(num_draft, max_rows - 1)
                    assert st["rounds"] == math.ceil((new - 1) / (kk + 1))
            if kind == "two_then_wrong" and n == 1 and eos is None and num_draft >= 4 and max_rows == 8:
                assert st["accepted"] == 2 * st["rounds"] or new - 1 < 3 * st["rounds"]      # two per round until the budget cuts
    if kind not in ("wrong", "empty") and n < 8:
        assert accepted > 0                                        # (the case is not vacuous)


def test_the_batched_plain_loop_of_the_stand_in_is_the_per_prompt_loop_and_streams_matter():
    prompts, streams = _prompts(3), STREAMS[:3]
    eng = ToyBatchEngine()
    want = [plain_ids(p, 9, s) for p, s in zip(prompts, streams)]
    assert eng.generate(prompts, 9, sampling=SP, streams=streams) == want
    assert want[0] != plain_ids(prompts[0], 9, streams[1]) and want[0] != plain_ids(prompts[0], 9)
    # a sequence's ids do not depend on its slot or on its neighbours
    d = lambda ids, k: []      # noqa: E731
    assert eng.generate_speculative(prompts[::-1], 9, d, sampling=SP, streams=streams[::-1]) == want[::-1]
    assert eng.generate_speculative(prompts[1:2], 9, d, sampling=SP, streams=streams[1:2]) == want[1:2]


def test_generate_speculative_refuses_bad_requests_before_the_engine_moves():
    eng = ToyBatchEngine(batch=2)
    eng.prefill(0, [7, 8])
    d = lambda ids, k: []      # noqa: E731
    gs = eng.generate_speculative
    with pytest.raises(TypeError):
        gs([[1, 2]], 4, d)                                                                  # sampling is required
    for bad in (None, 0.8, {"temperature": 0.8}, [SP, 0.8]):
        with pytest.raises(TypeError, match="SamplingParams"):
            gs([[1, 2], [3]], 4, d, sampling=bad)
    with pytest.raises(TypeError, match="callable drafts"):
        gs([[1, 2]], 4, object.__new__(BatchDecodeEngine), sampling=SP)
    with pytest.raises(TypeError, match="callable drafts"):
        gs([[1, 2], [3]], 4, [d, eng], sampling=SP)
    for bad in (5, None, "lookup"):
        with pytest.raises(TypeError, match="callable"):
            gs([[1, 2]], 4, bad, sampling=SP)
    with pytest.raises(ValueError, match="1 drafts for 2 prompts"):
        gs([[1, 2], [3]], 4, [d], sampling=SP)
    with pytest.raises(ValueError, match="1 SamplingParams / 2 streams for 2 prompts"):
        gs([[1, 2], [3]], 4, d, sampling=[SP])
    with pytest.raises(ValueError, match="2 SamplingParams / 1 streams for 2 prompts"):
        gs([[1, 2], [3]], 4, d, sampling=SP, streams=[4])
    with pytest.raises(ValueError, match="stream"):
        gs([[1, 2]], 4, d, sampling=SP, streams=[-1])
    for bad in (-1, True):
        with pytest.raises(ValueError, match="num_draft"):
            gs([[1, 2]], 4, d, sampling=SP, num_draft=bad)
    for bad in ([], [[1]] * 3):
        with pytest.raises(ValueError, match="prompts for 2 slots"):
            gs(bad, 4, d, sampling=SP)
    with pytest.raises(ValueError, match="exceeds the cache"):
        gs([[1, 2]], 63, d, sampling=SP)
    assert eng.prefix[0] == [7, 8] and eng._sampler is None and eng.spec_stats is None
    # generate(sampling=..., draft=...) refuses as before: generate_speculative is the entry point
    with pytest.raises(ValueError, match="greedy"):
        eng.generate([[1, 2]], 4, sampling=SP, draft=d)
    assert eng.prefix[0] == [7, 8]
