"""Penalties and logit bias in front of the seeded selection (step 0 of the rule) without a GPU: the numpy reference of
the transform against hand-computed cases, mq_sample_penalized's ABI (declared, bound, struct layouts, every refusal before any HIP
call), SamplingParams' new fields, the engines' unchanged ValueErrors and the barrier audit of the new instantiations.  Pointers are
fake and never read."""
import ctypes
import dataclasses
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sampling_penalty_ref as PR  # noqa: E402
import sampling_ref as R  # noqa: E402

P = 0x10000
F = np.float32


@pytest.fixture(scope="module")
def lib():
    from mobilequant_amd import _lib, build
    build.build()
    return _lib.load()


# ---- the reference transform against hand-computed cases ----------------------------------------------------------------------------
def test_reference_repetition_penalty_on_a_positive_a_negative_and_an_unseen_logit():
    l = np.array([2.0, -2.0, 2.0, -2.0, 0.0, 3.0, -0.0, 1.5], dtype=F)
    h = np.array([1 << 31, 1 << 31, 0, 0, 1, (1 << 31) | 2, 5, 0], dtype=np.uint32)      # prompt, prompt, unseen, unseen, generated, both, generated
    got = PR.transform(l, h, repetition=1.25)
    want = np.array([1.6, -2.5, 2.0, -2.0, 0.0, 2.4, -0.0, 1.5], dtype=F)                 # 2 / 1.25, -2 * 1.25, untouched, ..., 0 * 1.25, 3 / 1.25
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got, np.array([F(2.0) / F(1.25), F(-2.0) * F(1.25), 2.0, -2.0, 0.0, F(3.0) / F(1.25), -0.0, 1.5], dtype=F))
    # a repetition penalty that is not finite and positive counts as 1
    for bad in (0.0, -1.0, np.inf, np.nan):
        assert np.array_equal(PR.transform(l, h, repetition=bad).view(np.uint32), l.view(np.uint32))


def test_reference_presence_and_frequency_count_generated_tokens_only():
    l = np.array([1.0, 1.0, 1.0, -1.0], dtype=F)
    h = np.array([3, 1 << 31, 0, (1 << 31) | 3], dtype=np.uint32)                          # c = 3; prompt only; unseen; prompt and c = 3
    got = PR.transform(l, h, presence=0.5, frequency=0.25)
    # c = 3: t = 0.25 * 3 = 0.75, + 0.5 = 1.25 -> 1 - 1.25 = -0.25 and -1 - 1.25 = -2.25; c = 0: t = 0 -> untouched
    assert got.tolist() == [-0.25, 1.0, 1.0, -2.25]
    both = PR.transform(l, h, repetition=2.0, presence=0.5, frequency=0.25)
    assert both.tolist() == [0.5 - 1.25, 0.5, 1.0, -2.0 - 1.25]                            # the repetition penalty first, and on prompt tokens too
    # the count saturates: 65 535 stays 65 535
    hs = np.array([0xFFFF, 0xFFFE], dtype=np.uint32)
    PR.observe(hs, 0)
    PR.observe(hs, 1)
    assert hs.tolist() == [0xFFFF, 0xFFFF]
    assert PR.transform(np.zeros(2, dtype=F), hs, frequency=1.0).tolist() == [-65535.0, -65535.0]


def test_reference_bias_bans_a_token_and_the_neutral_request_keeps_the_bits():
    l = np.array([4.0, 1.0, np.inf, 0.5], dtype=F)
    h = np.zeros(4, dtype=np.uint32)
    b = PR.dense_bias(4, {0: -np.inf, 1: 2.5, 2: -np.inf})
    got = PR.transform(l, h, bias=b)
    assert got[0] == -np.inf and got[1] == 3.5 and np.isnan(got[2]) and got[3] == 0.5      # inf - inf is a NaN: -inf to the rule
    assert R.analyse(got, 0.0, 0, 1.0, 0.0, 0, 0, 0)["token"] == 1                         # the banned maximum is gone
    assert R.analyse(l, 0.0, 0, 1.0, 0.0, 0, 0, 0)["token"] == 2
    odd = np.array([-0.0, np.nan, -np.inf, 1e-42], dtype=F)
    keep = PR.transform(odd, np.array([7, 1 << 31, 0, 3], dtype=np.uint32))
    assert np.array_equal(keep.view(np.uint32), odd.view(np.uint32))
    # history helpers
    hp = PR.prompt_history(8, [1, 5, 5, 1])
    assert hp.tolist() == [0, 1 << 31, 0, 0, 0, 1 << 31, 0, 0]
    PR.observe(hp, 5)
    assert hp[5] == (1 << 31) | 1


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------
def _args(**kw):
    from mobilequant_amd._lib import MQ_SAMPLE_SCRATCH_BYTES, MqSamplePenalizedArgs
    a = MqSamplePenalizedArgs()
    s = a.s
    s.logits, s.pos, s.params, s.tok, s.scratch = P, P, P, P, P
    s.logits_stride, s.V, s.rows, s.cache_len, s.scratch_bytes = 32000, 32000, 2, 256, MQ_SAMPLE_SCRATCH_BYTES
    a.penalty, a.history, a.history_stride, a.bias, a.observe = P, P, 32000, None, 1
    for k, v in kw.items():
        setattr(s if hasattr(s, k) else a, k, v)
    return a


def _rejects(lib, a, text):
    rc = lib.mq_sample_penalized(ctypes.byref(a), None)
    msg = lib.mq_last_error()
    assert rc == 1 and text.encode() in msg and b"mq_sample_penalized" in msg, (rc, msg)


def test_entries_are_declared_exported_and_the_structs_match_the_header(lib):
    from mobilequant_amd import _lib
    from mobilequant_amd._lib import MqSampleArgs, MqSamplePenalizedArgs, MqSamplePenaltyRow
    from mobilequant_amd.sampling import PENALTY_DTYPE
    for name in ("mq_sample_penalized", "mq_sample_history_prompt"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    hdr = open(os.path.join(ROOT, "include", "mobilequant_amd.h")).read()
    assert re.search(r"int mq_sample_penalized\(const mq_sample_penalized_args\* args, mq_stream_t stream\);", hdr)
    assert re.search(r"int mq_sample_history_prompt\(uint32_t\* history, int64_t V, const int64_t\* ids, int64_t n, int clear, mq_stream_t stream\);", hdr)
    rf = ("repetition", "presence", "frequency", "reserved")
    af = ("s", "penalty", "history", "history_stride", "bias", "observe")
    src = "\n".join(["#include <stddef.h>", "#include <stdio.h>", '#include "mobilequant_amd.h"', "int main(void) {",
                     '  printf("%zu' + " %zu" * len(rf) + '\\n", sizeof(mq_sample_penalty_row), ' + ", ".join(f"offsetof(mq_sample_penalty_row, {f})" for f in rf) + ");",
                     '  printf("%zu' + " %zu" * len(af) + '\\n", sizeof(mq_sample_penalized_args), ' + ", ".join(f"offsetof(mq_sample_penalized_args, {f})" for f in af) + ");",
                     '  printf("%zu\\n", sizeof(mq_sample_args));', "  return 0;", "}"])
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        open(c, "w").write(src)
        cc = next((x for x in ("cc", "gcc", "clang") if subprocess.run(["which", x], stdout=subprocess.PIPE).returncode == 0), None)
        if cc is None:
            cc = "/opt/rocm/llvm/bin/clang"
        subprocess.run([cc, "-I" + os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        out = subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")
    assert [int(v) for v in out[0].split()] == [ctypes.sizeof(MqSamplePenaltyRow)] + [getattr(MqSamplePenaltyRow, f).offset for f in rf]
    assert [int(v) for v in out[1].split()] == [ctypes.sizeof(MqSamplePenalizedArgs)] + [getattr(MqSamplePenalizedArgs, f).offset for f in af]
    assert int(out[2]) == ctypes.sizeof(MqSampleArgs) and MqSamplePenalizedArgs.s.offset == 0       # mq_sample_args embedded unchanged, in front
    assert ctypes.sizeof(MqSamplePenaltyRow) == 16 == PENALTY_DTYPE.itemsize
    assert [PENALTY_DTYPE.fields[f][1] for f in rf] == [getattr(MqSamplePenaltyRow, f).offset for f in rf]


def test_rejects_argument_blocks_outside_the_limits(lib):
    assert lib.mq_sample_penalized(None, None) == 1 and b"null argument block" in lib.mq_last_error()
    # everything mq_sample checks
    for f in ("logits", "pos", "params", "tok", "scratch"):
        _rejects(lib, _args(**{f: None}), "null pointer")
    for r in (0, 9, -1):
        _rejects(lib, _args(rows=r), "outside 1..8")
    _rejects(lib, _args(V=31999, logits_stride=32000), "V=31999")
    _rejects(lib, _args(V=(1 << 20) + 4, logits_stride=(1 << 20) + 4, history_stride=(1 << 20) + 4), "multiple of 4 in [4, 2^20]")
    _rejects(lib, _args(V=0), "V=0")
    _rejects(lib, _args(logits_stride=31996), "logits_stride=31996")
    _rejects(lib, _args(logits_stride=32002), "logits_stride=32002")
    _rejects(lib, _args(cache_len=0), "cache_len=0")
    _rejects(lib, _args(logits=P + 8), "16-byte aligned")
    _rejects(lib, _args(params=P + 8), "16-byte aligned")
    _rejects(lib, _args(tok=P + 4), "8-byte")
    _rejects(lib, _args(kept=P + 2), "4-byte aligned")
    _rejects(lib, _args(scratch_bytes=4096), "scratch_bytes=4096")
    # and its own
    _rejects(lib, _args(history=None), "null pointer (penalty and history")
    _rejects(lib, _args(penalty=None), "null pointer (penalty and history")
    _rejects(lib, _args(history=P + 8), "16-byte aligned")
    _rejects(lib, _args(history=P + 4), "16-byte aligned")
    _rejects(lib, _args(history_stride=31996), "history_stride=31996")
    _rejects(lib, _args(history_stride=0), "history_stride=0")
    _rejects(lib, _args(history_stride=32002), "history_stride=32002")
    _rejects(lib, _args(observe=2), "observe=2")
    hp = lib.mq_sample_history_prompt
    assert hp(None, 32000, P, 4, 1, None) == 1 and b"mq_sample_history_prompt: history" in lib.mq_last_error()
    assert hp(P + 4, 32000, P, 4, 1, None) == 1 and b"16-byte aligned" in lib.mq_last_error()
    assert hp(P, 31999, P, 4, 1, None) == 1 and b"V=31999" in lib.mq_last_error()
    assert hp(P, 0, P, 4, 1, None) == 1 and b"V=0" in lib.mq_last_error()
    assert hp(P, 32000, P, -1, 1, None) == 1 and b"n=-1" in lib.mq_last_error()
    assert hp(P, 32000, None, 4, 1, None) == 1 and b"ids must be" in lib.mq_last_error()
    assert hp(P, 32000, P, 4, 2, None) == 1 and b"clear=2" in lib.mq_last_error()


def test_no_barrier_with_lds_traffic_in_flight_in_the_penalised_instantiations(tmp_path):
    """tools/barrier_audit.py on mq_sample.hip with the penalised instantiations in it, next to the plain ones."""
    from mobilequant_amd import build
    flags = [f for f in build.FLAGS if f != "-fPIC"]
    src = "mq_sample.hip"
    asm = str(tmp_path / "mq_sample.s")
    cmd = [build.HIPCC, *flags, *build.PER_FILE_FLAGS.get(src, ()), "-w", "--cuda-device-only", "-S", os.path.join(ROOT, "mobilequant_amd", "csrc", src), "-o", asm]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    rep = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "barrier_audit.py"), asm], stdout=subprocess.PIPE, text=True).stdout
    assert "PENDING" not in rep and "possibly in flight 0" in rep, rep
    text = open(asm).read()
    for k in (r"sample_scan_kernelINS\S*9NoPenalty", r"sample_select_kernelINS\S*9NoPenalty", r"sample_scan_kernelINS\S*7Penalty",
              r"sample_select_kernelINS\S*7Penalty"):
        assert re.search(k, text), k
    # the penalised select kernel keeps no scratch memory and no static LDS of its own (the history is read from memory, never staged)
    m = re.search(r"\.amdhsa_kernel \S*sample_select_kernelINS\S*7Penalty\S*\n(.*?)\.end_amdhsa_kernel", text, flags=re.S)
    assert m and re.search(r"\.amdhsa_group_segment_fixed_size 0\b", m.group(1)) and re.search(r"\.amdhsa_private_segment_fixed_size 0\b", m.group(1))


# ---- the Python surface ----------------------------------------------------------------------------------------------------------------
def test_sampling_params_new_fields_validate_hash_and_default():
    from mobilequant_amd import SamplingParams
    sp = SamplingParams()
    assert (sp.repetition_penalty, sp.presence_penalty, sp.frequency_penalty, sp.logit_bias) == (1.0, 0.0, 0.0, None)
    assert not sp.penalized and not SamplingParams(temperature=0.7, top_k=40, top_p=0.9, min_p=0.1, seed=5).penalized
    assert SamplingParams(0.7, 40, 0.9, 0.05, 3) == SamplingParams(temperature=0.7, top_k=40, top_p=0.9, min_p=0.05, seed=3)      # positions unchanged
    for kw in (dict(repetition_penalty=1.3), dict(repetition_penalty=0.5), dict(presence_penalty=0.1), dict(presence_penalty=-0.1),
               dict(frequency_penalty=2), dict(logit_bias={3: 0.0}), dict(logit_bias={3: float("-inf")})):
        assert SamplingParams(**kw).penalized, kw
    a = SamplingParams(logit_bias={7: 1.5, 2: float("-inf")}, repetition_penalty=1.2)
    assert a.logit_bias == ((2, float("-inf")), (7, 1.5))                                # a sorted tuple of pairs
    b = SamplingParams(logit_bias=[(7, 1.5), (2, float("-inf"))], repetition_penalty=1.2)
    assert a == b and hash(a) == hash(b) and len({a, b, sp}) == 2
    assert dataclasses.replace(a, seed=4).logit_bias == a.logit_bias
    assert SamplingParams(logit_bias={}).logit_bias is None and not SamplingParams(logit_bias={}).penalized
    with pytest.raises(dataclasses.FrozenInstanceError):
        a.repetition_penalty = 1.0
    for bad in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=float("inf")), dict(repetition_penalty=float("nan")),
                dict(repetition_penalty="1.1"), dict(repetition_penalty=True), dict(repetition_penalty=1e-60), dict(repetition_penalty=1e60),
                dict(presence_penalty=float("nan")), dict(presence_penalty=float("inf")), dict(presence_penalty="0"), dict(presence_penalty=1e60),
                dict(frequency_penalty=float("-inf")), dict(frequency_penalty=None), dict(frequency_penalty=False),
                dict(logit_bias={-1: 0.5}), dict(logit_bias={1.5: 0.5}), dict(logit_bias={True: 0.5}), dict(logit_bias={1: float("nan")}),
                dict(logit_bias={1: float("inf")}), dict(logit_bias={1: "x"}), dict(logit_bias=5), dict(logit_bias=[(1, 0.5), (1, 0.25)])):
        with pytest.raises(ValueError):
            SamplingParams(**bad)


def test_pack_penalty_rows_lays_out_mq_sample_penalty_row():
    from mobilequant_amd import SamplingParams
    from mobilequant_amd._lib import MqSamplePenaltyRow
    from mobilequant_amd.sampling import pack_penalty_rows
    raw = pack_penalty_rows([SamplingParams(repetition_penalty=1.3, presence_penalty=-0.5, frequency_penalty=0.25), SamplingParams(), (2.0, 0.0, 1.0)]).tobytes()
    r0, r1, r2 = (MqSamplePenaltyRow.from_buffer_copy(raw[16 * i:16 * i + 16]) for i in range(3))
    assert (F(r0.repetition), F(r0.presence), F(r0.frequency), r0.reserved) == (F(1.3), F(-0.5), F(0.25), 0)
    assert (r1.repetition, r1.presence, r1.frequency) == (1.0, 0.0, 0.0) and (r2.repetition, r2.frequency) == (2.0, 1.0)


def test_engines_still_refuse_a_draft_or_do_sample_with_a_penalised_request():
    """The checks run in front of everything else in generate: a bare object stands in for an engine."""
    from mobilequant_amd import SamplingParams
    from mobilequant_amd.decode import DecodeEngine
    from mobilequant_amd.decode_batch import BatchDecodeEngine
    sp = SamplingParams(temperature=0.0, repetition_penalty=1.3, logit_bias={1: -1.0})
    eng = object.__new__(DecodeEngine)
    with pytest.raises(ValueError, match="do_sample"):
        DecodeEngine.generate(eng, [1, 2], 4, do_sample=True, sampling=sp)
    with pytest.raises(ValueError, match="draft"):
        DecodeEngine.generate(eng, [1, 2], 4, sampling=sp, draft=lambda ids, k: [])
    be = object.__new__(BatchDecodeEngine)
    be.batch, be.cache_len = 2, 64
    with pytest.raises(ValueError, match="do_sample"):
        BatchDecodeEngine.generate(be, [[1], [2]], 4, do_sample=True, sampling=[sp, SamplingParams()])
    with pytest.raises(ValueError, match="exceeds the cache"):
        BatchDecodeEngine.generate(be, [[1] * 61, [2]], 4, sampling=[sp, SamplingParams()])
