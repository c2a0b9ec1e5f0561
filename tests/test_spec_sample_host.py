"""Speculative decoding under seeded sampling (mq_sample_rows, mq_sample_history_count) without a GPU: the ABI
(declared, bound, struct layout, every refusal before any HIP call), the refusals of the Python surface on CPU tensors and on a bare
engine object, and the host restatement of the in-flight history that tests/test_gpu_spec_sample.py checks the kernels against.
Pointers are fake and never read."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sampling_penalty_ref as PR  # noqa: E402
import sampling_ref as R  # noqa: E402

P = 0x10000
F = np.float32


# ---- the rule's extension, restated on the host ------------------------------------------------------------------------------------
def inflight_history(history, proposals, j):
    """Row j's history of a multi-row launch: a copy of the sequence's history (uint32 [V]) on which proposals[0 .. j-1] were counted
    one after the other (sampling_penalty_ref.observe: + 1, saturating at 65 535, bit 31 untouched); a proposal outside [0, V) counts
    nowhere."""
    h = np.array(history, dtype=np.uint32, copy=True)
    for d in list(proposals)[:j]:
        if 0 <= int(d) < len(h):
            PR.observe(h, int(d))
    return h


def count_history(history, ids, delta):
    """mq_sample_history_count as a host loop, in place: one id after the other, saturating at 65 535 and at 0."""
    for t in ids:
        t = int(t)
        if not 0 <= t < len(history):
            continue
        c = int(history[t]) & 0xFFFF
        if delta > 0 and c != 0xFFFF:
            history[t] += np.uint32(1)
        elif delta < 0 and c != 0:
            history[t] -= np.uint32(1)
    return history


def rows_reference(logits, history, proposals, n0, sp, stream):
    """sampling_ref.analyse of every row of one sequence: row j at index n0 + j, from step 0 over its in-flight history."""
    V = logits.shape[1]
    rows = []
    for j in range(logits.shape[0]):
        l = logits[j]
        if sp.penalized:
            h = inflight_history(history if history is not None else np.zeros(V, dtype=np.uint32), proposals, j)
            l = PR.transform(l, h, sp.repetition_penalty, sp.presence_penalty, sp.frequency_penalty, PR.dense_bias(V, sp.logit_bias))
        rows.append(R.analyse(l, sp.temperature, sp.top_k, sp.top_p, sp.min_p, sp.seed, stream, n0 + j))
    return rows


def test_inflight_history_counts_the_proposals_in_front_of_a_row_only():
    h = np.array([0, 1 << 31, 0xFFFE, (1 << 31) | 3, 0, 0, 0, 0], dtype=np.uint32)
    d = [2, 1, 2, 9, -1, 2, 4]
    assert inflight_history(h, d, 0).tolist() == h.tolist()
    assert inflight_history(h, d, 1).tolist() == [0, 1 << 31, 0xFFFF, (1 << 31) | 3, 0, 0, 0, 0]
    assert inflight_history(h, d, 3).tolist() == [0, (1 << 31) | 1, 0xFFFF, (1 << 31) | 3, 0, 0, 0, 0]      # saturated: the second 2 adds nothing
    assert inflight_history(h, d, 7).tolist() == [0, (1 << 31) | 1, 0xFFFF, (1 << 31) | 3, 1, 0, 0, 0]      # 9 and -1 match no entry
    assert h[2] == 0xFFFE                                                                                  # the sequence's history is not written
    back = count_history(inflight_history(h, d, 7), d, -1)
    assert back.tolist() == [0, 1 << 31, 0xFFFC, (1 << 31) | 3, 0, 0, 0, 0]                               # (- 1 is no inverse at the ceiling)
    assert count_history(np.array([0, 1 << 31], dtype=np.uint32), [0, 1, 1], -1).tolist() == [0, 1 << 31]      # floor at 0, bit 31 kept
    # a proposal decides a greedy draw only for the rows behind it
    from mobilequant_amd import SamplingParams
    sp = SamplingParams(temperature=0.0, presence_penalty=4.0)
    l = np.tile(np.array([0.0, 5.0, 4.0, 3.0, 2.0, 0.0, 0.0, 0.0], dtype=F), (4, 1))
    assert [a["token"] for a in rows_reference(l, None, [1, 2, 3], 10, sp, 0)] == [1, 2, 3, 4]
    assert [a["token"] for a in rows_reference(l, None, [7, 7, 7], 10, sp, 0)] == [1, 1, 1, 1]


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from mobilequant_amd import _lib, build
    build.build()
    return _lib.load()


def _args(**kw):
    from mobilequant_amd._lib import MQ_SAMPLE_SCRATCH_BYTES, MqSampleRowsArgs
    a = MqSampleRowsArgs()
    a.logits, a.n_base, a.params, a.tok, a.scratch, a.proposals = P, P, P, P, P, P
    a.logits_stride, a.V, a.rows, a.n_offset, a.scratch_bytes = 32000, 32000, 4, -3, MQ_SAMPLE_SCRATCH_BYTES
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _rejects(lib, a, text):
    rc = lib.mq_sample_rows(ctypes.byref(a), None)
    msg = lib.mq_last_error()
    assert rc == 1 and text.encode() in msg and b"mq_sample_rows" in msg, (rc, msg)


def test_entries_are_declared_exported_and_the_struct_matches_the_header(lib):
    from mobilequant_amd import _lib
    from mobilequant_amd._lib import MqSampleRowsArgs
    for name in ("mq_sample_rows", "mq_sample_history_count"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    hdr = open(os.path.join(ROOT, "include", "mobilequant_amd.h")).read()
    assert re.search(r"int mq_sample_rows\(const mq_sample_rows_args\* args, mq_stream_t stream\);", hdr)
    assert re.search(r"int mq_sample_history_count\(uint32_t\* history, int64_t V, const int64_t\* ids, int64_t n, int delta, mq_stream_t stream\);", hdr)
    ver = int(re.search(r"#define MQ_VERSION (\d+)", hdr).group(1))
    assert ver // 100 == _lib.HEADER_MAJOR == lib.mq_version() // 100                       # additive entries: the major stays
    af = [f for f, _ in MqSampleRowsArgs._fields_]
    assert af == ["logits", "logits_stride", "V", "rows", "n_base", "n_offset", "params", "penalty", "bias", "history", "proposals", "tok", "kept",
                  "logprob", "scratch", "scratch_bytes"]
    src = "\n".join(["#include <stddef.h>", "#include <stdio.h>", '#include "mobilequant_amd.h"', "int main(void) {",
                     '  printf("%zu' + " %zu" * len(af) + '\\n", sizeof(mq_sample_rows_args), ' + ", ".join(f"offsetof(mq_sample_rows_args, {f})" for f in af) + ");",
                     "  return 0;", "}"])
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        open(c, "w").write(src)
        cc = next((x for x in ("cc", "gcc", "clang") if subprocess.run(["which", x], stdout=subprocess.PIPE).returncode == 0), None)
        if cc is None:
            cc = "/opt/rocm/llvm/bin/clang"
        subprocess.run([cc, "-I" + os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        out = subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")
    assert [int(v) for v in out[0].split()] == [ctypes.sizeof(MqSampleRowsArgs)] + [getattr(MqSampleRowsArgs, f).offset for f in af]


def test_rejects_argument_blocks_outside_the_limits(lib):
    assert lib.mq_sample_rows(None, None) == 1 and b"null argument block" in lib.mq_last_error()
    for f in ("logits", "n_base", "params", "tok", "scratch"):
        _rejects(lib, _args(**{f: None}), "null pointer")
    for r in (0, 9, -1):
        _rejects(lib, _args(rows=r), "outside 1..8")
    _rejects(lib, _args(V=31999), "V=31999")
    _rejects(lib, _args(V=(1 << 20) + 4, logits_stride=(1 << 20) + 4), "multiple of 4 in [4, 2^20]")
    _rejects(lib, _args(V=0), "V=0")
    _rejects(lib, _args(logits_stride=31996), "logits_stride=31996")
    _rejects(lib, _args(logits_stride=32002), "logits_stride=32002")
    _rejects(lib, _args(logits=P + 8), "16-byte aligned")
    _rejects(lib, _args(params=P + 8), "16-byte aligned")
    _rejects(lib, _args(tok=P + 4), "8-byte")
    _rejects(lib, _args(kept=P + 2), "4-byte aligned")
    _rejects(lib, _args(scratch_bytes=4096), "scratch_bytes=4096")
    _rejects(lib, _args(n_offset=(1 << 30) + 1), "n_offset=")
    _rejects(lib, _args(proposals=None), "proposals holds rows - 1 ids")
    _rejects(lib, _args(proposals=P + 4), "proposals 8-byte aligned")
    for f in ("penalty", "history", "bias"):
        _rejects(lib, _args(**{f: P + 8}), "16-byte aligned")
    hc = lib.mq_sample_history_count
    assert hc(None, 32000, P, 4, 1, None) == 1 and b"mq_sample_history_count: history" in lib.mq_last_error()
    assert hc(P + 4, 32000, P, 4, 1, None) == 1 and b"16-byte aligned" in lib.mq_last_error()
    assert hc(P, 31999, P, 4, 1, None) == 1 and b"V=31999" in lib.mq_last_error()
    assert hc(P, 32000, P, -1, 1, None) == 1 and b"n=-1" in lib.mq_last_error()
    assert hc(P, 32000, None, 4, 1, None) == 1 and b"ids must be" in lib.mq_last_error()
    for bad in (0, 2, -2):
        assert hc(P, 32000, P, 4, bad, None) == 1 and f"delta={bad}".encode() in lib.mq_last_error()
    assert hc(P, 32000, None, 0, -1, None) == 0                                             # nothing to count: no launch


def test_the_new_kernels_keep_no_scratch_memory_and_no_static_lds(tmp_path):
    """The rows instantiation of the select kernel holds its proposals in registers: no private segment, nothing new in LDS."""
    from mobilequant_amd import build
    flags = [f for f in build.FLAGS if f != "-fPIC"]
    asm = str(tmp_path / "mq_sample.s")
    cmd = [build.HIPCC, *flags, "-w", "--cuda-device-only", "-S", os.path.join(ROOT, "mobilequant_amd", "csrc", "mq_sample.hip"), "-o", asm]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    rep = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "barrier_audit.py"), asm], stdout=subprocess.PIPE, text=True).stdout
    assert "PENDING" not in rep and "possibly in flight 0" in rep, rep
    text = open(asm).read()
    for k in (r"sample_scan_kernelINS\S*4Rows", r"sample_select_kernelINS\S*4Rows", "history_count_kernel"):
        m = re.search(r"\.amdhsa_kernel \S*" + k + r"\S*\n(.*?)\.end_amdhsa_kernel", text, flags=re.S)
        assert m, k
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", m.group(1)), k
    m = re.search(r"\.amdhsa_kernel \S*sample_select_kernelINS\S*4Rows\S*\n(.*?)\.end_amdhsa_kernel", text, flags=re.S)
    assert re.search(r"\.amdhsa_group_segment_fixed_size 0\b", m.group(1))


# ---- the Python surface ---------------------------------------------------------------------------------------------------------------
def test_sample_rows_and_history_count_refuse_before_touching_a_device():
    from mobilequant_amd import SamplingParams, ops, sampling
    assert ops.sample_rows is sampling.sample_rows and ops.sample_history_count is sampling.history_count
    sp = SamplingParams(temperature=0.8, seed=1)
    lg = torch.zeros(4, 160)
    nb, tok, prop = torch.zeros(1, dtype=torch.int32), torch.zeros(4, dtype=torch.int64), torch.zeros(3, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="ROCm device tensor"):
        sampling.sample_rows(lg, nb, 0, sp, 0, tok, proposals=prop)
    with pytest.raises(RuntimeError, match="fp32"):
        sampling.sample_rows(lg.double(), nb, 0, sp, 0, tok, proposals=prop)
    for rows in (0, 9):
        with pytest.raises(RuntimeError, match="outside 1..8"):
            sampling.sample_rows(torch.zeros(rows, 160), nb, 0, sp, 0, torch.zeros(rows, dtype=torch.int64))
    with pytest.raises(TypeError, match="SamplingParams"):
        sampling.sample_rows(lg, nb, 0, (0.8, 0, 1.0, 0.0), 0, tok, proposals=prop)
    with pytest.raises(ValueError, match="n_offset"):
        sampling.sample_rows(lg, nb, 1.5, sp, 0, tok, proposals=prop)
    with pytest.raises(ValueError, match="stream"):
        sampling.sample_rows(lg, nb, 0, sp, -1, tok, proposals=prop)
    h = torch.zeros(160, dtype=torch.int32)
    ids = torch.zeros(3, dtype=torch.int64)
    for delta in (0, 2, -2, True, 1.5):
        with pytest.raises(ValueError, match="delta"):
            sampling.history_count(h, ids, delta)
    with pytest.raises(RuntimeError, match="ROCm device tensor"):
        sampling.history_count(h, ids, 1)
    with pytest.raises(RuntimeError, match="int32"):
        sampling.history_count(h.long(), ids, 1)
    with pytest.raises(RuntimeError, match="int32"):
        sampling.history_count(h.view(2, 80), ids, -1)


def test_generate_speculative_refuses_bad_requests_on_a_bare_engine():
    """The checks run in front of everything else: a bare object stands in for an engine."""
    from mobilequant_amd import SamplingParams
    from mobilequant_amd.decode import DecodeEngine
    eng = object.__new__(DecodeEngine)
    sp = SamplingParams(temperature=0.8, seed=3)
    draft = lambda ids, k: []      # noqa: E731
    with pytest.raises(TypeError):
        DecodeEngine.generate_speculative(eng, [1, 2], 4, draft)                           # sampling is required
    for bad in (None, 0.8, {"temperature": 0.8}):
        with pytest.raises(TypeError, match="SamplingParams"):
            DecodeEngine.generate_speculative(eng, [1, 2], 4, draft, sampling=bad)
    with pytest.raises(ValueError, match="another engine"):
        DecodeEngine.generate_speculative(eng, [1, 2], 4, eng, sampling=sp)
    for bad in (5, None, "lookup"):
        with pytest.raises(TypeError, match="callable"):
            DecodeEngine.generate_speculative(eng, [1, 2], 4, bad, sampling=sp)
    with pytest.raises(ValueError, match="num_draft"):
        DecodeEngine.generate_speculative(eng, [1, 2], 4, draft, sampling=sp, num_draft=-1)
    with pytest.raises(ValueError, match="stream"):
        DecodeEngine.generate_speculative(eng, [1, 2], 4, draft, sampling=sp, stream=-1)
    # generate(sampling=..., draft=...) refuses as before: generate_speculative is the entry point
    with pytest.raises(ValueError, match="draft"):
        DecodeEngine.generate(eng, [1, 2], 4, sampling=sp, draft=draft)
