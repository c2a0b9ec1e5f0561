"""Per-token log-probabilities without a GPU: the numpy reference of tests/logprob_ref.py on hand-made rows, mq_logprob_top's ABI
(declared, bound, exported, struct layout, argument checks before any HIP call), the generate(logprobs=...) argument checks and the
barrier audit of mq_logprob.hip.  Pointers are fake and never read."""
import ctypes
import math
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import logprob_ref as R  # noqa: E402

P = 0x10000
INF = float("inf")


@pytest.fixture(scope="module")
def lib():
    from mobilequant_amd import _lib, build
    build.build()
    return _lib.load()


# ---- the reference -------------------------------------------------------------------------------------------------------------------
def test_reference_on_a_hand_made_distribution():
    p = np.array([0.1, 0.4, 0.2, 0.3])
    l = (np.log(p) + 1.25).astype(np.float32)                         # a shift does not move a log-softmax
    lp, rank, ids, tl = R.logprob_ref(l, 2, 3)
    assert rank == 3 and ids.tolist() == [1, 3, 2]
    assert abs(lp - math.log(0.2)) < 1e-6 and np.allclose(tl, np.log([0.4, 0.3, 0.2]), atol=1e-6)
    assert R.logprob_ref(l, 1, 0)[1] == 1 and R.logprob_ref(l, 0, 0)[1] == 4
    assert R.logprob_ref(l, 1, 0)[2].shape == (0,)


def test_reference_orders_ties_by_index_and_pads_past_the_vocabulary():
    l = np.array([1.0, 2.0, 2.0, 1.0], dtype=np.float32)
    lp, rank, ids, tl = R.logprob_ref(l, 3, 6)
    assert ids.tolist() == [1, 2, 0, 3, -1, -1] and rank == 4
    assert tl[0] == tl[1] and tl[2] == tl[3] == lp and np.all(tl[4:] == -INF)
    assert R.logprob_ref(l, 2, 0)[1] == 2 and R.logprob_ref(l, 0, 0)[1] == 3


def test_reference_special_values():
    nan = float("nan")
    # NaN is -inf; -0 ties with +0 and the lower index goes first
    l = np.array([-0.0, nan, 0.0, -INF], dtype=np.float32)
    lp, rank, ids, tl = R.logprob_ref(l, 2, 4)
    assert ids.tolist() == [0, 2, 1, 3] and rank == 2
    assert abs(lp - math.log(0.5)) < 1e-12 and tl[0] == tl[1] and tl[2] == tl[3] == -INF
    assert R.logprob_ref(l, 1, 0)[:2] == (-INF, 3)
    # an all -inf / NaN row: every lp -inf, the order is the index order
    l = np.array([-INF, nan, -INF, -INF], dtype=np.float32)
    lp, rank, ids, tl = R.logprob_ref(l, 2, 2)
    assert lp == -INF and rank == 3 and ids.tolist() == [0, 1] and np.all(tl == -INF)
    # +inf logits share the mass; everything else is -inf
    l = np.array([3.0, INF, -1.0, INF], dtype=np.float32)
    lp, rank, ids, tl = R.logprob_ref(l, 3, 3)
    assert ids.tolist() == [1, 3, 0] and rank == 2 and abs(lp + math.log(2)) < 1e-12 and tl[2] == -INF
    assert R.logprob_ref(np.array([0.0, INF, 1.0, 2.0], dtype=np.float32), 1, 1)[0] == 0.0
    # a token outside the vocabulary
    for t in (-1, 4, 1 << 40):
        lp, rank, ids, _ = R.logprob_ref(l, t, 1)
        assert math.isnan(lp) and rank == 0 and ids.tolist() == [1]


def test_reference_bound_stays_under_the_cap_for_the_tested_inputs():
    """Gaussian logits of scale 3 up to V = 2^20: |lp| stays below 36 (max - min of 2^20 draws is under 10.5 sigma = 31.5, log S under
    log V = 13.9 -- and the two do not reach their ends together), where the bound is still below 1e-5."""
    assert R.bound(1 << 20, 36.0) <= 1e-5
    assert R.bound(4, 0.0) > 2.0 ** -24 * 40                          # the summation term is there at any V


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def _args(**kw):
    from mobilequant_amd._lib import MQ_LOGPROB_SCRATCH_BYTES, MqLogprobTopArgs
    a = MqLogprobTopArgs()
    a.logits, a.tok, a.logprob, a.rank, a.top_id, a.top_logprob, a.scratch = P, P, P, P, P, P, P
    a.logits_stride, a.V, a.rows, a.n_top, a.batch, a.cache_len, a.record_len = 32000, 32000, 2, 5, 2, 64, 64
    a.scratch_bytes = MQ_LOGPROB_SCRATCH_BYTES
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _rejects(lib, a, text):
    rc = lib.mq_logprob_top(ctypes.byref(a), None)
    msg = lib.mq_last_error()
    assert rc == 1 and text.encode() in msg, (rc, msg)


def test_entry_is_declared_exported_and_the_struct_matches_the_header(lib):
    from mobilequant_amd import _lib
    from mobilequant_amd._lib import MqLogprobTopArgs
    assert "mq_logprob_top" in _lib.EXPORTED_SYMBOLS and hasattr(lib, "mq_logprob_top")
    hdr = open(os.path.join(ROOT, "include", "mobilequant_amd.h")).read()
    assert re.search(r"int mq_logprob_top\(const mq_logprob_top_args\* args, mq_stream_t stream\);", hdr)
    assert int(re.search(r"#define MQ_LOGPROB_SCRATCH_BYTES (\d+)", hdr).group(1)) == _lib.MQ_LOGPROB_SCRATCH_BYTES
    assert int(re.search(r"#define MQ_LOGPROB_MAX_TOP (\d+)", hdr).group(1)) == _lib.MQ_LOGPROB_MAX_TOP == R.MAX_TOP
    assert int(re.search(r"#define MQ_VERSION (\d+)", hdr).group(1)) == lib.mq_version()
    af = [f for f, _ in MqLogprobTopArgs._fields_]
    src = "\n".join(["#include <stddef.h>", "#include <stdio.h>", '#include "mobilequant_amd.h"', "int main(void) {",
                     '  printf("%zu' + " %zu" * len(af) + '\\n", sizeof(mq_logprob_top_args), ' + ", ".join(f"offsetof(mq_logprob_top_args, {f})" for f in af) + ");",
                     "  return 0;", "}"])
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        open(c, "w").write(src)
        cc = next((x for x in ("cc", "gcc", "clang") if subprocess.run(["which", x], stdout=subprocess.PIPE).returncode == 0), None)
        if cc is None:
            cc = "/opt/rocm/llvm/bin/clang"
        subprocess.run([cc, "-I" + os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        out = subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert [int(v) for v in out.split()] == [ctypes.sizeof(MqLogprobTopArgs)] + [getattr(MqLogprobTopArgs, f).offset for f in af]


def test_rejects_argument_blocks_outside_the_limits(lib):
    assert lib.mq_logprob_top(None, None) == 1 and b"null argument block" in lib.mq_last_error()
    _rejects(lib, _args(V=31999, logits_stride=32000), "V=31999")
    _rejects(lib, _args(V=(1 << 20) + 4, logits_stride=(1 << 20) + 4), "multiple of 4 in [4, 2^20]")
    _rejects(lib, _args(V=0), "V=0")
    _rejects(lib, _args(logits_stride=31996), "logits_stride=31996")
    _rejects(lib, _args(logits_stride=32002), "logits_stride=32002")
    for r in (0, 9, -1):
        _rejects(lib, _args(rows=r, batch=8), "outside 1..8")
    for n in (21, -1):
        _rejects(lib, _args(n_top=n), f"n_top={n}")
    for f in ("logits", "tok", "logprob", "rank"):
        _rejects(lib, _args(**{f: None}), "null pointer")
    _rejects(lib, _args(scratch=None), "scratch is required")
    _rejects(lib, _args(scratch_bytes=8192), "scratch_bytes=8192")
    _rejects(lib, _args(top_logprob=None), "top_id and top_logprob go together")
    _rejects(lib, _args(top_id=None), "top_id and top_logprob go together")
    _rejects(lib, _args(top_id=None, top_logprob=None), "needs top_id and top_logprob")
    # at most one index form
    _rejects(lib, _args(pos=P, n_base=P), "more than one index form")
    _rejects(lib, _args(pos=P, row_seq=P, row_pos=P), "more than one index form")
    _rejects(lib, _args(n_base=P, row_seq=P, row_pos=P), "more than one index form")
    _rejects(lib, _args(row_seq=P), "row_seq and row_pos go together")
    _rejects(lib, _args(batch=0), "batch=0")
    _rejects(lib, _args(rows=3, batch=2, pos=P), "rows=3 above batch=2")
    _rejects(lib, _args(record_len=0), "record_len=0")
    _rejects(lib, _args(pos=P, cache_len=0), "cache_len=0")
    _rejects(lib, _args(n_base=P, n_offset=(1 << 30) + 1), "n_offset")
    _rejects(lib, _args(logits=P + 8), "16-byte aligned")
    _rejects(lib, _args(tok=P + 4), "8-byte")
    _rejects(lib, _args(rank=P + 2), "4-byte aligned")


def test_no_barrier_with_lds_traffic_in_flight(tmp_path):
    """tools/barrier_audit.py on mq_logprob.hip: no s_barrier with an LDS operation possibly in flight; no private segment."""
    from mobilequant_amd import build
    flags = [f for f in build.FLAGS if f != "-fPIC"]
    src = "mq_logprob.hip"
    assert src in build.SOURCES
    asm = str(tmp_path / "mq_logprob.s")
    cmd = [build.HIPCC, *flags, *build.PER_FILE_FLAGS.get(src, ()), "-w", "--cuda-device-only", "-S", os.path.join(ROOT, "mobilequant_amd", "csrc", src), "-o", asm]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    rep = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "barrier_audit.py"), asm], stdout=subprocess.PIPE, text=True).stdout
    assert "PENDING" not in rep and "possibly in flight 0" in rep, rep
    text = open(asm).read()
    for k in ("logprob_slices_kernel", "logprob_merge_kernel", "logprob_row_kernel"):
        assert re.search(k, text), k
    assert re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text) == ["0", "0", "0"]      # the 16 entries and keys stay in registers
    assert "global_atomic" not in text and "ds_add_f32" not in text     # no atomics: the sum's order is fixed


# ---- the Python surface ----------------------------------------------------------------------------------------------------------------
def test_check_logprobs():
    from mobilequant_amd import SamplingParams
    from mobilequant_amd.sampling import check_logprobs
    sp = SamplingParams(temperature=0)
    assert check_logprobs("x", None, None) is None and check_logprobs("x", None, sp) is None
    assert check_logprobs("x", 0, sp) == 0 and check_logprobs("x", 20, sp) == 20 and check_logprobs("x", np.int64(5), sp) == 5
    for bad in (-1, 21, 1.0, "5", True, [5]):
        with pytest.raises(ValueError, match="0..20"):
            check_logprobs("x", bad, sp)
    with pytest.raises(ValueError, match=r"SamplingParams\(temperature=0\)"):
        check_logprobs("x", 5, None)


def test_engines_check_logprobs_before_touching_the_device():
    """The checks run in front of everything else in generate / generate_speculative: a bare object stands in for an engine."""
    from mobilequant_amd import SamplingParams
    from mobilequant_amd.decode import DecodeEngine
    from mobilequant_amd.decode_batch import BatchDecodeEngine
    sp = SamplingParams(temperature=0.7, top_k=40)
    draft = lambda ids, k: []      # noqa: E731
    eng = object.__new__(DecodeEngine)
    be = object.__new__(BatchDecodeEngine)
    be.batch, be.cache_len = 2, 64
    for bad in (-1, 21, 2.0, "3", True):
        with pytest.raises(ValueError, match="logprobs="):
            DecodeEngine.generate(eng, [1, 2], 4, sampling=sp, logprobs=bad)
        with pytest.raises(ValueError, match="logprobs="):
            DecodeEngine.generate_speculative(eng, [1, 2], 4, draft, sampling=sp, logprobs=bad)
        with pytest.raises(ValueError, match="logprobs="):
            BatchDecodeEngine.generate(be, [[1], [2]], 4, sampling=sp, logprobs=bad)
        with pytest.raises(ValueError, match="logprobs="):
            BatchDecodeEngine.generate_speculative(be, [[1], [2]], 4, draft, sampling=sp, logprobs=bad)
    # without sampling=: plain greedy, do_sample and generate(draft=...) pick their tokens with torch
    for kw in ({}, {"do_sample": True}, {"draft": draft}):
        with pytest.raises(ValueError, match=r"SamplingParams\(temperature=0\)"):
            DecodeEngine.generate(eng, [1, 2], 4, logprobs=5, **kw)
        with pytest.raises(ValueError, match=r"SamplingParams\(temperature=0\)"):
            BatchDecodeEngine.generate(be, [[1], [2]], 4, logprobs=5, **kw)
    # the existing refusals stay in front of a valid logprobs
    with pytest.raises(ValueError, match="do_sample"):
        DecodeEngine.generate(eng, [1, 2], 4, do_sample=True, sampling=sp, logprobs=5)
    with pytest.raises(ValueError, match="do_sample"):
        BatchDecodeEngine.generate(be, [[1], [2]], 4, do_sample=True, sampling=sp, logprobs=5)
    for e in (eng, be):
        with pytest.raises(ValueError, match="0..20"):
            type(e).set_logprobs(e, 21)


def test_the_package_exports_the_op_and_the_record_type():
    import mobilequant_amd as mq
    assert callable(mq.ops.logprob_top) and mq.TokenLogprobs._fields == ("logprob", "rank", "top_id", "top_logprob")
    with pytest.raises(RuntimeError, match="no CPU path"):
        import torch
        mq.ops.logprob_top(torch.zeros(1, 8), torch.zeros(1, dtype=torch.int64), 2)
