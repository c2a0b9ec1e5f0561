"""Seeded token selection without a GPU: the numpy Philox of tests/sampling_ref.py against Random123's known answers, the reference
rule against exact enumeration, mq_sample's ABI (declared, bound, exported, struct layouts, argument checks before any HIP call),
SamplingParams' range checks, the engines' ValueErrors and the barrier audit of mq_sample.hip.  Pointers are fake and never read."""
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

import sampling_ref as R  # noqa: E402

P = 0x10000


@pytest.fixture(scope="module")
def lib():
    from mobilequant_amd import _lib, build
    build.build()
    return _lib.load()


# ---- the generator -----------------------------------------------------------------------------------------------------------------
def test_numpy_philox_reproduces_the_published_known_answers():
    """Random123's kat_vectors for philox4x32-10 (zeros, all ones, digits of pi).  The zero and the pi vectors were also reproduced
    with an independent implementation (ATen's PhiloxRNGEngine.h) before they were pinned here."""
    kat = [([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
           ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
           ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])]
    for ctr, key, want in kat:
        assert [int(x) for x in R.philox4x32_10(ctr, key)] == want
    # vectorised over the counter: the same words as one call per counter
    idx = np.arange(0, 64)
    block = R.philox4x32_10([5, idx, 7, 9], [11, 13])
    for i in (0, 17, 63):
        assert [int(w[i]) for w in block] == [int(x) for x in R.philox4x32_10([5, i, 7, 9], [11, 13])]


def test_uniforms_are_exact_and_strictly_inside_the_unit_interval():
    u = R.uniforms(3, 1 << 40, 12, np.arange(1 << 16))
    assert u.dtype == np.float32 and u.min() > 0 and u.max() < 1
    k = u.astype(np.float64) * 2.0 ** 23 - 0.5                      # exact in fp32: the 23-bit integer comes back
    assert np.array_equal(k, np.round(k)) and k.min() >= 0 and k.max() < 2 ** 23
    # entries 4j .. 4j + 3 are the four words of one block
    r = R.philox4x32_10([12, 5, 0, 1 << 8], [3, 0])
    assert np.array_equal(u[20:24], ((np.array([int(x) for x in r], dtype=np.uint32) >> np.uint32(9)).astype(np.float32) + np.float32(0.5))
                          * np.float32(2.0 ** -23))
    # the edge the rule avoids: 24 random bits + 0.5 is not an fp32 number at the top of the range
    assert np.float32(2 ** 24 - 1) + np.float32(0.5) == np.float32(2 ** 24)


# ---- the reference against itself ------------------------------------------------------------------------------------------------
def test_reference_candidate_sets_on_hand_checked_rows():
    l = np.log(np.array([0.4, 0.3, 0.2, 0.1], dtype=np.float64)).astype(np.float32)
    z = lambda **kw: sorted(R.analyse(l, 1.0, kw.get("k", 0), kw.get("p", 1.0), kw.get("m", 0.0), 0, 0, 0)["C"].tolist())      # noqa: E731
    assert z() == [0, 1, 2, 3]
    assert z(k=2) == [0, 1]
    assert z(p=0.5) == [0, 1]                # 0.4 < 0.5 <= 0.7
    assert z(p=0.39) == [0]
    assert z(p=0.95) == [0, 1, 2, 3]
    assert z(k=3, p=0.8) == [0, 1, 2]        # 0.8 of the top-3 mass 0.9 = 0.72 > 0.7
    assert z(m=0.6) == [0, 1]                # 0.3 / 0.4 >= 0.6 > 0.2 / 0.4
    assert z(k=4, m=0.3) == [0, 1, 2]
    tie = np.array([1.0, 2.0, 2.0, 2.0, 0.0, 2.0], dtype=np.float32)
    assert sorted(R.analyse(tie, 1.0, 2, 1.0, 0.0, 0, 0, 0)["C"].tolist()) == [1, 2]           # ties enter by index
    assert R.analyse(tie, 0.0, 0, 1.0, 0.0, 0, 0, 0)["token"] == 1
    assert R.analyse(np.full(8, -np.inf, dtype=np.float32), 1.0, 0, 1.0, 0.0, 0, 0, 0)["token"] == 0
    nan = np.array([np.nan, 0.5, np.nan, 0.25], dtype=np.float32)
    assert R.analyse(nan, 0.0, 0, 1.0, 0.0, 0, 0, 0)["token"] == 1


@pytest.mark.parametrize("top_k,top_p,min_p", [(0, 1.0, 0.0), (5, 1.0, 0.0), (0, 0.7, 0.0), (6, 0.8, 0.1)])
def test_reference_gumbel_max_draws_the_enumerated_distribution(top_k, top_p, min_p):
    """float64 Gumbel-max over C against exact enumeration on a tiny vocabulary: 40 000 draws, chi-square below the 1 - 1e-6 quantile."""
    V, N, T = 12, 40000, 0.8
    rng = np.random.default_rng(3)
    l = rng.standard_normal(V).astype(np.float32)
    p = R.restricted_softmax(l, T, top_k, top_p, min_p)
    C = np.flatnonzero(p > 0)
    z = (l / np.float32(T)).astype(np.float32).astype(np.float64)
    n = np.arange(N)
    counts = np.zeros(V)
    u = np.stack([R.uniforms(17, 4, n, np.full(N, i)) for i in range(V)], axis=1)          # [N, V]
    score = np.where(p > 0, z + R.gumbel64(u), -np.inf)
    tok = np.argmax(score, axis=1)
    counts = np.bincount(tok, minlength=V).astype(np.float64)
    assert counts[p == 0].sum() == 0
    one = R.analyse(l, T, top_k, top_p, min_p, 17, 4, 123)
    assert one["token"] == int(np.argmax(np.where(p > 0, z + R.gumbel64(R.uniforms(17, 4, 123, np.arange(V))), -np.inf)))
    exp = p[C] * N
    chi2 = float(((counts[C] - exp) ** 2 / exp).sum())
    from test_gpu_sample import CHI2_1E6
    assert chi2 < CHI2_1E6[len(C) - 2], (chi2, len(C))


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------
def _args(**kw):
    from mobilequant_amd._lib import MQ_SAMPLE_SCRATCH_BYTES, MqSampleArgs
    a = MqSampleArgs()
    a.logits, a.pos, a.params, a.tok, a.scratch = P, P, P, P, P
    a.logits_stride, a.V, a.rows, a.cache_len, a.scratch_bytes = 32000, 32000, 2, 256, MQ_SAMPLE_SCRATCH_BYTES
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _rejects(lib, a, text):
    rc = lib.mq_sample(ctypes.byref(a), None)
    msg = lib.mq_last_error()
    assert rc == 1 and text.encode() in msg, (rc, msg)


def test_entry_is_declared_exported_and_the_structs_match_the_header(lib):
    from mobilequant_amd import _lib
    from mobilequant_amd._lib import MqSampleArgs, MqSampleRow
    from mobilequant_amd.sampling import ROW_DTYPE
    assert "mq_sample" in _lib.EXPORTED_SYMBOLS and "mq_sample_uniforms" in _lib.EXPORTED_SYMBOLS
    assert hasattr(lib, "mq_sample") and hasattr(lib, "mq_sample_uniforms")
    hdr = open(os.path.join(ROOT, "include", "mobilequant_amd.h")).read()
    assert re.search(r"int mq_sample\(const mq_sample_args\* args, mq_stream_t stream\);", hdr)
    assert int(re.search(r"#define MQ_VERSION (\d+)", hdr).group(1)) == 304 == lib.mq_version()
    assert int(re.search(r"#define MQ_SAMPLE_SCRATCH_BYTES (\d+)", hdr).group(1)) == _lib.MQ_SAMPLE_SCRATCH_BYTES
    rf = ("temperature", "top_k", "top_p", "min_p", "seed", "stream")
    af = ("logits", "logits_stride", "V", "rows", "pos", "cache_len", "params", "tok", "kept", "logprob", "scratch", "scratch_bytes")
    src = "\n".join(["#include <stddef.h>", "#include <stdio.h>", '#include "mobilequant_amd.h"', "int main(void) {",
                     '  printf("%zu' + " %zu" * len(rf) + '\\n", sizeof(mq_sample_row), ' + ", ".join(f"offsetof(mq_sample_row, {f})" for f in rf) + ");",
                     '  printf("%zu' + " %zu" * len(af) + '\\n", sizeof(mq_sample_args), ' + ", ".join(f"offsetof(mq_sample_args, {f})" for f in af) + ");",
                     "  return 0;", "}"])
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        open(c, "w").write(src)
        cc = next((x for x in ("cc", "gcc", "clang") if subprocess.run(["which", x], stdout=subprocess.PIPE).returncode == 0), None)
        if cc is None:
            cc = "/opt/rocm/llvm/bin/clang"
        subprocess.run([cc, "-I" + os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        out = subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")
    assert [int(v) for v in out[0].split()] == [ctypes.sizeof(MqSampleRow)] + [getattr(MqSampleRow, f).offset for f in rf]
    assert [int(v) for v in out[1].split()] == [ctypes.sizeof(MqSampleArgs)] + [getattr(MqSampleArgs, f).offset for f in af]
    assert ROW_DTYPE.itemsize == 32 and [ROW_DTYPE.fields[f][1] for f in rf] == [getattr(MqSampleRow, f).offset for f in rf]


def test_rejects_argument_blocks_outside_the_limits(lib):
    assert lib.mq_sample(None, None) == 1 and b"null argument block" in lib.mq_last_error()
    for f in ("logits", "pos", "params", "tok", "scratch"):
        _rejects(lib, _args(**{f: None}), "null pointer")
    for r in (0, 9, -1):
        _rejects(lib, _args(rows=r), "outside 1..8")
    _rejects(lib, _args(V=31999, logits_stride=32000), "V=31999")
    _rejects(lib, _args(V=(1 << 20) + 4, logits_stride=(1 << 20) + 4), "multiple of 4 in [4, 2^20]")
    _rejects(lib, _args(V=0), "V=0")
    _rejects(lib, _args(logits_stride=31996), "logits_stride=31996")
    _rejects(lib, _args(logits_stride=32002), "logits_stride=32002")
    _rejects(lib, _args(cache_len=0), "cache_len=0")
    _rejects(lib, _args(logits=P + 8), "16-byte aligned")
    _rejects(lib, _args(params=P + 8), "16-byte aligned")
    _rejects(lib, _args(tok=P + 4), "8-byte")
    _rejects(lib, _args(kept=P + 2), "4-byte aligned")
    _rejects(lib, _args(scratch_bytes=4096), "scratch_bytes=4096")
    assert lib.mq_sample_uniforms(0, 0, 0, 0, 16, None, None) == 1 and b"null pointer" in lib.mq_last_error()
    assert lib.mq_sample_uniforms(0, 0, 0, -1, 16, P, None) == 1 and b"first=-1" in lib.mq_last_error()
    assert lib.mq_sample_uniforms(0, 0, 0, 0, 0, P, None) == 1 and b"count=0" in lib.mq_last_error()


def test_no_barrier_with_lds_traffic_in_flight(tmp_path):
    """tools/barrier_audit.py on mq_sample.hip: no s_barrier with an LDS operation possibly in flight."""
    from mobilequant_amd import build
    flags = [f for f in build.FLAGS if f != "-fPIC"]
    src = "mq_sample.hip"
    assert src in build.SOURCES
    asm = str(tmp_path / "mq_sample.s")
    cmd = [build.HIPCC, *flags, *build.PER_FILE_FLAGS.get(src, ()), "-w", "--cuda-device-only", "-S", os.path.join(ROOT, "mobilequant_amd", "csrc", src), "-o", asm]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    rep = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "barrier_audit.py"), asm], stdout=subprocess.PIPE, text=True).stdout
    assert "PENDING" not in rep and "possibly in flight 0" in rep, rep
    text = open(asm).read()
    assert re.search(r"sample_select_kernelINS\S*9NoPenalty", text) and re.search(r"sample_scan_kernelINS\S*9NoPenalty", text)
    assert "ds_add_u64" in text                                     # the mass histogram is 64-bit LDS integer atomics


# ---- the Python surface ----------------------------------------------------------------------------------------------------------------
def test_sampling_params_validate_their_ranges():
    import dataclasses
    from mobilequant_amd import SamplingParams
    sp = SamplingParams()
    assert (sp.temperature, sp.top_k, sp.top_p, sp.min_p, sp.seed) == (1.0, 0, 1.0, 0.0, 0)
    with pytest.raises(dataclasses.FrozenInstanceError):
        sp.seed = 1
    SamplingParams(temperature=0, top_k=2 ** 31 - 1, top_p=1e-6, min_p=0.999, seed=2 ** 64 - 1)
    for bad in (dict(temperature=-0.1), dict(temperature=float("nan")), dict(temperature=float("inf")), dict(top_k=-1), dict(top_k=1.5),
                dict(top_k=2 ** 31), dict(top_p=0.0), dict(top_p=1.01), dict(top_p=float("nan")), dict(min_p=-0.1), dict(min_p=1.0),
                dict(seed=-1), dict(seed=2 ** 64), dict(seed=1.0), dict(temperature="1")):
        with pytest.raises(ValueError):
            SamplingParams(**bad)


def test_pack_rows_lays_out_mq_sample_row():
    from mobilequant_amd import SamplingParams
    from mobilequant_amd._lib import MqSampleRow
    from mobilequant_amd.sampling import pack_rows
    rows = pack_rows([SamplingParams(0.7, 40, 0.9, 0.05, 2 ** 64 - 2), SamplingParams()], [1 << 63, 7])
    raw = rows.tobytes()
    r0 = MqSampleRow.from_buffer_copy(raw[:32])
    assert (r0.top_k, r0.seed, r0.stream) == (40, 2 ** 64 - 2, 1 << 63)
    assert np.float32(r0.temperature) == np.float32(0.7) and np.float32(r0.top_p) == np.float32(0.9) and np.float32(r0.min_p) == np.float32(0.05)
    assert MqSampleRow.from_buffer_copy(raw[32:]).stream == 7
    with pytest.raises(ValueError):
        pack_rows([SamplingParams()], [0, 1])
    with pytest.raises(ValueError):
        pack_rows([SamplingParams()], [-1])
    with pytest.raises(TypeError):
        pack_rows([0.7], [0])


def _one_shot(name, lg):
    """sampling.<name> over the logits lg with every other argument sized to its rows, all on the CPU."""
    from mobilequant_amd import SamplingParams, sampling
    sp = SamplingParams(temperature=0.8, seed=1)
    rows = 1 if lg.dim() == 1 else lg.shape[0]
    i32, i64 = torch.zeros(rows, dtype=torch.int32), torch.zeros(rows, dtype=torch.int64)
    if name == "sample":
        return sampling.sample(lg, i32, ([sp] * rows, list(range(rows))), i64)
    if name == "sample_rows":
        return sampling.sample_rows(lg, torch.zeros(1, dtype=torch.int32), 0, sp, 0, i64, proposals=torch.zeros(max(rows - 1, 0), dtype=torch.int64))
    return sampling.sample_ragged(lg, i32, i32.clone(), i64, 1, ([sp, sp], [0, 1]), i64.clone())


@pytest.mark.parametrize("name", ["sample", "sample_rows", "sample_ragged"])
def test_the_one_shot_functions_check_their_logits_alike_and_before_any_device(name):
    with pytest.raises(RuntimeError, match="ROCm device tensor"):
        _one_shot(name, torch.zeros(4, 160))
    with pytest.raises(RuntimeError, match="fp32"):
        _one_shot(name, torch.zeros(4, 160).double())
    for rows in (0, 9):
        with pytest.raises(RuntimeError, match="outside 1..8"):
            _one_shot(name, torch.zeros(rows, 160))
    with pytest.raises(RuntimeError, match="unit column stride"):
        _one_shot(name, torch.zeros(160, 4).t())
    with pytest.raises(RuntimeError, match="ROCm device tensor"):
        _one_shot(name, torch.zeros(160))                             # 1-D logits are one row: only the device is wrong


def test_engines_refuse_sampling_with_do_sample_or_a_draft_before_touching_the_device():
    """The checks run in front of everything else in generate: a bare object stands in for an engine."""
    from mobilequant_amd import SamplingParams
    from mobilequant_amd.decode import DecodeEngine
    from mobilequant_amd.decode_batch import BatchDecodeEngine
    sp = SamplingParams(temperature=0.7, top_k=40)
    eng = object.__new__(DecodeEngine)
    with pytest.raises(ValueError, match="do_sample"):
        DecodeEngine.generate(eng, [1, 2], 4, do_sample=True, sampling=sp)
    with pytest.raises(ValueError, match="draft"):
        DecodeEngine.generate(eng, [1, 2], 4, sampling=sp, draft=lambda ids, k: [])
    with pytest.raises(ValueError, match="greedy decoding only"):
        DecodeEngine.generate(eng, [1, 2], 4, do_sample=True, draft=lambda ids, k: [])        # the existing refusal stays
    be = object.__new__(BatchDecodeEngine)
    be.batch, be.cache_len = 2, 64
    with pytest.raises(ValueError, match="do_sample"):
        BatchDecodeEngine.generate(be, [[1], [2]], 4, do_sample=True, sampling=sp)
    with pytest.raises(ValueError, match="2 streams for 2 prompts|1 SamplingParams"):
        BatchDecodeEngine.generate(be, [[1], [2]], 4, sampling=[sp])
    with pytest.raises(ValueError, match="streams"):
        BatchDecodeEngine.generate(be, [[1], [2]], 4, sampling=sp, streams=[0])
    with pytest.raises(ValueError, match="streams= belongs to sampling="):
        BatchDecodeEngine.generate(be, [[1], [2]], 4, streams=[0, 1])
    with pytest.raises(ValueError, match="exceeds the cache"):
        BatchDecodeEngine.generate(be, [[1] * 61, [2]], 4, sampling=sp)
    with pytest.raises(TypeError):
        BatchDecodeEngine.generate(be, [[1], [2]], 4, sampling=[sp, 0.7])
