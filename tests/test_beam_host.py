"""Beam search without a GPU: the ABI of mq_beam_select and mq_decode_cache_reorder (declared, bound, exported, struct
layout, argument checks before any HIP call), the compiled kernels' metadata and barrier audit, the wrappers' refusals that need no
device, generate_beam's argument errors on a bare object that stands in for an engine, and tests/beam_ref.py's host rule against the
beam search of `transformers` on a tiny random CPU Llama.  Pointers are fake and never read."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
P = 0x10000


@pytest.fixture(scope="module")
def lib():
    from mobilequant_amd import _lib, build
    build.build()
    return _lib.load()


# ---- the C entry points --------------------------------------------------------------------------------------------------------------
def _select_args(**kw):
    from mobilequant_amd import _lib
    a = _lib.MqBeamSelectArgs()
    for f in ("logits", "cum", "group", "cand_score", "cand_row", "cand_token", "cand_logprob", "row_lse", "scratch"):
        setattr(a, f, P)
    a.logits_stride, a.V, a.rows, a.n_groups, a.n_cand, a.scratch_bytes = 32000, 32000, 8, 2, 8, _lib.MQ_BEAM_SCRATCH_BYTES
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _reorder_args(**kw):
    from mobilequant_amd._lib import MqDecodeCacheForkArgs
    a = MqDecodeCacheForkArgs()
    a.caches, a.pos, a.parent = P, P, P
    a.n_caches, a.batch, a.kv_heads, a.cache_len, a.head_dim = 44, 8, 4, 2048, 64
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _rejects(lib, fn, a, text):
    rc = getattr(lib, fn)(ctypes.byref(a), None)
    msg = lib.mq_last_error()
    assert rc == 1 and msg.startswith(fn.encode() + b": ") and text.encode() in msg, (rc, msg)


def test_entries_are_declared_exported_and_the_struct_matches_the_header(lib):
    from mobilequant_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "mobilequant_amd.h")).read()
    for fn, src in (("mq_beam_select", "mq_beam.hip"), ("mq_decode_cache_reorder", "mq_decode_reorder.hip")):
        assert fn in _lib.EXPORTED_SYMBOLS and hasattr(lib, fn) and src in build.SOURCES
    assert re.search(r"int mq_beam_select\(const mq_beam_select_args\* args, mq_stream_t stream\);", hdr)
    assert re.search(r"int mq_decode_cache_reorder\(const mq_decode_cache_fork_args\* args, mq_stream_t stream\);", hdr)
    assert int(re.search(r"#define MQ_BEAM_SCRATCH_BYTES (\d+)", hdr).group(1)) == _lib.MQ_BEAM_SCRATCH_BYTES == _lib.MQ_LOGPROB_SCRATCH_BYTES + 8 * 20 * 16
    assert int(re.search(r"#define MQ_VERSION (\d+)", hdr).group(1)) // 100 == _lib.HEADER_MAJOR == lib.mq_version() // 100     # additive entries: the major stays
    S = _lib.MqBeamSelectArgs
    af = [f for f, _ in S._fields_]
    src = "\n".join(["#include <stddef.h>", "#include <stdio.h>", '#include "mobilequant_amd.h"', "int main(void) {",
                     '  printf("%zu' + " %zu" * len(af) + '\\n", sizeof(mq_beam_select_args), ' +
                     ", ".join(f"offsetof(mq_beam_select_args, {f})" for f in af) + ");", "  return 0;", "}"])
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        open(c, "w").write(src)
        cc = next((x for x in ("cc", "gcc", "clang") if subprocess.run(["which", x], stdout=subprocess.PIPE).returncode == 0), None)
        if cc is None:
            cc = "/opt/rocm/llvm/bin/clang"
        subprocess.run([cc, "-I" + os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        out = subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert [int(v) for v in out.split()] == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in af]


def test_beam_select_rejects_argument_blocks_outside_the_limits(lib):
    """Every check returns 1 with its message before any HIP call: this process has no device, and the pointers are fake."""
    fn = "mq_beam_select"
    assert lib.mq_beam_select(None, None) == 1 and lib.mq_last_error().startswith(b"mq_beam_select: null argument block")
    for f in ("logits", "cum", "group", "cand_score", "cand_row", "cand_token", "cand_logprob", "row_lse", "scratch"):
        _rejects(lib, fn, _select_args(**{f: None}), "null pointer")
    for r in (0, -1, 9):
        _rejects(lib, fn, _select_args(rows=r), f"rows={r} outside 1..8")
    for v in (0, 2, 30, 31999, (1 << 20) + 4):
        _rejects(lib, fn, _select_args(V=v, logits_stride=1 << 21), f"V={v} must be a multiple of 4 in [4, 2^20]")
    for s in (31996, 32002):
        _rejects(lib, fn, _select_args(logits_stride=s), f"logits_stride={s} must be >= V and a multiple of 4")
    for g in (0, -1, 9):
        _rejects(lib, fn, _select_args(n_groups=g), f"n_groups={g} outside 1..8")
    for k in (0, -1, 21):
        _rejects(lib, fn, _select_args(n_cand=k), f"n_cand={k} outside 1..20")
    _rejects(lib, fn, _select_args(scratch_bytes=363007), "scratch_bytes=363007 below MQ_BEAM_SCRATCH_BYTES")
    _rejects(lib, fn, _select_args(logits=P + 8), "16-byte aligned")
    _rejects(lib, fn, _select_args(scratch=P + 4), "16-byte aligned")
    for f in ("cum", "group", "cand_score", "cand_row", "cand_token", "cand_logprob", "row_lse"):
        _rejects(lib, fn, _select_args(**{f: P + 2}), "4-byte aligned")


def test_cache_reorder_rejects_what_cache_fork_rejects(lib):
    fn = "mq_decode_cache_reorder"
    assert lib.mq_decode_cache_reorder(None, None) == 1 and lib.mq_last_error().startswith(b"mq_decode_cache_reorder: null argument block")
    for f in ("caches", "pos", "parent"):
        _rejects(lib, fn, _reorder_args(**{f: None}), "null pointer")
    for n in (0, -1, 1025):
        _rejects(lib, fn, _reorder_args(n_caches=n), f"n_caches={n} outside 1..1024")
    for b in (0, -1, 9):
        _rejects(lib, fn, _reorder_args(batch=b), f"batch={b} outside 1..8")
    for h in (0, -3):
        _rejects(lib, fn, _reorder_args(kv_heads=h), f"kv_heads={h}")
    for n in (0, -1):
        _rejects(lib, fn, _reorder_args(cache_len=n), f"cache_len={n}")
    for d in (0, 8, 15, 17, 24, 72, 250, 257, 272, 512, -16):
        _rejects(lib, fn, _reorder_args(head_dim=d), f"head_dim={d} must be a multiple of 16 in [16, 256]")
    _rejects(lib, fn, _reorder_args(n_caches=1024, kv_heads=64), "n_caches x kv_heads = 65536")
    _rejects(lib, fn, _reorder_args(caches=P + 4), "8-byte")
    _rejects(lib, fn, _reorder_args(pos=P + 2), "4-byte aligned")
    _rejects(lib, fn, _reorder_args(parent=P + 1), "4-byte aligned")
    # the same blocks, the same wording under the other entry point's name
    for bad in (_reorder_args(head_dim=24), _reorder_args(batch=9), _reorder_args(pos=None)):
        assert lib.mq_decode_cache_fork(ctypes.byref(bad), None) == 1
        fork = lib.mq_last_error()
        assert lib.mq_decode_cache_reorder(ctypes.byref(bad), None) == 1
        assert lib.mq_last_error() == fork.replace(b"mq_decode_cache_fork", b"mq_decode_cache_reorder")


def _compile(tmp_path, src):
    from mobilequant_amd import build
    flags = [f for f in build.FLAGS if f != "-fPIC"]
    asm = str(tmp_path / src.replace(".hip", ".s"))
    cmd = [build.HIPCC, *flags, *build.PER_FILE_FLAGS.get(src, ()), "-w", "--cuda-device-only", "-S", os.path.join(ROOT, "mobilequant_amd", "csrc", src), "-o", asm]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    return asm


def test_reorder_kernel_has_no_private_segment_and_no_lds(tmp_path):
    """The compiled kernel's metadata: no private segment (the chunk registers are compile-time indexed, nothing spilled) and no LDS."""
    text = open(_compile(tmp_path, "mq_decode_reorder.hip")).read()
    assert re.search("cache_reorder_kernel", text)
    assert re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text) == ["0"] and re.findall(r"\.group_segment_fixed_size:\s*(\d+)", text) == ["0"]
    assert "global_load_dwordx4" in text and "global_store_dwordx4" in text


def test_beam_kernels_use_static_lds_only_and_pass_the_barrier_audit(tmp_path):
    """tools/barrier_audit.py on the new source with barriers (test_cabi.py's audit covers a fixed list of files; mq_logprob.hip shares
    the audited bodies through mq_logprob_slice.h and is audited beside it): no s_barrier with LDS traffic in flight on any path."""
    for src, kernels in (("mq_beam.hip", 4), ("mq_logprob.hip", 3)):
        asm = _compile(tmp_path, src)
        rep = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "barrier_audit.py"), asm], stdout=subprocess.PIPE, text=True).stdout
        assert "PENDING" not in rep and "possibly in flight 0" in rep, rep
        text = open(asm).read()
        assert re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text) == ["0"] * kernels
        lds = [int(v) for v in re.findall(r"\.group_segment_fixed_size:\s*(\d+)", text)]
        assert len(lds) == kernels and 0 < max(lds) <= 48 * 1024        # static, below the 64 KiB a launch gets without an attribute


# ---- the wrappers: refusals that need no device -----------------------------------------------------------------------------------------
def test_ops_refuse_before_the_c_call():
    import mobilequant_amd as mq
    assert mq.beam_select is mq.ops.beam_select and mq.decode_cache_reorder is mq.ops.decode_cache_reorder
    R = mq.ops.decode_cache_reorder
    c = torch.zeros(2, 1, 8, 16, dtype=torch.int8)
    i32 = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="decode_cache_reorder needs at least one cache"):
        R([], i32, i32)
    with pytest.raises(RuntimeError, match="decode_cache_reorder: caches are int8"):
        R([c.to(torch.float32)], i32, i32)
    with pytest.raises(ValueError, match="different shapes"):
        R([c, torch.zeros(2, 1, 9, 16, dtype=torch.int8)], i32, i32)
    with pytest.raises(RuntimeError, match=r"decode_cache_reorder: parent must be a contiguous int32 \[2\]"):
        R([c], i32, i32.to(torch.int64))
    with pytest.raises(ValueError, match="head_dim=24"):
        R([torch.zeros(2, 1, 8, 24, dtype=torch.int8)], i32, i32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        R([c], i32, i32)
    S = mq.ops.beam_select
    lg, cum, grp = torch.zeros(4, 160), torch.zeros(4), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path|ROCm device tensor"):
        S(lg, cum, grp, 1, 4)


def test_torch_library_registration_and_meta_kernels():
    import mobilequant_amd.torch_ops as T
    assert "decode_cache_reorder" in T.OPS and "beam_select" in T.OPS
    op = torch.ops.mobilequant_amd.decode_cache_reorder
    assert op([torch.empty(2, 1, 8, 16, dtype=torch.int8, device="meta")], torch.empty(2, dtype=torch.int32, device="meta"),
              torch.empty(2, dtype=torch.int32, device="meta")) is None
    with pytest.raises(NotImplementedError):                           # no CPU implementation to dispatch to
        op([torch.zeros(2, 1, 8, 16, dtype=torch.int8)], torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32))
    sel = torch.ops.mobilequant_amd.beam_select
    out = sel(torch.empty(8, 160, device="meta"), torch.empty(8, device="meta"), torch.empty(8, dtype=torch.int32, device="meta"), 2, 8)
    assert [tuple(t.shape) for t in out] == [(2, 8)] * 4 + [(8,)] and [t.dtype for t in out] == [torch.float32, torch.int32, torch.int32, torch.float32, torch.float32]
    with pytest.raises(NotImplementedError):
        sel(torch.zeros(8, 160), torch.zeros(8), torch.zeros(8, dtype=torch.int32), 2, 8)


# ---- generate_beam: argument errors on a bare object -----------------------------------------------------------------------------------
def _bare(batch=8):
    from mobilequant_amd.decode_batch import BatchDecodeEngine
    be = object.__new__(BatchDecodeEngine)
    be.batch, be.cache_len = batch, 64
    be.shape = types.SimpleNamespace(vocab=160)
    be._active, be._host_pos = [False] * batch, [64] * batch
    return be


@pytest.mark.parametrize("args,kw,exc,text", [
    (([[1, 2]], 4, 0), {}, ValueError, "num_beams=0"),
    (([[1, 2]], 4, 9), {}, ValueError, "num_beams=9"),
    (([[1, 2]], 4, 2.0), {}, ValueError, "num_beams=2.0"),
    (([[1, 2]], 4, True), {}, ValueError, "num_beams=True"),
    (([], 4, 2), {}, ValueError, "0 prompts x num_beams=2 for 8 slots"),
    (([[1]] * 3, 4, 4), {}, ValueError, "3 prompts x num_beams=4 for 8 slots"),
    (([[1], []], 4, 2), {}, ValueError, "prompt 1 is empty"),
    ((7, 4, 2), {}, ValueError, "sequence of token id sequences"),
    (([[1, 160]], 4, 2), {}, IndexError, "token 160 of prompt 0 outside the vocabulary"),
    (([[1], [-1]], 4, 2), {}, IndexError, "token -1 of prompt 1"),
    (([[1, 2]], 0, 2), {}, ValueError, "max_new_tokens=0"),
    (([[1, 2]], 2.5, 2), {}, ValueError, "max_new_tokens=2.5"),
    (([[1, 2]], 4, 2), {"num_return_sequences": 3}, ValueError, "num_return_sequences=3 must be an integer in 1..num_beams (2)"),
    (([[1, 2]], 4, 2), {"num_return_sequences": 0}, ValueError, "num_return_sequences=0"),
    (([[1, 2]], 4, 8), {"eos_token_id": [3, 4]}, ValueError, "= 24 candidates per step, above 20"),
    (([[1, 2]], 4, 4), {"eos_token_id": [3, 4, 5, 6, 7]}, ValueError, "= 24 candidates per step, above 20"),
    (([[1, 2]], 4, 2), {"eos_token_id": "3"}, ValueError, "eos_token_id="),
    (([[1] * 61], 4, 2), {}, ValueError, "a prompt plus 4 new tokens exceeds the cache (64 positions)"),
    (([[1, 2]], 4, 2), {"length_penalty": float("nan")}, ValueError, "length_penalty=nan"),
    (([[1, 2]], 4, 2), {"length_penalty": "1"}, ValueError, "length_penalty='1'"),
    (([[1, 2]], 4, 2), {"early_stopping": "never"}, ValueError, "early_stopping='never'"),
])
def test_generate_beam_refuses_before_anything_is_launched(args, kw, exc, text):
    """The bare object has no device buffers at all: reaching a launch or a copy would be an AttributeError."""
    from mobilequant_amd.decode_batch import BatchDecodeEngine
    be = _bare()
    with pytest.raises(exc, match=re.escape("BatchDecodeEngine.generate_beam: ")) as e:
        BatchDecodeEngine.generate_beam(be, *args, **kw)
    assert text in str(e.value)
    assert be._active == [False] * 8 and be._host_pos == [64] * 8
    with pytest.raises(AttributeError):                                # arguments in order pass every check and reach the device buffers
        BatchDecodeEngine.generate_beam(be, [[1, 2]], 4, 2, eos_token_id=3)


def test_small_vocabulary_is_refused():
    from mobilequant_amd.decode_batch import BatchDecodeEngine
    be = _bare()
    be.shape.vocab = 12
    with pytest.raises(ValueError, match="16 candidates per step, above the vocabulary"):
        BatchDecodeEngine.generate_beam(be, [[1, 2]], 4, 8)


# ---- the host rule against transformers' beam search --------------------------------------------------------------------------------
def test_host_rule_is_transformers_beam_search_on_a_tiny_cpu_llama():
    """tests/beam_ref.py's host rule over a float64 log-softmax of a tiny random fp32 Llama's logits against `generate(num_beams=W)`
    of the installed transformers: the same sequences, scores to fp32 rounding.  Compared with and without an EOS at
    length_penalty 0, 1 and 2 and both early_stopping values: the configurations on which the installed version was found to agree
    with the written rule.  It parts from it where a prompt becomes done by an EOS of the very LAST step: the written rule (BeamSearchScorer's)
    then returns the finished hypotheses alone, the installed version still ranks that step's live beams among them ([3, 4, 5], W = 3
    with 8 new tokens is such a case and is left out)."""
    transformers = pytest.importorskip("transformers")
    import beam_ref
    torch.manual_seed(0)
    cfg = transformers.LlamaConfig(vocab_size=48, hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=4,
                                   num_key_value_heads=4, max_position_embeddings=64)
    model = transformers.LlamaForCausalLM(cfg).eval()
    rows = {}

    def lister(ids, K):
        key = tuple(ids)
        if key not in rows:
            with torch.no_grad():
                lp = torch.log_softmax(model(torch.tensor([ids])).logits[0, -1].float(), dim=-1).numpy()
            o = np.lexsort((np.arange(lp.size), -lp.astype(np.float64)))[:20]
            rows[key] = (o.astype(np.int32), lp[o].astype(np.float32))
        return rows[key][0][:K], rows[key][1][:K]

    checked = 0
    for prompt, W, new in (([3, 4, 5], 3, 9), ([9], 2, 6), ([1, 2, 3, 4, 5, 6, 7], 4, 8)):
        free = beam_ref.beam_search(lister, prompt, new, W, (), 1.0, True, W)
        eos = free[0][-1][len(prompt) + 2]                              # finishes hypotheses mid-run
        for e, lp, es in ((None, 1.0, True), (eos, 1.0, True), (eos, 0.0, True), (eos, 2.0, True), (eos, 1.0, False), (eos, 0.0, False), (eos, 2.0, False)):
            want = beam_ref.beam_search(lister, prompt, new, W, () if e is None else (e,), lp, es, W)
            with torch.no_grad():
                out = model.generate(torch.tensor([prompt]), max_new_tokens=new, num_beams=W, do_sample=False, eos_token_id=e, pad_token_id=0,
                                     length_penalty=lp, early_stopping=es, num_return_sequences=W, output_scores=True, return_dict_in_generate=True)
            got = [[int(t) for t in s] for s in out.sequences]
            for s, w, sc, wsc in zip(got, want[0], out.sequences_scores.tolist(), want[1]):
                assert s[:len(w)] == w and all(t in (0, e) for t in s[len(w):]), (prompt, W, e, lp, es, s, w)      # (transformers pads behind an EOS)
                assert abs(sc - wsc) <= 1e-4 * max(1.0, abs(wsc)), (sc, wsc)
            checked += 1
    assert checked == 21
