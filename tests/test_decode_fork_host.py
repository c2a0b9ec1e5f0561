"""Forking cached sequences without a GPU: mq_decode_cache_fork's ABI (declared, bound, exported, struct layout,
argument checks before any HIP call), ops.decode_cache_fork's refusals that need no device, and the argument errors of
BatchDecodeEngine.fork / generate(n=) / generate_speculative(n=) on a bare object that stands in for an engine.  Pointers are fake and
never read."""
import ctypes
import os
import re
import subprocess
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x10000


@pytest.fixture(scope="module")
def lib():
    from mobilequant_amd import _lib, build
    build.build()
    return _lib.load()


def _args(**kw):
    from mobilequant_amd._lib import MqDecodeCacheForkArgs
    a = MqDecodeCacheForkArgs()
    a.caches, a.pos, a.parent = P, P, P
    a.n_caches, a.batch, a.kv_heads, a.cache_len, a.head_dim = 44, 8, 4, 2048, 64
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _rejects(lib, a, text):
    rc = lib.mq_decode_cache_fork(ctypes.byref(a), None)
    msg = lib.mq_last_error()
    assert rc == 1 and msg.startswith(b"mq_decode_cache_fork: ") and text.encode() in msg, (rc, msg)


def test_entry_is_declared_exported_and_the_struct_matches_the_header(lib):
    from mobilequant_amd import _lib, build
    from mobilequant_amd._lib import MqDecodeCacheForkArgs
    assert "mq_decode_cache_fork" in _lib.EXPORTED_SYMBOLS and hasattr(lib, "mq_decode_cache_fork")
    assert "mq_decode_fork.hip" in build.SOURCES
    hdr = open(os.path.join(ROOT, "include", "mobilequant_amd.h")).read()
    assert re.search(r"int mq_decode_cache_fork\(const mq_decode_cache_fork_args\* args, mq_stream_t stream\);", hdr)
    assert int(re.search(r"#define MQ_VERSION (\d+)", hdr).group(1)) == lib.mq_version() == 304
    af = [f for f, _ in MqDecodeCacheForkArgs._fields_]
    src = "\n".join(["#include <stddef.h>", "#include <stdio.h>", '#include "mobilequant_amd.h"', "int main(void) {",
                     '  printf("%zu' + " %zu" * len(af) + '\\n", sizeof(mq_decode_cache_fork_args), ' +
                     ", ".join(f"offsetof(mq_decode_cache_fork_args, {f})" for f in af) + ");", "  return 0;", "}"])
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        open(c, "w").write(src)
        cc = next((x for x in ("cc", "gcc", "clang") if subprocess.run(["which", x], stdout=subprocess.PIPE).returncode == 0), None)
        if cc is None:
            cc = "/opt/rocm/llvm/bin/clang"
        subprocess.run([cc, "-I" + os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        out = subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert [int(v) for v in out.split()] == [ctypes.sizeof(MqDecodeCacheForkArgs)] + [getattr(MqDecodeCacheForkArgs, f).offset for f in af]


def test_rejects_argument_blocks_outside_the_limits(lib):
    """Every check returns 1 with its message before any HIP call: this process has no device, and the pointers are fake."""
    assert lib.mq_decode_cache_fork(None, None) == 1 and lib.mq_last_error().startswith(b"mq_decode_cache_fork: null argument block")
    for f in ("caches", "pos", "parent"):
        _rejects(lib, _args(**{f: None}), "null pointer")
    for n in (0, -1, 1025):
        _rejects(lib, _args(n_caches=n), f"n_caches={n} outside 1..1024")
    for b in (0, -1, 9):
        _rejects(lib, _args(batch=b), f"batch={b} outside 1..8")
    for h in (0, -3):
        _rejects(lib, _args(kv_heads=h), f"kv_heads={h}")
    for n in (0, -1):
        _rejects(lib, _args(cache_len=n), f"cache_len={n}")
    for d in (0, 8, 15, 17, 24, 72, 250, 257, 272, 512, -16):
        _rejects(lib, _args(head_dim=d), f"head_dim={d} must be a multiple of 16 in [16, 256]")
    _rejects(lib, _args(n_caches=1024, kv_heads=64), "n_caches x kv_heads = 65536")
    _rejects(lib, _args(caches=P + 4), "8-byte")
    _rejects(lib, _args(pos=P + 2), "4-byte aligned")
    _rejects(lib, _args(parent=P + 1), "4-byte aligned")


def test_kernel_has_no_private_segment_and_no_lds(tmp_path):
    """The compiled kernel's metadata: no private segment (nothing spilled or indexed at run time) and no LDS."""
    from mobilequant_amd import build
    flags = [f for f in build.FLAGS if f != "-fPIC"]
    src = "mq_decode_fork.hip"
    asm = str(tmp_path / "mq_decode_fork.s")
    cmd = [build.HIPCC, *flags, *build.PER_FILE_FLAGS.get(src, ()), "-w", "--cuda-device-only", "-S", os.path.join(ROOT, "mobilequant_amd", "csrc", src), "-o", asm]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    text = open(asm).read()
    assert re.search("cache_fork_kernel", text)
    assert re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text) == ["0"] and re.findall(r"\.group_segment_fixed_size:\s*(\d+)", text) == ["0"]


# ---- ops.decode_cache_fork: refusals that need no device ---------------------------------------------------------------------------
def test_op_refuses_before_the_c_call():
    import mobilequant_amd as mq
    assert callable(mq.ops.decode_cache_fork)
    F = mq.ops.decode_cache_fork
    c = torch.zeros(2, 1, 8, 16, dtype=torch.int8)
    i32 = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="at least one cache"):
        F([], i32, i32)
    with pytest.raises(RuntimeError, match="caches are int8"):
        F([c, c.to(torch.uint8)], i32, i32)                            # wrong dtype
    with pytest.raises(RuntimeError, match="caches are int8"):
        F([c.to(torch.float32)], i32, i32)
    with pytest.raises(ValueError, match="different shapes"):
        F([c, torch.zeros(2, 1, 9, 16, dtype=torch.int8)], i32, i32)   # shape mismatch
    with pytest.raises(ValueError, match=r"\[batch, kv_heads, cache_len, head_dim\]"):
        F([c[0]], i32, i32)
    with pytest.raises(RuntimeError, match="not contiguous"):
        F([c, torch.zeros(2, 1, 16, 16, dtype=torch.int8)[:, :, ::2]], i32, i32)
    with pytest.raises(RuntimeError, match="not contiguous"):
        F([torch.zeros(2, 8, 2, 16, dtype=torch.int8).transpose(1, 2)], i32, i32)
    for bad in (i32.to(torch.int64), torch.zeros(3, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)[::2]):
        with pytest.raises(RuntimeError, match=r"pos must be a contiguous int32 \[2\]"):
            F([c], bad, i32)
        with pytest.raises(RuntimeError, match=r"parent must be a contiguous int32 \[2\]"):
            F([c], i32, bad)
    with pytest.raises(ValueError, match="head_dim=24"):
        F([torch.zeros(2, 1, 8, 24, dtype=torch.int8)], i32, i32)
    with pytest.raises(ValueError, match="outside the launch's limits"):
        F([torch.zeros(9, 1, 8, 16, dtype=torch.int8)], torch.zeros(9, dtype=torch.int32), torch.zeros(9, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        F([c], i32, i32)                                               # everything in order but the device: a CPU tensor


def test_torch_library_registration_and_meta_kernel():
    import mobilequant_amd.torch_ops as T
    assert "decode_cache_fork" in T.OPS
    op = torch.ops.mobilequant_amd.decode_cache_fork
    assert op([torch.empty(2, 1, 8, 16, dtype=torch.int8, device="meta")], torch.empty(2, dtype=torch.int32, device="meta"),
              torch.empty(2, dtype=torch.int32, device="meta")) is None
    with pytest.raises(NotImplementedError):                           # no CPU implementation to dispatch to
        op([torch.zeros(2, 1, 8, 16, dtype=torch.int8)], torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32))


# ---- BatchDecodeEngine: argument errors on a bare object -----------------------------------------------------------------------------
def _bare(batch=4, active=(True, False, True, False)):
    from mobilequant_amd.decode_batch import BatchDecodeEngine
    be = object.__new__(BatchDecodeEngine)
    be.batch, be.cache_len = batch, 64
    be._active, be._host_pos = list(active), [10 if a else 64 for a in active]
    return be


@pytest.mark.parametrize("forks,exc,text", [
    ({}, ValueError, "empty mapping"),
    ({0: []}, ValueError, "empty destination list"),
    ({4: [1]}, IndexError, "source slot 4 outside 0..3"),
    ({-1: [1]}, IndexError, "source slot -1 outside"),
    ({0: [4]}, IndexError, "destination slot 4 outside 0..3"),
    ({0: [-1]}, IndexError, "destination slot -1 outside"),
    ({1: [3]}, RuntimeError, "source slot 1 is idle"),
    ({0: [0]}, ValueError, "slot 0 is its own destination"),
    ({0: [1, 1]}, ValueError, "destination slot 1 is named twice"),
    ({0: [1], 2: [3, 1]}, ValueError, "destination slot 1 is named twice"),
    ({0: [2], 2: [3]}, ValueError, "slot 2 is a source and a destination"),
    ({2: [3], 0: [2]}, ValueError, "slot 2 is a source and a destination"),
    ([0, 1], ValueError, "must be a mapping"),
    ({0: 1}, ValueError, "must be a mapping"),
])
def test_fork_refuses_before_anything_is_launched(forks, exc, text):
    """The bare object has no device buffers at all: reaching a launch or a copy would be an AttributeError."""
    from mobilequant_amd.decode_batch import BatchDecodeEngine
    be = _bare()
    with pytest.raises(exc, match=re.escape("BatchDecodeEngine.fork: ")) as e:
        BatchDecodeEngine.fork(be, forks)
    assert text in str(e.value)
    assert be._active == [True, False, True, False] and be._host_pos == [10, 64, 10, 64]


def test_fork_refuses_a_source_whose_cache_is_full():
    """An active slot at position cache_len carries the idle sentinel on the device: the launch would copy nothing, so fork must not
    hand its position, token and logits row to a destination."""
    from mobilequant_amd.decode_batch import BatchDecodeEngine
    be = _bare()
    be._host_pos[0] = be.cache_len
    with pytest.raises(RuntimeError, match=re.escape("BatchDecodeEngine.fork: source slot 0's KV cache is full (64 positions)")):
        BatchDecodeEngine.fork(be, {0: [1]})
    assert be._active == [True, False, True, False] and be._host_pos == [64, 64, 10, 64]
    with pytest.raises(AttributeError):                                # one position short of full passes every check and reaches the device buffers
        be._host_pos[0] = be.cache_len - 1
        BatchDecodeEngine.fork(be, {0: [1]})


def test_generate_n_argument_errors():
    from mobilequant_amd import SamplingParams
    from mobilequant_amd.decode_batch import BatchDecodeEngine
    be = _bare()
    sp = SamplingParams(temperature=0.7, top_k=40)
    draft = lambda ids, k: []      # noqa: E731
    G, S = BatchDecodeEngine.generate, BatchDecodeEngine.generate_speculative
    for bad in (0, -1, 2.0, "2", True, [2]):
        with pytest.raises(ValueError, match="n="):
            G(be, [[1, 2]], 4, sampling=sp, n=bad)
        with pytest.raises(ValueError, match="n="):
            S(be, [[1, 2]], 4, draft, sampling=sp, n=bad)
    with pytest.raises(ValueError, match="needs sampling="):
        G(be, [[1, 2]], 4, n=2)
    with pytest.raises(ValueError, match="needs sampling="):
        G(be, [[1, 2]], 4, do_sample=True, n=2)
    with pytest.raises(ValueError, match="draft"):
        G(be, [[1, 2]], 4, draft=draft, n=2)
    with pytest.raises(ValueError, match="draft"):
        G(be, [[1, 2]], 4, sampling=sp, draft=draft, n=2)
    for prompts, k in (([[1, 2]], 5), ([[1], [2], [3]], 2), ([[1]] * 5, 1), ([], 2)):
        with pytest.raises(ValueError, match="for 4 slots"):
            G(be, prompts, 4, sampling=sp, n=k)
        with pytest.raises(ValueError, match="for 4 slots"):
            S(be, prompts, 4, draft, sampling=sp, n=k)
    with pytest.raises(ValueError, match="1 SamplingParams for 2 prompts"):
        G(be, [[1], [2]], 4, sampling=[sp], n=2)
    with pytest.raises(ValueError, match="4 SamplingParams for 2 prompts"):
        G(be, [[1], [2]], 4, sampling=[sp] * 4, n=2)                  # one request per PROMPT, not per sample
    with pytest.raises(TypeError, match="SamplingParams"):
        G(be, [[1], [2]], 4, sampling=[sp, 3], n=2)
    per_slot = re.escape("4 samples (2 prompts x n=2, one per slot)")
    with pytest.raises(ValueError, match="3 streams for " + per_slot):
        G(be, [[1], [2]], 4, sampling=sp, streams=[1, 2, 3], n=2)     # streams are per slot: len(prompts) * n
    with pytest.raises(ValueError, match="3 streams for " + per_slot):
        S(be, [[1], [2]], 4, draft, sampling=sp, streams=[1, 2, 3], n=2)
    with pytest.raises(ValueError, match="3 drafts for " + per_slot):
        S(be, [[1], [2]], 4, [draft] * 3, sampling=sp, n=2)           # one draft, one per prompt (2) or one per sample (4)
    with pytest.raises(ValueError, match="3 streams for 2 prompts"):  # without n= the wording is the one it always was
        G(be, [[1], [2]], 4, sampling=sp, streams=[1, 2, 3])
    with pytest.raises(ValueError, match="3 drafts for 2 prompts"):
        S(be, [[1], [2]], 4, [draft] * 3, sampling=sp)
    with pytest.raises(ValueError, match="exceeds the cache"):
        G(be, [[1] * 61], 4, sampling=sp, n=2)
    with pytest.raises(ValueError, match="logprobs="):
        G(be, [[1, 2]], 4, sampling=sp, n=2, logprobs=21)
