"""The grouped decode GEMV entry without a GPU: the library exports it, the ctypes block mirrors the header, argument blocks outside
its limits are refused with MQ_EINVAL / MQ_EUNSUPPORTED and a message before any HIP call, and the barriers of mq_decode_grouped.hip
have no LDS traffic in flight.  Pointers are fake, aligned and never dereferenced."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x10000          # a fake, 16-byte aligned device address


@pytest.fixture(scope="module")
def lib():
    from mobilequant_amd import _lib, build
    build.build()
    return _lib.load()


def _args(batch=2, K=2048, N=256, gs=128, **kw):
    from mobilequant_amd._lib import MqDecodeGemvArgs, MqDecodeGemvBatchArgs, MqDecodeGemvGroupedArgs, MqGrid
    g = MqDecodeGemvArgs()
    g.x, g.K, g.N, g.norm_w = P, K, N, P
    g.a_grid, g.norm_in = MqGrid(P, P, 0.0, 255.0), MqGrid(P, P, 0.0, 65535.0)
    g.w, g.y, g.consts = P, P, P
    g.seg_end[0] = g.seg_end[1] = N
    a = MqDecodeGemvGroupedArgs()
    a.group_size, a.alpha, a.cw, a.t = gs, P, P, P
    for k, v in kw.items():
        setattr(a if k in ("group_size", "alpha", "cw", "t") else g, k, v)
    b = MqDecodeGemvBatchArgs()
    b.g, b.batch, b.x_stride, b.y_stride, b.gate_stride = g, batch, K, N, 0
    a.b = b
    return a


def _rejects(lib, args, text, rc=1):
    got = lib.mq_decode_gemv_grouped(ctypes.byref(args), None)
    msg = lib.mq_last_error()
    assert got == rc, (got, msg)
    assert text.encode() in msg, msg


def test_entry_and_struct_layout(lib):
    from mobilequant_amd._lib import MqDecodeGemvBatchArgs, MqDecodeGemvGroupedArgs
    assert hasattr(lib, "mq_decode_gemv_grouped")
    assert lib.mq_version() == 304
    src = "\n".join([
        "#include <stddef.h>", "#include <stdio.h>", '#include "mobilequant_amd.h"', "int main(void) {",
        '  printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(mq_decode_gemv_grouped_args), offsetof(mq_decode_gemv_grouped_args, b),',
        "         offsetof(mq_decode_gemv_grouped_args, group_size), offsetof(mq_decode_gemv_grouped_args, alpha),",
        "         offsetof(mq_decode_gemv_grouped_args, cw), offsetof(mq_decode_gemv_grouped_args, t));", "  return 0;", "}"])
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        open(c, "w").write(src)
        cc = next((x for x in ("cc", "gcc", "clang") if subprocess.run(["which", x], stdout=subprocess.PIPE).returncode == 0), None)
        if cc is None:
            cc = "/opt/rocm/llvm/bin/clang"
        subprocess.run([cc, "-I" + os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    F = MqDecodeGemvGroupedArgs
    assert got == [ctypes.sizeof(F), F.b.offset, F.group_size.offset, F.alpha.offset, F.cw.offset, F.t.offset]
    assert F.group_size.offset == ctypes.sizeof(MqDecodeGemvBatchArgs)


def test_rejects_bad_argument_blocks(lib):
    assert lib.mq_decode_gemv_grouped(None, None) == 1 and b"null argument block" in lib.mq_last_error()
    for k in ("alpha", "cw", "t", "w"):
        _rejects(lib, _args(**{k: None}), "null pointer")
    _rejects(lib, _args(consts=None), "consts")
    for b in (0, 9):
        _rejects(lib, _args(batch=b), "outside 1..8")
    for gs in (0, 32, 100, -64):
        _rejects(lib, _args(gs=gs), f"group_size={gs} must be a multiple of 64")
    _rejects(lib, _args(K=2304, gs=1024), "divides K")
    _rejects(lib, _args(K=2304, gs=192), "not a power of two", rc=3)                  # MQ_EUNSUPPORTED
    _rejects(lib, _args(batch=8, K=32768, gs=128, x=None, xq=P, norm_w=None), "exceeds the 131072 bytes")
    _rejects(lib, _args(batch=5, K=32768, gs=128, x=None, xq=P, norm_w=None), "exceeds the 131072 bytes")
    _rejects(lib, _args(alpha=P + 4), "16-byte aligned")
    _rejects(lib, _args(zero_acc=P, zero_n=4), "zero_acc / o_acc")
    _rejects(lib, _args(K=1000), "multiple of 256")


def test_barriers_have_no_lds_operation_in_flight(tmp_path):
    """tools/barrier_audit.py (tests/test_cabi.py) on mq_decode_grouped.hip: no s_barrier with an LDS operation possibly in flight."""
    from mobilequant_amd import build
    flags = [f for f in build.FLAGS if f != "-fPIC"]
    src = "mq_decode_grouped.hip"
    asm = str(tmp_path / "mq_decode_grouped.s")
    cmd = [build.HIPCC, *flags, *build.PER_FILE_FLAGS.get(src, ()), "-w", "--cuda-device-only", "-S", os.path.join(ROOT, "mobilequant_amd", "csrc", src), "-o", asm]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    rep = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "barrier_audit.py"), asm], stdout=subprocess.PIPE, text=True).stdout
    assert "PENDING" not in rep and "possibly in flight 0" in rep, rep
    assert re.search(r"decode_gemv_grouped_kernel", open(asm).read())
