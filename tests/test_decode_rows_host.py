"""mq_decode_rows.hip without a GPU: the one kernel behind mq_decode_attention_multi and mq_decode_attention_ragged compiles for gfx950,
none of its barriers has LDS traffic in flight, and every instantiation is built.  (The entries' argument checks:
tests/test_decode_multi_host.py, tests/test_decode_ragged_host.py.)"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_no_barrier_with_lds_traffic_in_flight(tmp_path):
    """tools/barrier_audit.py (tests/test_cabi.py) on mq_decode_rows.hip, the one kernel behind mq_decode_attention_multi and
    mq_decode_attention_ragged: no s_barrier with an LDS operation possibly in flight, and every instantiation is there -- head_dim
    32 / 64 / 128 / 256 x flat / chunked values without a row table, head_dim x flat values with one."""
    from mobilequant_amd import build
    flags = [f for f in build.FLAGS if f != "-fPIC"]
    src = "mq_decode_rows.hip"
    assert src in build.SOURCES
    asm = str(tmp_path / "mq_decode_rows.s")
    cmd = [build.HIPCC, *flags, *build.PER_FILE_FLAGS.get(src, ()), "-w", "--cuda-device-only", "-S", os.path.join(ROOT, "mobilequant_amd", "csrc", src), "-o", asm]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    rep = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "barrier_audit.py"), asm], stdout=subprocess.PIPE, text=True).stdout
    assert "PENDING" not in rep and "possibly in flight 0" in rep, rep
    # (Itanium mangling of decode_attention_rows_kernel<D, VCH, TABLE>: ILi<D>ELb<VCH>ELb<TABLE>EE)
    kernels = re.findall(r"^\s*\.amdhsa_kernel \w*decode_attention_rows_kernelILi(\d+)ELb([01])ELb([01])EE", open(asm).read(), re.M)
    assert len(kernels) == len(set(kernels)) == 12, kernels
    assert sorted(k for k in kernels if k[2] == "0") == sorted((str(d), v, "0") for d in (32, 64, 128, 256) for v in "01")
    assert sorted(k for k in kernels if k[2] == "1") == sorted((str(d), "0", "1") for d in (32, 64, 128, 256))
