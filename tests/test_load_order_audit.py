"""tools/load_order_audit.py on the device assembly of csrc/mq_quantize.hip: in every quantize_tiled8_kernel instantiation the
full-workgroup path requests all 2 V vectors of x before its first vmcnt wait, that wait is a counted one, the grid values' wait
stands behind the last request, and no kernel argument is read behind a vector load (DESIGN 4.1 "request order").  The audit is also
held to hand-written listings of the three patterns it exists to catch."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _audit():
    spec = importlib.util.spec_from_file_location("load_order_audit", os.path.join(ROOT, "tools", "load_order_audit.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_staged_quantize_instantiation_requests_before_it_waits(tmp_path):
    from mobilequant_amd import build
    if not os.path.exists(build.HIPCC):
        pytest.skip("no hipcc on this machine")
    import subprocess
    flags = [f for f in build.FLAGS if f != "-fPIC"] + list(build.PER_FILE_FLAGS.get("mq_quantize.hip", ()))
    asm = str(tmp_path / "mq_quantize.s")
    r = subprocess.run([build.HIPCC, *flags, "-w", "--cuda-device-only", "-S", os.path.join(ROOT, "mobilequant_amd", "csrc", "mq_quantize.hip"),
                        "-o", asm], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    count, report = _audit().audit(asm)
    assert count == 16, count                       # V = 1 .. 4, with and without row sums, four and eight rows per workgroup
    assert report == [], "\n".join(report)


GOOD = """_ZN2mq22quantize_tiled8_kernelILi2ELb1ELi2EEEvPKfPallS2_S2_ffiPi:
	s_load_dwordx8 s[4:11], s[0:1], 0x0
	s_load_dwordx2 s[20:21], s[0:1], 0x40
	s_waitcnt lgkmcnt(0)
	s_load_dword s24, s[12:13], 0x0
	s_cbranch_vccnz .LBB0_2
	; mq-full-path-begin
	global_load_dwordx4 v[18:21], v10, s[14:15]
	global_load_dwordx4 v[28:31], v10, s[18:19]
	global_load_dwordx4 v[6:9], v10, s[14:15]
	global_load_dwordx4 v[2:5], v10, s[0:1]
	s_waitcnt lgkmcnt(0)
	s_waitcnt vmcnt(3)
	s_waitcnt vmcnt(0)
	; mq-full-path-end
.LBB0_2:
	s_barrier
	global_store_dwordx4 v[4:5], v[0:3], off
	s_endpgm
.Lfunc_end0:
"""


@pytest.mark.parametrize("kind, old, new", [
    (None, "", ""),
    # the fourth load sunk behind the grid values' wait, the first conversion behind all four
    ("LOADS", "\tglobal_load_dwordx4 v[2:5], v10, s[0:1]\n\ts_waitcnt lgkmcnt(0)\n\ts_waitcnt vmcnt(3)\n",
     "\ts_waitcnt lgkmcnt(0)\n\ts_waitcnt vmcnt(2)\n\tglobal_load_dwordx4 v[2:5], v10, s[0:1]\n"),
    ("WAIT", "s_waitcnt vmcnt(3)", "s_waitcnt vmcnt(0)"),
    ("GRID", "\tglobal_load_dwordx4 v[28:31], v10, s[18:19]\n", "\tglobal_load_dwordx4 v[28:31], v10, s[18:19]\n\ts_waitcnt lgkmcnt(0)\n"),
    # a pointer argument read in the tail, behind the barrier
    ("KERNARG", "\ts_barrier\n", "\ts_barrier\n\ts_load_dwordx2 s[6:7], s[0:1], 0x8\n"),
    ("LOADS", "\t; mq-full-path-begin\n", ""),
])
def test_the_audit_reports_the_patterns_it_is_for(tmp_path, kind, old, new):
    text = GOOD.replace(old, new) if old else GOOD
    assert old == "" or text != GOOD
    p = tmp_path / "k.s"
    p.write_text(text)
    count, report = _audit().audit(str(p))
    assert count == 1
    if kind is None:
        assert report == [], report
    else:
        assert report and any(" %s " % kind in line for line in report), report
