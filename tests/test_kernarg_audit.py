"""tools/kernarg_audit.py on the device assembly of csrc/mq_quantize.hip and csrc/mq_gemm.hip, compiled with the flags the library
ships with: every quantize_tiled8_kernel instantiation gets its whole parameter list preloaded and reads nothing from the
kernel-argument segment behind the compiler's entry block; gemm_i8_fr_kernel gets its leading scalars preloaded and waits once, behind
the tile map, for the trailing struct before its first vector request (DESIGN 4.1 / 4.2 "kernel arguments").  The audit is also held
to hand-written listings: a good one, a late kernel-argument read, a missing preload."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _audit():
    spec = importlib.util.spec_from_file_location("kernarg_audit", os.path.join(ROOT, "tools", "kernarg_audit.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("src, kernels", [("mq_quantize.hip", 16), ("mq_gemm.hip", 1)])
def test_the_shipped_kernels_take_their_arguments_from_registers(tmp_path, src, kernels):
    from mobilequant_amd import build
    if not os.path.exists(build.HIPCC):
        pytest.skip("no hipcc on this machine")
    import subprocess
    flags = [f for f in build.FLAGS if f != "-fPIC"] + list(build.PER_FILE_FLAGS.get(src, ()))
    asm = str(tmp_path / src.replace(".hip", ".s"))
    r = subprocess.run([build.HIPCC, *flags, "-w", "--cuda-device-only", "-S", os.path.join(ROOT, "mobilequant_amd", "csrc", src), "-o", asm],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    count, report = _audit().audit(asm)
    assert count == kernels, count
    assert report == [], "\n".join(report)


QNAME = "_ZN2mq22quantize_tiled8_kernelILi2ELb1ELi2EEEvPKfPaS2_S2_Piiiff"
GNAME = "_ZN2mq17gemm_i8_fr_kernelEPKaPKviiiiiPKfS5_NS_8GemmArgsE"
FILLER = "\ts_add_i32 s40, s40, 1\n" * 40        # the tile map's scalar arithmetic
GOOD = """%(q)s:
	s_load_dwordx2 s[2:3], s[0:1], 0x0
	s_load_dwordx8 s[4:11], s[0:1], 0x8
	s_load_dwordx4 s[12:15], s[0:1], 0x28
	s_waitcnt lgkmcnt(0)
	s_branch .LBB0_0
	.p2align	8
.LBB0_0:
	s_load_dword s20, s[6:7], 0x0
	s_load_dword s18, s[8:9], 0x0
	global_load_dwordx4 v[20:23], v11, s[2:3]
	s_waitcnt lgkmcnt(0)
	s_waitcnt vmcnt(0)
	s_barrier
	global_store_dwordx4 v[4:5], v[0:3], off
	s_endpgm
.Lfunc_end0:
	.amdhsa_kernel %(q)s
		.amdhsa_kernarg_size 56
		.amdhsa_user_sgpr_kernarg_preload_length 14
	.end_amdhsa_kernel
%(g)s:
	s_load_dwordx2 s[2:3], s[0:1], 0x0
	s_load_dwordx8 s[4:11], s[0:1], 0x8
	s_load_dwordx4 s[12:15], s[0:1], 0x28
	s_waitcnt lgkmcnt(0)
	s_branch .LBB1_0
	.p2align	8
.LBB1_0:
	s_load_dwordx8 s[20:27], s[0:1], 0x58
	s_load_dwordx2 s[34:35], s[0:1], 0x78
%(filler)s	s_waitcnt lgkmcnt(0)
	s_add_u32 s22, s22, s40
	;;#ASMSTART
	s_load_dword s96, s[12:13], 0x0
	global_load_dword v103, v89, s[20:21]
	s_waitcnt lgkmcnt(0)
	;;#ASMEND
	s_endpgm
.Lfunc_end1:
	.amdhsa_kernel %(g)s
		.amdhsa_kernarg_size 296
		.amdhsa_user_sgpr_kernarg_preload_length 14
	.end_amdhsa_kernel
amdhsa.kernels:
  - .agpr_count:     0
    .args:
      - .address_space:  global
        .offset:         0
        .size:           8
        .value_kind:     global_buffer
      - .offset:         48
        .size:           4
        .value_kind:     by_value
      - .offset:         52
        .size:           4
        .value_kind:     by_value
    .group_segment_fixed_size: 64
    .name:           %(q)s
    .symbol:         %(q)s.kd
  - .agpr_count:     128
    .args:
      - .address_space:  global
        .offset:         0
        .size:           8
        .value_kind:     global_buffer
      - .offset:         32
        .size:           4
        .value_kind:     by_value
      - .address_space:  global
        .offset:         48
        .size:           8
        .value_kind:     global_buffer
      - .offset:         56
        .size:           240
        .value_kind:     by_value
      - .offset:         296
        .size:           4
        .value_kind:     hidden_block_count_x
    .group_segment_fixed_size: 0
    .name:           %(g)s
    .symbol:         %(g)s.kd
""" % {"q": QNAME, "g": GNAME, "filler": FILLER}


@pytest.mark.parametrize("kind, old, new", [
    (None, "", ""),
    # late kernel-argument reads: the quantize's row-sum pointer read in the tail, behind the barrier
    ("KERNARG", "\ts_barrier\n", "\ts_barrier\n\ts_load_dwordx2 s[6:7], s[0:1], 0x20\n"),
    # ... the GEMM's trailing struct waited for in front of the tile map, a late field behind it with a wait of its own
    ("WAIT", "\ts_load_dwordx2 s[34:35], s[0:1], 0x78\n", "\ts_load_dwordx2 s[34:35], s[0:1], 0x78\n\ts_waitcnt lgkmcnt(0)\n"),
    ("WAIT", "\ts_add_u32 s22, s22, s40\n", "\ts_add_u32 s22, s22, s40\n\ts_load_dword s3, s[0:1], 0x7c\n\ts_waitcnt lgkmcnt(0)\n"),
    ("WAIT", FILLER, ""),
    # missing preload: no flag (length 0), a parameter list longer than what is preloaded, a struct in front
    ("PRELOAD", "preload_length 14\n\t.end_amdhsa_kernel\n%s:" % GNAME, "preload_length 0\n\t.end_amdhsa_kernel\n%s:" % GNAME),
    ("PRELOAD", "      - .offset:         52\n", "      - .offset:         56\n"),
    ("PRELOAD", "preload_length 14\n\t.end_amdhsa_kernel\namdhsa", "preload_length 12\n\t.end_amdhsa_kernel\namdhsa"),
])
def test_the_audit_reports_the_patterns_it_is_for(tmp_path, kind, old, new):
    text = GOOD.replace(old, new) if old else GOOD
    assert old == "" or text != GOOD
    p = tmp_path / "k.s"
    p.write_text(text)
    count, report = _audit().audit(str(p))
    assert count == 2
    if kind is None:
        assert report == [], report
    else:
        assert report and all(" %s " % kind in line for line in report), report
