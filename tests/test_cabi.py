"""The C-ABI library builds for gfx950 (cross-compiled, no GPU needed), loads, and exports exactly the
entry points include/*.h declare (mobilequant_amd.h: the drop-in boundary; mobilequant_amd_tuning.h: profiling knobs).
No compute calls here."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = sorted(os.path.join(ROOT, "include", f) for f in os.listdir(os.path.join(ROOT, "include")) if f.endswith(".h"))


def declared_functions(headers=None):
    found = set()
    for h in headers or HEADERS:
        src = re.sub(r"/\*.*?\*/", "", open(h).read(), flags=re.S)
        found |= set(re.findall(r"\b(mq_[a-z0-9_]+)\s*\(", src))
    return sorted(found)


def test_tuning_knobs_are_not_part_of_the_boundary_header():
    boundary = declared_functions([os.path.join(ROOT, "include", "mobilequant_amd.h")])
    assert not any(n.startswith("mq_gemm_set_") or n == "mq_gemm_variant_name" for n in boundary)
    assert "mq_w8a8_linear" in boundary and "mq_minmax_tensor" in boundary


@pytest.fixture(scope="module")
def lib_path():
    from mobilequant_amd import build
    return build.build()          # no-op when the in-tree library is newer than its sources


def test_header_and_binding_agree():
    from mobilequant_amd import _lib
    assert declared_functions() == sorted(_lib.EXPORTED_SYMBOLS)


def test_library_exports_every_declared_symbol(lib_path):
    lib = ctypes.CDLL(lib_path)
    for name in declared_functions():
        assert hasattr(lib, name), name
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (mq_[a-z0-9_]+)$", out, flags=re.M))
    assert exported == set(declared_functions())       # nothing undeclared leaks out either


def test_library_contains_gfx950_code_only(lib_path):
    out = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", lib_path], capture_output=True, text=True).stdout
    blob = open(lib_path, "rb").read()
    assert b"gfx950" in blob and b"gfx942" not in blob and b"gfx90a" not in blob, out[:200]


def test_binding_loads_and_reports_errors_without_a_gpu(lib_path):
    from mobilequant_amd import _lib
    lib = _lib.load()
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mobilequant_amd.h")).read()
    ver = int(re.search(r"#define MQ_VERSION (\d+)", hdr).group(1))
    assert lib.mq_version() == ver and ver // 100 == _lib.HEADER_MAJOR      # the ctypes structs mirror this major
    nvar = lib.mq_gemm_set_variant(-1)
    assert nvar >= 4 and lib.mq_gemm_variant_name(0).decode().startswith("t")
    # argument validation happens before any HIP call: null pointers -> MQ_EINVAL + a message, no crash
    rc = lib.mq_fake_quant(None, None, 0, 4, 4, None, None, 1, 0.0, 255.0, None)
    assert rc == 1 and b"null pointer" in lib.mq_last_error()
    with pytest.raises(_lib.MobileQuantLibraryError, match="K=100"):
        _lib.call("mq_w8a8_linear", 16, 16, 4, 8, 100, None, 16, 16, 16, None, None, None, 0.0, 0.0, 16, 0, None)


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from mobilequant_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_lib.MobileQuantLibraryError, match="no CPU or PyTorch fallback"):
        _lib.load()


def test_generated_isa_is_current(tmp_path):
    """csrc/mq_gemm_pp_asm.inc is generated (tools/gen_pp_asm.py) and committed: regenerating must reproduce it."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    inc = os.path.join(root, "mobilequant_amd", "csrc", "mq_gemm_pp_asm.inc")
    spec = importlib.util.spec_from_file_location("gen_pp_asm", os.path.join(root, "tools", "gen_pp_asm.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    fresh = str(tmp_path / "fresh.inc")
    mod.main(fresh)
    assert open(fresh).read() == open(inc).read()


def test_generated_free_running_kernel_is_current(tmp_path):
    """csrc/mq_gemm_fr_asm.inc (tools/gen_fr_asm.py: the whole-kernel ISA of GEMM variant 11) is committed: regenerating must
    reproduce it, and the generator's VMEM-queue simulation must hold (it asserts the loop body is a fixed point)."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    inc = os.path.join(root, "mobilequant_amd", "csrc", "mq_gemm_fr_asm.inc")
    spec = importlib.util.spec_from_file_location("gen_fr_asm", os.path.join(root, "tools", "gen_fr_asm.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    fresh = str(tmp_path / "fresh.inc")
    mod.main(fresh)
    assert open(fresh).read() == open(inc).read()
    # the 128-column variants of the same generator (q | k | v; o_proj / w2 with the residual add)
    for variant, (_, _, _, _, fname) in mod.VARIANTS.items():
        if variant in mod.EXPERIMENTAL:            # not committed: generated on demand by `build --experiments`
            assert not os.path.exists(os.path.join(root, "mobilequant_amd", "csrc", fname)), fname + " is an experiment-only file: do not commit it"
            continue
        fresh = str(tmp_path / ("fresh_" + variant + ".inc"))
        mod.main(fresh, variant=variant)
        assert open(fresh).read() == open(os.path.join(root, "mobilequant_amd", "csrc", fname)).read(), variant


def test_argument_checks_fail_before_any_launch():
    """Bad shapes are rejected by the entry points themselves (MQ_EINVAL / MQ_EUNSUPPORTED + mq_last_error), before any
    HIP call: checkable without a GPU.  Pointers are fake, aligned and never dereferenced."""
    import ctypes
    from mobilequant_amd import _lib as L
    lib = L.load()
    p = ctypes.c_void_p(0x10000)
    # cols must be a multiple of 128 for the fragment-blocked layout
    assert lib.mq_quantize_tiled(p, L.MQ_F32, 32, 100, p, p, 0.0, 255.0, 128, None, p, None, None) == 1
    assert b"multiple of 128" in lib.mq_last_error()
    # fused norm: cols % 4, integer output without an output grid
    assert lib.mq_rmsnorm_quant(p, 4, 30, p, None, 1e-5, None, None, 0.0, 0.0, None, None, 0.0, 0.0, p, None, None, 0, None, None) == 1
    assert lib.mq_rmsnorm_quant(p, 4, 32, p, None, 1e-5, None, None, 0.0, 0.0, None, None, 0.0, 0.0, None, p, None, 0, None, None) == 1
    assert b"output quantizer" in lib.mq_last_error()
    # activation kernel: unknown activation code
    assert lib.mq_act_quant(p, 16, 7, None, None, 0.0, 0.0, None, None, 0.0, 0.0, None, None, 0.0, 0.0, p, None) == 1
    # shapes the fragment-blocked GEMM path does not serve
    assert lib.mq_gemm_tiled_supported(2048, 5632, 2048) == 1 and lib.mq_gemm_tiled_supported(2048, 2048, 2048) == 0
    assert lib.mq_w8a8_linear_tiled(p, p, 2048, 2048, 2048, None, p, p, p, None, None, None, 0.0, 0.0, p, L.MQ_F32, None) == 3
    assert b"mq_gemm_tiled_supported" in lib.mq_last_error()
    # fresh min/max needs its scratch
    assert lib.mq_minmax_tensor_fresh(p, L.MQ_F32, 100, p, p, p, 10, None) == 1
    # round 4: the training-step passes -- row lengths, bit widths, mask periodicity; empty tensors are a no-op
    assert lib.mq_lwc_fake_quant(p, 8, 30, p, p, 4, 0, p, p, p, p, p, None) == 1 and b"multiple of 4" in lib.mq_last_error()
    assert lib.mq_lwc_fake_quant(p, 8, 32768, p, p, 4, 0, p, p, p, p, p, None) == 1
    assert lib.mq_lwc_fake_quant(p, 8, 64, p, p, 17, 0, p, p, p, p, p, None) == 1 and b"bitwidth" in lib.mq_last_error()
    assert lib.mq_lwc_fake_quant(None, 0, 64, None, None, 4, 0, None, None, None, None, None, None) == 0
    assert lib.mq_lwc_fake_quant_backward(p, p, 8, 64, p, p, p, p, 4, 0, p, p, None, None) == 1 and b"null pointer" in lib.mq_last_error()
    assert lib.mq_attention_probs_train(p, 64, 8192, None, 1, p, p, 0.0, 65535.0, p, p, 0.0, 65535.0, 8.0, p, None) == 1
    assert b"4096 columns" in lib.mq_last_error()
    assert lib.mq_attention_probs_train(p, 64, 128, p, 48, p, p, 0.0, 65535.0, p, p, 0.0, 65535.0, 8.0, p, None) == 1
    assert b"mask_rows" in lib.mq_last_error()
    assert lib.mq_attention_probs_train(p, 64, 128, None, 1, p, p, 0.0, 65535.0, p, p, 0.0, 65535.0, 0.0, p, None) == 1
    assert lib.mq_attention_probs_train_backward(p, p, 0, 128, None, 1, p, p, 0.0, 65535.0, p, p, 0.0, 65535.0, 8.0, None, None, None) == 0
    assert lib.mq_attention_probs_train_backward(p, p, 64, 128, None, 1, p, p, 0.0, 65535.0, p, p, 0.0, 65535.0, 8.0, p, None, None) == 1
    # per-group weight grids: group size, N
    assert lib.mq_w8a8_linear_grouped(p, p, 64, 128, 1024, 100, p, p, p, p, None, p, None) == 1 and b"group_size" in lib.mq_last_error()
    assert lib.mq_w8a8_linear_grouped(p, p, 64, 100, 1024, 128, p, p, p, p, None, p, None) == 1 and b"multiple of 128" in lib.mq_last_error()
    assert lib.mq_w8a8_linear_grouped(p, p, 0, 128, 1024, 128, None, None, None, None, None, None, None) == 0
    assert lib.mq_w4a8_linear_tiled_residual(p, p, 2048, 2048, 2048, None, p, p, p, None, p, p, 0.0, 255.0, p, p, None) == 1 and b"16-bit output grid" in lib.mq_last_error()
    assert lib.mq_w4a8_linear_tiled_residual(p, p, 2048, 2000, 2048, None, p, p, p, None, p, p, 0.0, 65535.0, p, p, None) == 3
    assert lib.mq_w4a8_linear_tiled_gated(p, 2048, 2000, 2048, None, p, p, p, p, None, p, p, p, p, p, p, None, p, p, p, p, p, p, None) == 3


def test_no_barrier_with_lds_traffic_in_flight(tmp_path):
    """Round 6: hipcc (ROCm 7.2) put the release fence's `s_waitcnt lgkmcnt(0)` BEHIND an s_barrier that opens a loop header whose latch
    ends in LDS writes (mq_qmatmul's row-panel kernel, element-load variants): another wave read the x2 tile before the last dword had
    landed (tests/fuzz_qmatmul.py case 85, one run in five).  The kernel now waits explicitly; tools/barrier_audit.py walks every
    s_barrier of a compiled file backwards through the control-flow graph and must find no path with an LDS operation in flight.
    Audited here: every source whose barriers are the compiler's (mq_gemm.hip and mq_attention.hip place theirs, and the waits in front
    of them, by hand in inline assembly; mq_fake_quant.hip and mq_quantize.hip -- block reductions only -- are left to the tool by hand: 80 s to compile)."""
    import sys
    from mobilequant_amd import build
    flags = [f for f in build.FLAGS if f != "-fPIC"]
    procs = []
    for src in ("mq_qmatmul.hip", "mq_decode.hip", "mq_norm.hip", "mq_activation.hip", "mq_gemv.hip", "mq_reduce.hip", "mq_gemm_grouped.hip"):
        asm = str(tmp_path / src.replace(".hip", ".s"))
        cmd = [build.HIPCC, *flags, *build.PER_FILE_FLAGS.get(src, ()), "-w", "--cuda-device-only", "-S", os.path.join(ROOT, "mobilequant_amd", "csrc", src), "-o", asm]
        procs.append((asm, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for asm, p in procs:
        out, _ = p.communicate()
        assert p.returncode == 0, out[-2000:]
        rep = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "barrier_audit.py"), asm], stdout=subprocess.PIPE, text=True).stdout
        assert "PENDING" not in rep and "possibly in flight 0" in rep, rep


def test_tiled_gemm_refusals_keep_their_text():
    """The residual pair, the gated pair and the three segmented entry points share one body / one segment check each (mq_gemm.hip): every
    refusal keeps its return code and the text it had when each entry point carried its own copy.  No HIP call is reached."""
    import ctypes
    from mobilequant_amd import _lib as L
    lib = L.load()
    p = ctypes.c_void_p(0x10000)

    def grids(qmax=(255.0, 255.0, 255.0)):
        g = (L.MqGrid * 3)()
        for i in range(3):
            g[i].scale, g[i].offset, g[i].qmin, g[i].qmax = 0x10000, 0x10000, 0.0, qmax[i]
        return g

    def ends(*v):
        return (ctypes.c_int64 * 3)(*v)

    def err():
        return lib.mq_last_error().decode()

    seg = {"mq_w8a8_linear_segmented": lambda n, e, g, N=2560: lib.mq_w8a8_linear_segmented(p, p, 2048, N, 2048, None, p, p, p, None, n, e, g, p, None),
           "mq_w4a8_linear_segmented": lambda n, e, g, N=2560: lib.mq_w4a8_linear_segmented(p, p, 2048, N, 2048, None, p, p, p, None, n, e, g, p, None),
           "mq_w8a8_linear_tiled_segmented": lambda n, e, g, N=2560: lib.mq_w8a8_linear_tiled_segmented(p, p, 2048, N, 2048, None, p, p, p, None, n, e, g, p, None),
           "mq_w4a8_linear_tiled": lambda n, e, g, N=2560: lib.mq_w4a8_linear_tiled(p, p, 2048, N, 2048, None, p, p, p, None, n, e, g, p, L.MQ_U8, None)}
    for fn, call in seg.items():
        assert call(0, ends(2560), grids()) == 1 and err() == fn + ": 1..3 segments"
        assert call(3, ends(2048, 2304, 2560), grids((255.0, 65535.0, 255.0))) == 1 and err() == fn + ": segment 1 needs an 8-bit unsigned output grid"
        assert call(3, ends(2048, 2048, 2560), grids()) == 1 and err() == fn + ": segment ends must increase, be multiples of 4, <= N"
        assert call(3, ends(2048, 2304, 2432), grids()) == 1 and err() == fn + ": the last segment must end at N"
    # a single segment of the packed tiled entry point comes without ends; the others insist on them
    assert lib.mq_w4a8_linear_tiled(p, p, 2048, 2000, 2048, None, p, p, p, None, 1, None, grids(), p, L.MQ_U8, None) == 3
    assert err() == ("mq_w4a8_linear_tiled: shape 2048x2000x2048 is not served (mq_gemm_tiled_w4_supported: N % 176 == 0 or N % 128 == 0 "
                     "(segments: 128), K % 256 == 0, K >= 768)")
    assert seg["mq_w8a8_linear_tiled_segmented"](1, None, grids()) == 1 and err() == "mq_w8a8_linear_tiled_segmented: 1..3 segments"
    assert seg["mq_w8a8_linear_tiled_segmented"](1, ends(2000), grids(), 2000) == 3
    assert err() == "mq_w8a8_linear_tiled_segmented: shape 2048x2000x2048 is not served (mq_gemm_tiled128_supported: N % 128 == 0, K % 256 == 0, K >= 768)"

    # residual pair: one body, the 8-bit hint in the int8 entry point's message only
    for fn, hint in (("mq_w8a8_linear_tiled_residual", " (8-bit grids: mq_w8a8_linear_residual)"), ("mq_w4a8_linear_tiled_residual", "")):
        f = getattr(lib, fn)
        assert f(p, p, 2048, 2048, 2048, None, p, p, p, None, p, p, 0.0, 65535.0, None, p, None) == 1
        assert err() == fn + ": resid must be non-null and 16-byte aligned"
        assert f(p, p, 2048, 2048, 2048, None, p, p, p, None, p, p, 0.0, 255.0, p, p, None) == 1
        assert err() == fn + ": a 16-bit output grid is required" + hint
        assert f(p, p, 2048, 2000, 2048, None, p, p, p, None, p, p, 0.0, 65535.0, p, p, None) == 3
        assert err() == fn + ": shape 2048x2000x2048 is not served (mq_gemm_tiled128_supported: N % 128 == 0, K % 256 == 0, K >= 768)"

    # gated pair: one body, each entry point's own "not served" text
    served = {"mq_w8a8_linear_tiled_gated": "mq_gemm_tiled_supported or N % 128 == 0 with >= 192 tiles; K % 256 == 0, K >= 768",
              "mq_w4a8_linear_tiled_gated": "as mq_w8a8_linear_tiled_gated"}
    for fn, why in served.items():
        f = getattr(lib, fn)
        assert f(p, 2048, 5632, 2048, None, p, p, p, p, None, p, p, p, p, p, p, None, p, p, None, p, p, p, None) == 1
        assert err() == fn + ": both linears carry an 8-bit unsigned output grid; table / scratch / image must be non-null and 16-byte aligned"
        assert f(p, 2048, 2000, 2048, None, p, p, p, p, None, p, p, p, p, p, p, None, p, p, p, p, p, p, None) == 3
        assert err() == fn + ": shape 2048x2000x2048 is not served (" + why + ")"
    # the pair launch of the same family
    assert lib.mq_w8a8_linear_tiled_pair(p, 2048, 2048, 2048, None, p, p, p, p, None, p, p, p, p, p, p, p, None, p, p, p, L.MQ_U8, None) == 3
    assert err() == "mq_w8a8_linear_tiled_pair: shape 2048x2048x2048 is not served (mq_gemm_tiled_supported, K % 256 == 0, K >= 768)"
