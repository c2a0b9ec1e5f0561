"""GPU: mq_w4a16_linear (csrc/mq_w4a16.hip) at every branch of its launch arithmetic and of the GEMV's streaming loop, against the numpy
oracle tests/w4a16_ref.py.  The cases and the mirror of the launch arithmetic that says which branch each one takes live in
tests/w4a16_cases.py (checked on the host by tests/test_w4a16_oracle.py); tests/test_gpu_w4a16.py holds the tests of the feature itself.

- the exact table: bit-equal to the float64 oracle (more than one row slot per wave, more than one chunk pass per row, a second
  issue_pass, dynamic LDS up to the 128 KB limit and the M <= 8 shapes just past it on the GEMM, the 1024-row cap, division-arm group
  sizes, every MT instantiation, zero points at +-1024); every output sits between a guard row in front and a guard row and 64 elements
  behind, which must come back untouched;
- the fp16 output's final rounding at 65504, 65520 (-> inf), the subnormals and the ties at 2^-25, on both kernels;
- Gaussian cases inside the project's derived bound R.bound at the long-K and many-row shapes;
- in fresh child processes: the > 32 KB forms before and after small ones, and graph capture of the wrapper with no earlier call;
- weight_only.w4a16_linear / w4a16_pack refuse malformed operands before anything is launched, and convert the rest.

Measured wall time of the whole file on an MI355X: 11.1 s for its 43 tests (the two tests with child processes 4.7 s and 2.3 s, which is
the children's torch import; the largest cases -- slotsxpasses, slotsxpasses-m2, cap -- 0.3 to 0.4 s each; everything else under 0.3 s)."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(1, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import w4a16_cases as C  # noqa: E402
from test_gpu_w4a16 import assert_bits, bits, check_bound  # noqa: E402
from w4a16_child import _t  # noqa: E402

pytestmark = pytest.mark.gpu

F16, F32 = np.float16, np.float32
TESTS = os.path.dirname(os.path.abspath(__file__))
IDS = [c.id for c in C.exact_cases(256)]                     # (the ids do not depend on the CU count, the shapes do)
GUARD_BYTE = 0x55


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cus(dev):
    return torch.cuda.get_device_properties(0).multi_processor_count


class Weights:
    """The packed weight, its grid and the bias on the device, uploaded once per case."""

    def __init__(self, dev, packed, s16, z16, bias, g):
        self.dev, self.N, self.K, self.g = dev, packed.shape[0], packed.shape[1] * 2, g
        self.qw, self.s, self.z, self.b = _t(packed, dev), _t(s16, dev), _t(z16, dev), _t(bias, dev)

    def launch(self, x, bias, out_dtype, what):
        """mq_w4a16_linear through the C entry itself, as test_gpu_w4a16.launch does, into a NaN-filled output with a guard row in front
        and a guard row and 64 elements behind it: returns the output after asserting that the guards kept their bytes."""
        import ctypes

        from mobilequant_amd import _lib as L
        M, N = x.shape[0], self.N
        tdt = torch.float32 if out_dtype == F32 else torch.float16
        size = np.dtype(out_dtype).itemsize
        buf = torch.full(((M + 2) * N + 64,), float("nan"), dtype=tdt, device=self.dev)
        raw = buf.view(torch.uint8)
        raw[:N * size] = GUARD_BYTE
        raw[(M + 1) * N * size:] = GUARD_BYTE
        out = buf[N:(M + 1) * N]
        assert out.data_ptr() % 16 == 0
        xt = _t(x, self.dev)
        a = L.MqW4A16Args()
        a.x, a.x_dtype = xt.data_ptr(), L.MQ_F32 if x.dtype == F32 else L.MQ_F16
        a.M, a.N, a.K, a.group_size = M, N, self.K, self.K if self.g == -1 else self.g
        a.w_packed, a.scales, a.zeros = self.qw.data_ptr(), self.s.data_ptr(), self.z.data_ptr()
        a.bias = self.b.data_ptr() if bias else None
        a.out, a.out_dtype = out.data_ptr(), L.MQ_F32 if out_dtype == F32 else L.MQ_F16
        L.call("mq_w4a16_linear", ctypes.byref(a), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        h = raw.cpu().numpy()
        front, back = h[:N * size], h[(M + 1) * N * size:]
        assert np.all(front == GUARD_BYTE), "%s: %d bytes of the guard row in front of the output changed, first at byte %d" % (
            what, int((front != GUARD_BYTE).sum()), int(np.argmax(front != GUARD_BYTE)))
        assert np.all(back == GUARD_BYTE), "%s: %d bytes of the guard behind the output changed, first at byte %d (element %d past the end)" % (
            what, int((back != GUARD_BYTE).sum()), int(np.argmax(back != GUARD_BYTE)), int(np.argmax(back != GUARD_BYTE)) // size)
        return h[N * size:(M + 1) * N * size].copy().view(out_dtype).reshape(M, N)


def assert_case_bits(got, want, what, p):
    """assert_bits with the launch plan and the bad columns modulo 16 (wave of the GEMV, lane of the GEMM tile) and modulo rows_per_wg
    (position inside the workgroup: slot = that // 16) -- a slot or bias mix-up reads off the message."""
    try:
        assert_bits(got, want, what)
    except AssertionError as e:
        cols = np.unique(np.argwhere(bits(got) != bits(want))[:, 1])
        more = "; bad columns mod 16: %s" % sorted(set(int(c) % 16 for c in cols))[:16]
        if p["variant"] == 1:
            rows = p["rows_per_wg"]
            more += "; mod rows_per_wg=%d: %s; their slots: %s" % (rows, sorted(set(int(c) % rows for c in cols))[:16],
                                                                 sorted(set(int(c) % rows // 16 for c in cols))[:16])
        raise AssertionError("%s%s; plan %r" % (e, more, p)) from None


# ---- the exact table ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("id", IDS)
def test_exact_case(dev, cus, id):
    from mobilequant_amd import weight_only
    c = next(c for c in C.exact_cases(cus) if c.id == id)
    p = C.plan(c.M, c.N, c.K, c.g, cus)
    assert weight_only.w4a16_variant(c.M, c.N, c.K, c.g) == p["variant"], p
    b = C.build_exact(c)
    w = Weights(dev, b.packed, b.s16, b.z16, b.bias, c.g)
    for xname, x in (("random", b.x), ("one-hot", b.x_hot)):
        if x is None:
            continue
        for xdt in c.xdts:
            for bias in (False, True):
                what = "%s M=%d N=%d K=%d g=%d x=%s/%s bias=%s" % (c.id, c.M, c.N, c.K, c.g, xname, np.dtype(xdt).name, bias)
                got = w.launch(x.astype(xdt), bias, F32, what)
                assert_case_bits(got, C.want_f32(b, x.astype(xdt), b.bias if bias else None), what, p)


@pytest.mark.parametrize("M", [2, 17])
def test_fp16_out_rounds_once_at_its_edges(dev, cus, M):
    """Column n of every row is W[n] + bias[n], an fp32 number by construction: 65504, the fp32 number below 65520, +-65520 (-> inf),
    subnormals, 2^-25 and 3 2^-25 (ties).  The expectation is the float64 oracle converted to fp16 in one step."""
    from mobilequant_amd import weight_only
    e = C.build_edges(M)
    p = C.plan(M, C.EDGE_N, C.EDGE_K, C.EDGE_G, cus)
    assert weight_only.w4a16_variant(M, C.EDGE_N, C.EDGE_K, C.EDGE_G) == p["variant"] == (1 if M <= 8 else 2)
    w = Weights(dev, e.packed, e.s16, e.z16, e.bias, C.EDGE_G)
    for xdt in (F32, F16):
        what = "fp16 edges M=%d x=%s" % (M, np.dtype(xdt).name)
        assert_case_bits(w.launch(e.x.astype(xdt), True, F16, what), e.want, what, p)
        # and the fp32 output is the unrounded value itself
        assert_case_bits(w.launch(e.x.astype(xdt), True, F32, what + " (fp32 out)"), e.y64.astype(F32), what + " (fp32 out)", p)


# ---- tolerance cases -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("xdt", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("i", range(5))
def test_gaussian_within_the_derived_bound(dev, cus, i, xdt):
    from mobilequant_amd import weight_only
    M, N, K, g = C.tolerance_shapes(cus)[i]
    assert weight_only.w4a16_variant(M, N, K, g) == C.plan(M, N, K, g, cus)["variant"]
    t = C.build_gaussian(M, N, K, g, xdt)
    what = "gaussian M=%d N=%d K=%d g=%d %s" % (M, N, K, g, np.dtype(xdt).name)
    got = Weights(dev, t.packed, t.s16, t.z16, t.bias, g).launch(t.x, True, xdt, what)
    check_bound(got, t.x, t.w16, t.bias, K, xdt, what)


# ---- fresh processes -------------------------------------------------------------------------------------------------------------------
def child(mode, path, limit=240):
    """One child at a time under its own time limit; a child that fails, faults or runs out of time ends the test here."""
    r = subprocess.run([sys.executable, os.path.join(TESTS, "w4a16_child.py"), mode, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=limit)
    tail = "\n".join(r.stdout.splitlines()[-30:])
    assert r.returncode == 0, "w4a16_child.py %s: exit %d\n%s" % (mode, r.returncode, tail)
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def test_big_lds_forms_before_and_after_small_ones(dev, tmp_path):
    """The raised dynamic-LDS limit is cached per process, instantiation and device: a > 32 KB shape as the first call of a process and a
    small one after it, and the other way round in a second process, give the oracle's bits (checked in the child) and each other's."""
    a = child("big-first", str(tmp_path / "a.npz"))
    b = child("small-first", str(tmp_path / "b.npz"))
    assert sorted(a) == sorted(b) and len(a) == 5
    for k in a:
        assert_bits(a[k], b[k], "%s: big-first against small-first" % k)


def test_capture_with_no_earlier_call(dev, tmp_path):
    """"One launch, no host synchronisation: capturable" (include/mobilequant_amd.h): weight_only.w4a16_linear under torch.cuda.graph as
    the first W4A16 call of a process -- a GEMV shape, a GEMM shape and longrow, whose first call raises the LDS limit --, replayed twice
    with x rewritten in place: the oracle's bits each time (checked in the child)."""
    import w4a16_child
    out = child("capture", str(tmp_path / "c.npz"))
    assert sorted(out) == sorted("%s@%d" % (id, r) for id in w4a16_child.CAPTURED for r in (0, 1))
    for id in w4a16_child.CAPTURED:
        assert not np.array_equal(out[id + "@0"], out[id + "@1"])          # the two replays saw different x


# ---- the wrappers ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def small(dev, cus):
    c = next(c for c in C.exact_cases(cus) if c.id == "mt-m5")
    b = C.build_exact(c)
    return c, b, dict(x=_t(b.x, dev), qweight=_t(b.packed, dev), scales=_t(b.s16, dev), zeros=_t(b.z16, dev), bias=_t(b.bias, dev),
                      group_size=c.g)


@pytest.fixture()
def recorder(dev, monkeypatch):
    """_lib.call replaced for the whole test (test_gpu_ops_contract.py's pattern): no malformed pointer can reach a kernel."""
    import mobilequant_amd._lib as L
    from mobilequant_amd import ops, weight_only
    calls = []
    monkeypatch.setattr(L, "call", lambda name, *args: calls.append(name))
    assert weight_only._lib.call is L.call and ops._lib.call is L.call
    return calls


def test_wrappers_refuse_malformed_operands_before_any_launch(dev, small, recorder):
    from mobilequant_amd import weight_only
    c, b, ok = small
    N, K, G = c.N, c.K, c.K // c.g
    bad = {
        "x on the CPU": dict(x=ok["x"].cpu()),
        "qweight on the CPU": dict(qweight=ok["qweight"].cpu()),
        "scales on the CPU": dict(scales=ok["scales"].cpu()),
        "bias on the CPU": dict(bias=ok["bias"].cpu()),
        "float32 scales": dict(scales=ok["scales"].float()),
        "float32 zeros": dict(zeros=ok["zeros"].float()),
        "non-contiguous qweight": dict(qweight=torch.zeros(N, K, dtype=torch.uint8, device=dev)[:, ::2]),
        "scales one element short": dict(scales=ok["scales"].reshape(-1)[:-1].clone()),
        "zeros one element short": dict(zeros=ok["zeros"].reshape(-1)[:-1].clone()),
        "bias of N - 1 elements": dict(bias=ok["bias"][:-1].clone()),
        "x with K - 64 features": dict(x=ok["x"][:, :K - 64].contiguous()),
        "int32 x": dict(x=ok["x"].to(torch.int32)),
        "float64 x": dict(x=ok["x"].double()),
        "integer bias": dict(bias=ok["bias"].to(torch.int32)),
        "a group size that does not divide K": dict(group_size=96),
    }
    assert bad["non-contiguous qweight"]["qweight"].shape == ok["qweight"].shape and not bad["non-contiguous qweight"]["qweight"].is_contiguous()
    wrong = []
    for name, kw in bad.items():
        try:
            weight_only.w4a16_linear(**{**ok, **kw})
            wrong.append(name + ": accepted")
        except (RuntimeError, ValueError) as e:
            if "mobilequant_amd" not in str(e):
                wrong.append("%s: refused by something else: %s" % (name, str(e)[:160]))
        if recorder:
            wrong.append("%s: reached %s" % (name, recorder[0]))
            del recorder[:]
    # w4a16_pack: a CPU weight, a grid one entry short, another bitwidth, a 1-D weight, an unserved K
    wt = torch.zeros(N, K, device=dev)
    s, o = torch.ones(N, G, device=dev), torch.zeros(N, G, device=dev)
    for name, args in (("pack: CPU weight", (wt.cpu(), s, o, 4, False, c.g)), ("pack: short scale", (wt, s.reshape(-1)[:-1], o, 4, False, c.g)),
                       ("pack: short offset", (wt, s, o.reshape(-1)[:-1], 4, False, c.g)), ("pack: 8 bits", (wt, s, o, 8, False, c.g)),
                       ("pack: 1-D weight", (wt.reshape(-1), s, o, 4, False, c.g)), ("pack: K = 96", (wt[:, :96].contiguous(), s, o, 4, False, 32))):
        try:
            weight_only.w4a16_pack(*args)
            wrong.append(name + ": accepted")
        except (RuntimeError, ValueError) as e:
            if "mobilequant_amd" not in str(e):
                wrong.append("%s: refused by something else: %s" % (name, str(e)[:160]))
        if recorder:
            wrong.append("%s: reached %s" % (name, recorder[0]))
            del recorder[:]
    assert not wrong, "; ".join(wrong)
    # the valid call is ONE launch; M == 0 is none and keeps the shape; a 1-D x is one launch of M = 1
    y = weight_only.w4a16_linear(**ok)
    assert recorder == ["mq_w4a16_linear"] and y.shape == (c.M, N)
    del recorder[:]
    for lead in ((0,), (0, 3), (2, 0)):
        y = weight_only.w4a16_linear(**{**ok, "x": torch.zeros(*lead, K, device=dev)})
        assert y.shape == (*lead, N) and y.dtype == torch.float32 and not recorder, lead
    y = weight_only.w4a16_linear(**{**ok, "x": ok["x"][0]})
    assert y.shape == (N,) and recorder == ["mq_w4a16_linear"]


def test_wrapper_converts_what_it_may(dev, small):
    """A misaligned and a non-contiguous x, a float64 and an fp16 bias, a 1-D and a 3-D x: the bits of the aligned contiguous call, which
    are the oracle's."""
    from mobilequant_amd import weight_only
    c, b, ok = small
    want = C.want_f32(b, b.x, b.bias)
    y0 = weight_only.w4a16_linear(**ok)
    torch.cuda.synchronize()
    assert_bits(y0.cpu().numpy(), want, "canonical call")
    off = torch.zeros(c.M * c.K + 1, device=dev)[1:].view(c.M, c.K)
    off.copy_(ok["x"])
    wide = torch.zeros(c.M, 2 * c.K, device=dev)
    wide[:, ::2] = ok["x"]
    assert off.data_ptr() % 16 == 4 and off.is_contiguous() and not wide[:, ::2].is_contiguous()
    assert np.array_equal(b.bias.astype(F16).astype(F32), b.bias)                            # the fp16 bias holds the same values
    forms = {"x 4 bytes past a 16-byte boundary": dict(x=off), "non-contiguous x": dict(x=wide[:, ::2]),
             "transposed x": dict(x=ok["x"].t().contiguous().t()), "float64 bias": dict(bias=ok["bias"].double()),
             "fp16 bias": dict(bias=ok["bias"].half()), "bias 4 bytes past a boundary": dict(bias=torch.cat((ok["bias"][:1], ok["bias"]))[1:]),
             "3-D x": dict(x=ok["x"].reshape(1, c.M, c.K))}
    for name, kw in forms.items():
        y = weight_only.w4a16_linear(**{**ok, **kw})
        torch.cuda.synchronize()
        assert_bits(y.cpu().numpy().reshape(c.M, c.N), want, name)
    y = weight_only.w4a16_linear(**{**ok, "x": ok["x"][2]})
    torch.cuda.synchronize()
    assert y.shape == (c.N,)
    assert_bits(y.cpu().numpy().reshape(1, c.N), want[2:3], "1-D x")
    # fp16 x: fp16 out, the oracle rounded once
    yh = weight_only.w4a16_linear(**{**ok, "x": ok["x"].half()})
    torch.cuda.synchronize()
    assert yh.dtype == torch.float16
    assert_bits(yh.cpu().numpy(), C.R.linear64(b.x, b.w16, b.bias)[0].astype(F16), "fp16 x")


if __name__ == "__main__":                                    # wall time of the file's GPU work: `python tests/test_gpu_w4a16_oracle.py`
    t0 = time.time()
    rc = pytest.main(["-q", "-m", "gpu", "--durations=8", os.path.abspath(__file__)])
    print("wall time %.1f s" % (time.time() - t0))
    sys.exit(rc)
