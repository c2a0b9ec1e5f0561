"""GPU: the wrappers of mobilequant_amd/ops.py held to the pointer contract of ops_contract_cases.py -- the layer between callers and the
C entries that the oracle pins (which call _lib.call on their own buffers) go around.

a. Every valid call of the table through ops.*, canonical operands, against the oracle and the exactness class of the entry's own pin
   (bit equality where that pin is exact, its own bound where it is bounded: the comparisons live with the cases).
b. Every operand the table marks as converted again as a stride-2 view, as a view 4 bytes past a 16-byte boundary, as a 0-dim and a
   [1]-shaped per-tensor grid, as float64 and (where every value is exact in fp16) as float16, and all of them as float64 at once: all
   outputs equal the canonical call's bits.
c. With _lib.call replaced by a recorder that launches NOTHING (installed for the whole part): every malformed operand -- wrong dtype,
   one element too few, non-contiguous where the pointer is raw, on the CPU, an odd K, a `rows` that does not divide -- raises with a
   message that names the operand and with no call recorded; every valid call (canonical and each form of b) hands the current stream's
   handle, pointers that lie inside blocks the caching allocator reports as allocated at that moment, and no pointer twice.
d. The fake (meta) kernel of every operator of torch_ops.py gives the real operator's output shapes and dtypes.

Whether torch.cuda.memory_snapshot() reports block states on a given build is probed once (SNAPSHOT_OK); without them the liveness check
is skipped and distinctness and part b's value check remain.  On the ROCm build this was written on the states are reported: a wrapper
that lets a temporary go before the call fails the liveness check.

A result that holds atomic sums is held to its pin's bound again in part b (Built.stable), and what no caller may read -- the padding rows
of a fragment-blocked image -- is blanked before two calls are compared (Built.canon).

Measured wall time of the whole file on an MI355X: 14.5 s for its 726 tests (the slowest, part b of the gated pair at 1793 x 3072 x 768 --
the smallest shape its dispatch serves --, 2.0 s; part d 1.4 s; the pair's part a 0.8 s; everything else under 0.7 s).  One test, the
two-device refusal, skips on a single device."""
import ctypes
import functools
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ops_contract_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F16 = np.float32, np.float16
ALL = C.all_cases()
IDS = ["%s-%s" % (w.name, c.id) for w, c in ALL]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    import mobilequant_amd._lib as L
    assert L.device_info()["arch"].startswith("gfx950")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def built(i):
    return ALL[i][1].build()


# ---- numpy <-> device -----------------------------------------------------------------------------------------------------------------
def to_dev(v, dev):
    if isinstance(v, np.ndarray):
        return torch.from_numpy(np.array(v, order="K")).to(dev)          # order K: a transposed view keeps its strides on the device
    if isinstance(v, torch.Tensor):
        return v
    if isinstance(v, str) and v == C.DEVICE:
        return dev
    if isinstance(v, dict):
        return {k: to_dev(x, dev) for k, x in v.items()}
    if isinstance(v, (tuple, list)):
        return type(v)(to_dev(x, dev) for x in v)
    return v


def to_np(v):
    if isinstance(v, torch.Tensor):
        if v.dtype == torch.uint16:
            return v.view(torch.int16).cpu().numpy().view(np.uint16)
        return v.detach().cpu().numpy()
    if isinstance(v, dict):
        return {k: to_np(x) for k, x in v.items()}
    if isinstance(v, (tuple, list)):
        return type(v)(to_np(x) for x in v)
    return v


def invoke(w, args):
    from mobilequant_amd import ops
    return getattr(ops, w.name)(**args)


def all_float64(w, b, args):
    """args with EVERY converted operand as float64 at once: each needs a temporary of its own, so one released too early is handed to the
    next (the single-operand forms leave a stale pointer's old bits in place)."""
    n = 0
    for o, a in present(w, b):
        if o.kind == "conv":
            args = C.replace(args, o.path, C.lookup(args, o.path).double())
            n += 1
    return args if n >= 2 else None


def run(w, args_np, dev, replace=None, fresh_cache=False, every=None):
    """One call from the numpy arguments (replace: (path, device tensor) put in place of one operand) -> (result, arguments afterwards).
    fresh_cache: the caching allocator's free lists are emptied behind the arguments, so that a temporary the wrapper releases too early is
    the best fit of its next allocation: the stale pointer then reads another operand's value instead of its own old bits."""
    args = to_dev(args_np, dev)
    if replace is not None:
        args = C.replace(args, *replace)
    if every is not None:
        args = every(args)
    if fresh_cache:
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    out = invoke(w, args)
    torch.cuda.synchronize()
    return to_np(out), to_np(args)


def present(w, b):
    """(operand, canonical array) of every operand of the table that this call passes."""
    for o in w.operands:
        try:
            v = C.lookup(b.args, o.path)
        except (KeyError, IndexError, TypeError):
            continue
        if isinstance(v, np.ndarray):
            yield o, v


# ---- the forms of part b ---------------------------------------------------------------------------------------------------------------
def stride2(t):
    if t.dim() == 0:
        return None
    buf = torch.zeros(t.shape[:-1] + (2 * t.shape[-1],), dtype=t.dtype, device=t.device)
    v = buf[..., ::2]
    v.copy_(t)
    assert t.numel() < 2 or not v.is_contiguous()
    return v


def offset4(t):
    k = max(1, 4 // t.element_size())
    buf = torch.zeros(t.numel() + k + 16, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[k:k + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == max(4, t.element_size()) and v.is_contiguous()          # (an 8-byte element: 8 bytes past)
    return v


def exact_in_f16(a):
    with np.errstate(over="ignore", invalid="ignore"):
        back = a.astype(F16).astype(a.dtype)
    return bool(np.all((back == a) | (np.isnan(back) & np.isnan(a))) and np.array_equal(np.signbit(back), np.signbit(a)))


def forms(o, a, dev):
    """(name, device tensor) of every other form operand o (canonical array a) may arrive in."""
    t = torch.from_numpy(np.array(a)).to(dev)
    out = [("stride2", stride2(t))]
    if not o.align16:
        out.append(("offset4", offset4(t)))
    if o.kind == "conv":
        out.append(("float64", t.double()))
        if exact_in_f16(a):
            out.append(("float16", t.half()))
        if a.size == 1:
            out += [("0-dim", t.reshape(())), ("[1]", t.reshape(1))]
    return [(n, v) for n, v in out if v is not None]


def same_tree(got, want, what, flat=False):
    """flat: a result shaped like a per-tensor grid follows that grid's own form (0-dim or [1]); its one value is compared."""
    if isinstance(want, np.ndarray):
        if flat and want.size == 1 and np.asarray(got).size == 1:
            got, want = np.asarray(got).reshape(-1), want.reshape(-1)
        C.same_bits(got, want, what)
    elif isinstance(want, dict):
        for k in want:
            same_tree(got[k], want[k], "%s[%r]" % (what, k), flat)
    elif isinstance(want, (tuple, list)):
        assert len(got) == len(want), what
        for i, (g, x) in enumerate(zip(got, want)):
            same_tree(g, x, "%s[%d]" % (what, i), flat)
    else:
        assert got == want or (got is None and want is None), (what, got, want)


def stop_unless_refusal(e):
    """Part b goes on to the next form after a wrong value or a refusal of the project's own (the wrapper's "mobilequant_amd: ..." or the
    entry's status).  Any other RuntimeError -- a HIP error is one -- ends the test there: nothing more is launched behind a fault."""
    from mobilequant_amd._lib import MobileQuantLibraryError
    if isinstance(e, AssertionError) or isinstance(e, MobileQuantLibraryError) or str(e).startswith("mobilequant_amd:"):
        return
    raise e


def written(w, after):
    """The in-place and caller-owned output operands of a call, after it."""
    out = {}
    for o in w.operands:
        if o.kind in ("inplace", "out"):
            try:
                out[o.path] = C.lookup(after, o.path)
            except (KeyError, IndexError, TypeError):
                pass
    return out


# ---- a ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(ALL)), ids=IDS)
def test_wrapper_computes_what_the_oracle_says(dev, i):
    """The pin's comparison made through the wrapper: wrong rows / cols, a wrong entry, swapped arguments, wrong output shapes and dtypes."""
    w, _ = ALL[i]
    b = built(i)
    out, after = run(w, b.args, dev)
    b.check(out, after)


# ---- b ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(ALL)), ids=IDS)
def test_layout_and_dtype_independence(dev, i):
    """Every converted operand in every other form it may arrive in: the bits of the canonical call, in-place statistics included."""
    w, _ = ALL[i]
    b = built(i)
    ops_here = [(o, a) for o, a in present(w, b) if o.kind in ("conv", "layout")]
    if not ops_here:
        return
    canon = b.canon or (lambda r: r)
    out0, after0 = run(w, b.args, dev)
    out0, wr0 = canon(out0), written(w, after0)

    def judge(out, after, what, flat=False):
        if not b.stable:                       # atomic sums: the pin's own comparison again
            b.check(out, after)
            return
        same_tree(canon(out), out0, what, flat)
        same_tree(written(w, after), wr0, what + " (written operands)")
    bad = []
    for o, a in ops_here:
        for name, t in forms(o, a, dev):
            what = "%s %s as %s" % (IDS[i], ".".join(str(p) for p in o.path), name)
            try:
                out, after = run(w, b.args, dev, replace=(o.path, t), fresh_cache=o.kind == "conv" and a.size == 1)
                judge(out, after, what, flat=name in ("0-dim", "[1]"))
            except (AssertionError, RuntimeError) as e:
                stop_unless_refusal(e)
                bad.append("%s: %s" % (what, str(e).splitlines()[0][:300]))
    if all_float64(w, b, to_dev(b.args, dev)) is not None:
        what = "%s every converted operand as float64" % IDS[i]
        try:
            out, after = run(w, b.args, dev, fresh_cache=True, every=lambda args: all_float64(w, b, args))
            judge(out, after, what)
        except (AssertionError, RuntimeError) as e:
            stop_unless_refusal(e)
            bad.append("%s: %s" % (what, str(e).splitlines()[0][:300]))
    assert not bad, "\n".join(bad)


# ---- c: the recorder -------------------------------------------------------------------------------------------------------------------
SNAPSHOT_OK = None


def live_blocks():
    """[(begin, end)] of every block the caching allocator holds as allocated right now; None where the build reports no block states."""
    global SNAPSHOT_OK
    out, states = [], set()
    for seg in torch.cuda.memory_snapshot():
        addr = seg.get("address", 0)
        for blk in seg.get("blocks", ()):
            a = blk.get("address", addr)
            states.add(blk.get("state"))
            if blk.get("state") == "active_allocated":
                out.append((a, a + blk["size"]))
            addr = a + blk["size"]
    if SNAPSHOT_OK is None:
        SNAPSHOT_OK = "active_allocated" in states and bool(out) and all(b > a > 0 for a, b in out)
    return out if SNAPSHOT_OK else None


def pointers(v, pos, out):
    """(top-level argument position, address) of everything in a C argument that is a device address: integers past 2^32 -- sizes, counts
    and dtype codes lie below --, the elements of ctypes arrays, the fields of structs (by value or by reference)."""
    if v is None or isinstance(v, (float, bool)):
        return
    if isinstance(v, int):
        if v >= 1 << 32:
            out.append((pos, v))
    elif isinstance(v, ctypes.Array):
        for e in v:
            pointers(e, pos, out)
    elif isinstance(v, ctypes.Structure):
        for f in v._fields_:
            pointers(getattr(v, f[0]), pos, out)
    elif hasattr(v, "_obj"):                     # ctypes.byref(...)
        pointers(v._obj, pos, out)
    elif hasattr(v, "value"):
        pointers(v.value, pos, out)


class Recorder:
    """Stands in for _lib.call: stores (entry, arguments) and judges the pointers AT THE MOMENT OF THE CALL; never reaches the library."""

    def __init__(self):
        self.calls, self.problems, self.aliases, self.last_ptrs = [], [], (), set()

    def __call__(self, name, *args):
        self.calls.append((name, args))
        stream = torch.cuda.current_stream().cuda_stream
        if args[-1] != stream:
            self.problems.append("%s: stream argument %r is not the current stream's handle %r" % (name, args[-1], stream))
        ptrs = []
        for pos, a in enumerate(args[:-1]):
            pointers(a, pos, ptrs)
        self.last_ptrs = {p for _, p in ptrs}
        live = live_blocks()
        if live is not None:
            for pos, p in ptrs:
                if not any(a <= p < b for a, b in live):
                    self.problems.append("%s: argument %d points at %#x, inside no block that is allocated now (a released temporary)" % (name, pos, p))
        seen = {}
        for pos, p in ptrs:
            if p in seen and seen[p] != pos and (seen[p], pos) not in self.aliases:
                self.problems.append("%s: arguments %d and %d hold one pointer %#x" % (name, seen[p], pos, p))
            seen.setdefault(p, pos)

    def take(self):
        calls, problems = self.calls, self.problems
        self.calls, self.problems = [], []
        return calls, problems


@pytest.fixture()
def recorder(dev, monkeypatch):
    """_lib.call replaced for the whole test: no malformed pointer can reach a kernel."""
    import mobilequant_amd._lib as L
    rec = Recorder()
    monkeypatch.setattr(L, "call", rec)
    from mobilequant_amd import ops
    assert ops._lib.call is rec
    return rec


def _wrong_dtype(o, a):
    with np.errstate(invalid="ignore"):
        if o.kind == "conv":
            return a.astype(np.int32)
        if a.dtype.kind == "f":
            return a.astype(np.float64) if len(o.dtype) > 1 else a.astype(np.int32)
        return a.astype(np.float32)


def malformed(o, a, dev):
    """(name, value) of every malformed form of operand o: a CPU tensor, a wrong dtype, one element too few, and -- where the pointer is
    passed raw -- a non-contiguous view that holds every element."""
    t = torch.from_numpy(np.array(a))
    out = [("cpu", t), ("dtype", torch.from_numpy(_wrong_dtype(o, a)).to(dev))]
    if o.numel is not None:
        out.append(("short", t.reshape(-1)[:-1].clone().to(dev)))
    if o.kind in ("raw", "inplace", "out") and a.size > 1:
        out.append(("noncontiguous", stride2(t.to(dev))))
    return out


def first_case_with(wi, path):
    for i, (w, _) in enumerate(ALL):
        if w is wi:
            try:
                if isinstance(C.lookup(built(i).args, path), np.ndarray):
                    return i
            except (KeyError, IndexError, TypeError):
                pass
    return None


OPERANDS = [(w, o) for w in C.WRAPPERS for o in w.operands]


@pytest.mark.parametrize("k", range(len(OPERANDS)), ids=["%s-%s" % (w.name, ".".join(str(p) for p in o.path)) for w, o in OPERANDS])
def test_malformed_operand_is_refused_before_anything_is_launched(dev, recorder, k):
    w, o = OPERANDS[k]
    i = first_case_with(w, o.path)
    assert i is not None, "no case of %s passes %r" % (w.name, o.path)
    b = built(i)
    a = C.lookup(b.args, o.path)
    bad = []
    for name, t in malformed(o, a, dev):
        args = C.replace(to_dev(b.args, dev), o.path, t)
        try:
            invoke(w, args)
            bad.append("%s: accepted" % name)
        except (RuntimeError, ValueError) as e:
            if not re.search(o.label, str(e)):
                bad.append("%s: refused without naming %r: %s" % (name, o.label, str(e)[:200]))
        calls, _ = recorder.take()
        if calls:
            bad.append("%s: reached %s" % (name, calls[0][0]))
    assert not bad, "%s %s: %s" % (w.name, o.path, "; ".join(bad))


def test_other_refusals(dev, recorder):
    """An odd K and a non-2-D tensor for pack_w4, a `rows` that does not divide, scales that do not divide, an out= and a grad_y of another
    shape, weights whose K does not match a_q, a stats list of the wrong length or with a 2-element slot, an out= that is raw itself."""
    from mobilequant_amd import ops
    x = torch.zeros(6, 10, device=dev)
    s1, o1 = torch.ones(1, device=dev), torch.zeros(1, device=dev)
    raw = torch.zeros(2, 8, 8, device=dev)
    res_out = torch.zeros(16, 8, device=dev)                                       # out= that is the residual itself
    cases = [
        ("nibbles", lambda: ops.pack_w4(torch.zeros(3, 7, dtype=torch.uint8, device=dev))),
        ("nibbles", lambda: ops.pack_w4(torch.zeros(8, dtype=torch.uint8, device=dev))),
        ("nibbles", lambda: ops.pack_w4(torch.randint(0, 16, (3, 128), device=dev))),                  # int64, what randint gives by default
        ("rows", lambda: ops.quantize(x, s1, o1, 0.0, 255.0, rows=7)),
        ("rows", lambda: ops.quantize(x, torch.ones(3, device=dev), torch.zeros(3, device=dev), 0.0, 255.0, rows=6)),
        ("scales do not divide", lambda: ops.fake_quant(x, torch.ones(7, device=dev), torch.zeros(7, device=dev), 0.0, 255.0)),
        ("out", lambda: ops.fake_quant(x, s1, o1, 0.0, 255.0, out=torch.zeros(10, 6, device=dev))),
        ("grad_y", lambda: ops.fake_quant_backward(x, torch.zeros(10, 6, device=dev), s1, o1, 0.0, 255.0)),
        ("w_q", lambda: ops.int8_linear(torch.zeros(4, 64, dtype=torch.int8, device=dev), torch.zeros(8, 32, dtype=torch.int8, device=dev), None,
                                        torch.ones(8, device=dev), torch.zeros(8, dtype=torch.int32, device=dev),
                                        torch.zeros(8, dtype=torch.int32, device=dev))),
        ("stats", lambda: ops.calib_gated_(x, x.clone(), "silu", [torch.zeros(1, device=dev) for _ in range(7)])),
        ("stats", lambda: ops.calib_gated_(x, x.clone(), "silu", [torch.zeros(1, device=dev) for _ in range(7)] + [torch.zeros(2, device=dev)])),
        ("resid must be", lambda: ops.int8_linear(torch.zeros(16, 128, dtype=torch.int8, device=dev), torch.zeros(8, 128, dtype=torch.int8, device=dev),
                                                  None, torch.ones(8, device=dev), torch.zeros(8, dtype=torch.int32, device=dev),
                                                  torch.zeros(8, dtype=torch.int32, device=dev), out=res_out, resid=res_out)),
        ("out must not be raw", lambda: ops.calib_attention_probs_causal_(raw, raw, 1.0, False, *[torch.zeros(1, device=dev) for _ in range(4)])),
    ]
    bad = []
    for label, fn in cases:
        try:
            fn()
            bad.append("%s: accepted" % label)
        except (RuntimeError, ValueError) as e:
            if label not in str(e):
                bad.append("refused without naming %r: %s" % (label, str(e)[:200]))
        calls, _ = recorder.take()
        if calls:
            bad.append("%s: reached %s" % (label, calls[0][0]))
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("i", range(len(ALL)), ids=IDS)
def test_valid_calls_hand_over_live_distinct_pointers_on_the_current_stream(dev, recorder, i):
    """The canonical call and every form of part b under the recorder: the stream handle, live blocks, no pointer twice."""
    w, _ = ALL[i]
    b = built(i)
    recorder.aliases = w.aliases
    todo = [("canonical", None)]
    for o, a in present(w, b):
        if o.kind in ("conv", "layout"):
            todo += [("%s as %s" % (".".join(str(p) for p in o.path), n), (o.path, t)) for n, t in forms(o, a, dev)]
    todo.append(("every converted operand as float64", "all"))
    bad = []
    for what, rep in todo:
        args = to_dev(b.args, dev)
        if rep == "all":
            args = all_float64(w, b, args)
            if args is None:
                continue
        elif rep is not None:
            args = C.replace(args, *rep)
        invoke(w, args)
        calls, problems = recorder.take()
        if not calls and w.operands:
            bad.append("%s: nothing was called" % what)
        if rep not in (None, "all") and what.endswith(("as float64", "as float16")) and rep[1].data_ptr() in recorder.last_ptrs:
            bad.append("%s: the operand's own pointer went to the entry, which reads float32" % what)
        bad += ["%s: %s" % (what, p) for p in problems]
    assert not bad, "\n".join(bad)


def test_side_stream_handle_reaches_the_entry(dev, recorder):
    """Under torch.cuda.stream(s) the entry gets s's handle (the default stream's handle is 0: only a side stream tells)."""
    s = torch.cuda.Stream(device=dev)
    assert s.cuda_stream != 0
    seen = []
    with torch.cuda.stream(s):
        for name in ("fake_quant", "quantize", "act_quant", "int8_linear", "minmax_tensor_", "linear_epilogue_prepare"):
            i = next(j for j, (w, _) in enumerate(ALL) if w.name == name)
            invoke(ALL[i][0], to_dev(built(i).args, dev))
            calls, problems = recorder.take()
            assert calls and not problems, (name, problems)
            seen += [c[1][-1] for c in calls]
    assert seen and all(h == s.cuda_stream for h in seen), (seen, s.cuda_stream)


def test_operand_on_another_device_is_refused(dev, recorder):
    if torch.cuda.device_count() < 2:
        pytest.skip("one visible device: _on's two-device refusal needs a second one")
    other = torch.device("cuda:1")
    bad = []
    for name, path in (("fake_quant", ("offset",)), ("quantize", ("scale",)), ("act_quant", ("out_grid", 0)), ("int8_linear", ("alpha",)),
                       ("minmax_rows_", ("mx",)), ("lwc_fake_quant", ("sig_hi",))):
        i = next(j for j, (w, _) in enumerate(ALL) if w.name == name)
        b = built(i)
        args = C.replace(to_dev(b.args, dev), path, torch.from_numpy(np.array(C.lookup(b.args, path))).to(other))
        try:
            invoke(ALL[i][0], args)
            bad.append(name + ": accepted")
        except RuntimeError as e:
            if "different devices" not in str(e):
                bad.append("%s: %s" % (name, e))
        if recorder.take()[0]:
            bad.append(name + ": launched")
    assert not bad, bad


# ---- predicates ------------------------------------------------------------------------------------------------------------------------
def test_decode_shape_and_gemm_predicates(dev, recorder):
    """Each condition violated once gives False; a True is a call the wrapper then accepts (under the recorder)."""
    from mobilequant_amd import ops
    import gemm_cases as G
    assert ops.decode_shape(8, 256) and ops.decode_shape(1, 65280)
    for M, K in ((9, 256), (8, 128), (8, 8192), (1, 65536), (2, 32768)):
        assert not ops.decode_shape(M, K), (M, K)
    M, K, N = 8, 256, 24
    ops.int8_linear_f32in(torch.zeros(M, K, device=dev), torch.ones(1, device=dev), torch.zeros(1, device=dev), 0.0, 255.0, 128,
                          torch.zeros(N, K, dtype=torch.int8, device=dev), torch.ones(N, device=dev), torch.zeros(N, dtype=torch.int32, device=dev),
                          torch.zeros(N, dtype=torch.int32, device=dev))
    assert [c[0] for c in recorder.take()[0]] == ["mq_w8a8_linear_f32in"]
    for pred, ref, ok, viol in (
            (ops.gemm_tiled128_supported, G.fr128_shape, (17, 128, 768), [(17, 120, 768), (17, 128, 512), (17, 128, 800), (0, 128, 768)]),
            (ops.gemm_tiled_supported, G.tiled_supported, (256, 176 * 192, 256), [(256, 176 * 191, 256), (256, 176 * 192, 128), (256, 176 * 192 + 16, 256),
                                                                                   (0, 176 * 192, 256)]),
            (ops.gemm_tiled_w4_supported, G.frw4_shape, (17, 176, 768), [(17, 120, 768), (17, 176, 512), (17, 176, 800), (0, 176, 768)])):
        assert pred(*ok) and ref(*ok), (pred.__name__, ok)
        for sh in viol:
            assert not ref(*sh) and not pred(*sh), (pred.__name__, sh)
    # a True is the call the wrapper then accepts: the fragment-blocked image of M rows against [N, K] (packed: [N, K / 2]) weights
    def z(*shape, dtype=torch.int8):
        return torch.zeros(*shape, dtype=dtype, device=dev)
    g = (torch.ones(1, device=dev), torch.zeros(1, device=dev) + 3)
    for (M, N, K), w4, want in (((17, 128, 768), False, "mq_w8a8_linear_tiled"), ((256, 176 * 192, 256), False, "mq_w8a8_linear_tiled"),
                                ((17, 176, 768), True, "mq_w4a8_linear_tiled")):
        a = z((M + 15) // 16 * 16, K)
        vec = (z(M, dtype=torch.int32), torch.ones(N, device=dev), z(N, dtype=torch.int32), z(N, dtype=torch.int32))
        if w4:
            ops.w4a8_linear_tiled(a, M, z(N, K // 2, dtype=torch.uint8), *vec, None, [g])
        else:
            ops.int8_linear(a, z(N, K), *vec, None, out_scale=g[0], out_offset=g[1], out_dtype=C.MQ["u8"], a_tiled_rows=M)
        assert [c[0] for c in recorder.take()[0]] == [want], (M, N, K)
    M, N, K = 17, 128, 768                   # gemm_tiled128_supported is also what int8_linear(resid=, a_tiled_rows=) asks
    ops.int8_linear(z(32, K), z(N, K), z(M, dtype=torch.int32), torch.ones(N, device=dev), z(N, dtype=torch.int32), z(N, dtype=torch.int32), None,
                    out_scale=g[0], out_offset=g[1], out_qmin=0.0, out_qmax=65535.0, a_tiled_rows=M, resid=torch.zeros(M, N, device=dev))
    assert [c[0] for c in recorder.take()[0]] == ["mq_w8a8_linear_tiled_residual"]


def test_tensor_predicates(dev, recorder):
    from mobilequant_amd import ops
    w = torch.zeros(5, 64, device=dev)
    assert ops.lwc_fake_quant_supported(w)
    ops.lwc_fake_quant(w, torch.ones(5, device=dev), torch.ones(5, device=dev), 4, False)
    assert [c[0] for c in recorder.take()[0]] == ["mq_lwc_fake_quant"]
    big = torch.zeros(2, 16388, device=dev)
    for bad in (w.cpu(), w.half(), w[0], torch.zeros(5, 66, device=dev), torch.zeros(5, 0, device=dev), big, torch.zeros(5, 128, device=dev)[:, ::2],
                torch.zeros(5 * 64 + 4, device=dev)[1:1 + 5 * 64].view(5, 64)):
        assert not ops.lwc_fake_quant_supported(bad), (bad.shape, bad.dtype, bad.device)
    raw = torch.zeros(2, 3, 8, 16, device=dev)
    mask = torch.zeros(1, 1, 8, 16, device=dev)
    assert ops.attention_probs_train_supported(raw, None) and ops.attention_probs_train_supported(raw, mask)
    g = (torch.ones(1, device=dev), torch.zeros(1, device=dev) + 3, 0.0, 255.0)
    ops.attention_probs_train(raw, mask, g, g, 4.0)
    assert [c[0] for c in recorder.take()[0]] == ["mq_attention_probs_train"]
    for r in (raw.cpu(), raw.half(), raw[0, 0, 0], raw[..., ::2], torch.zeros(2, 8, 18, device=dev), torch.zeros(2, 8, 4100, device=dev),
              torch.zeros(2 * 8 * 16 + 4, device=dev)[1:1 + 256].view(2, 8, 16)):
        assert not ops.attention_probs_train_supported(r, None), (r.shape, r.dtype, r.device)
    for m in (mask.cpu(), mask.half(), mask[0, 0, 0], torch.zeros(2, 1, 8, 16, device=dev), torch.zeros(1, 1, 8, 12, device=dev),
              torch.zeros(1, 1, 4, 16, device=dev)):
        assert not ops.attention_probs_train_supported(raw, m), (m.shape, m.dtype, m.device)
    x1, x2 = torch.zeros(2, 5, 8, device=dev), torch.zeros(2, 8, 12, device=dev)
    assert ops.qmatmul_supported(x1, x2)
    ops.qmatmul(x1, x2, g, g, None)
    assert [c[0] for c in recorder.take()[0]] == ["mq_qmatmul"]
    for a, b in ((x1.cpu(), x2), (x1, x2.cpu()), (x1.half(), x2), (x1, x2.half()), (x1[0, 0], x2[0, 0]), (x1[0], x2), (x1[:1], x2), (x1, x2[:, :4]),
                 (x1[:, :0], x2), (x1, x2[..., :0]), (torch.zeros(1, 1, 131072, device=dev), torch.zeros(1, 131072, 4, device=dev))):
        assert not ops.qmatmul_supported(a, b), (a.shape, b.shape)


# ---- d: torch_ops fake kernels ---------------------------------------------------------------------------------------------------------
def _meta(v):
    if isinstance(v, torch.Tensor):
        return (tuple(v.shape), v.dtype)
    if isinstance(v, (tuple, list)):
        return tuple(_meta(x) for x in v)
    return v


def _case_args(name, cid, dev):
    i = IDS.index("%s-%s" % (name, cid))
    return to_dev(built(i).args, dev)


def torch_op_calls(dev):
    """name -> positional arguments of the operator on the table's small case (or, for the operators without an entry, a minimal one)."""
    fq = _case_args("fake_quant", "f32-row", dev)
    q = _case_args("quantize", "chan-sum", dev)
    lin = _case_args("int8_linear", "plain-f32-16", dev)
    lin4 = dict(_case_args("int8_linear", "w4-u8", dev))
    x = _case_args("minmax_cols", "f32", dev)["x2d"]
    run_mm = _case_args("minmax_cols_", "f32", dev)
    caches = [torch.zeros(2, 2, 32, 16, dtype=torch.int8, device=dev) for _ in range(2)]
    pos, parent = torch.tensor([3, 0], dtype=torch.int32, device=dev), torch.tensor([0, 0], dtype=torch.int32, device=dev)
    w2d = torch.randn(5, 64, device=dev)
    lin_args = lambda a: (a["a_q"], a["a_rowsum"], a["w_q"], a["alpha"], a["w_zp"], a["col_term"], a["bias"], a["out_scale"], a["out_offset"],  # noqa: E731
                          a["out_qmin"], a["out_qmax"])
    return {
        "fake_quant": (fq["x"], fq["scale"], fq["offset"], fq["qmin"], fq["qmax"]),
        "quantize": (q["x"], q["scale"], q["offset"], q["qmin"], q["qmax"], q["shift"], q["chan_scale"]),
        "minmax": (x, True),
        "minmax_update_": (torch.stack([run_mm["mn"], run_mm["mx"]]), x),
        "hist_minmax_update_": (torch.zeros(512, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev),
                                torch.tensor([[float("inf")], [float("-inf")]], device=dev), x, 0),
        "w8a8_linear": lin_args(lin),
        "pack_w4": (_case_args("pack_w4", "3x128", dev)["nibbles"],),
        "w4a8_linear": lin_args(lin4),
        "decode_cache_fork": (caches, pos, parent),
        "decode_cache_reorder": (caches, pos, parent),
        "beam_select": (torch.randn(4, 100, device=dev), torch.zeros(4, device=dev), torch.tensor([0, 0, 1, 1], dtype=torch.int32, device=dev), 2, 3),
        "lwc_search": (w2d, torch.linspace(0.5, 1.0, 6, device=dev), torch.linspace(0.5, 1.0, 6, device=dev), 4, False, None),
    }


def test_fake_kernels_give_the_real_operators_shapes_and_dtypes(dev):
    from torch._subclasses.fake_tensor import FakeTensorMode
    import mobilequant_amd.torch_ops as T
    calls = torch_op_calls(dev)
    assert sorted(calls) == sorted(T.OPS), "an operator of torch_ops.OPS without a call here"
    bad = []
    for name in T.OPS:
        fn = getattr(torch.ops.mobilequant_amd, name)
        args = calls[name]
        real = _meta(fn(*args))
        torch.cuda.synchronize()
        mode = FakeTensorMode()
        conv = lambda v: mode.from_tensor(v) if isinstance(v, torch.Tensor) else ([conv(x) for x in v] if isinstance(v, list) else v)  # noqa: E731
        with mode:
            fake = _meta(fn(*[conv(a) for a in args]))
        if real != fake:
            bad.append("%s: real %r, fake %r" % (name, real, fake))
    assert not bad, "\n".join(bad)
