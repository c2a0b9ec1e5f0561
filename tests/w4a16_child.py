"""Child process of tests/test_gpu_w4a16_oracle.py: what has to be the FIRST W4A16 call of a process (the cache of raised LDS limits in
mq_w4a16_linear is per process, and so is whatever a first launch sets up).  `python tests/w4a16_child.py MODE OUT.npz`:

  big-first      the > 32 KB forms (longrow in <1>, lds-max-m8 in <8>) first, small shapes of the same instantiations after them,
                 then longrow once more (the cached limit)
  small-first    the small shapes first
  capture        torch.cuda.graph around weight_only.w4a16_linear for a GEMV shape, a GEMM shape and longrow, none of them called
                 before in the process; two replays each with x rewritten in place in between

Every output is compared with the float64 oracle bit for bit (exact cases) and written to OUT.npz, so that the parent can compare the two
orders with each other.  Exit status 0: all equal; 1: a mismatch or an error (the traceback is on stdout)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(1, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import w4a16_cases as C  # noqa: E402

BIG, SMALL = ("longrow", "lds-max-m8"), ("slots2-m1", "mt-m5")
CAPTURED = ("mt-m5", "gdiv-m17-k192", "longrow")


def _t(a, dev):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(dev)             # a copy: the case table's arrays are read-only


def case(cus, id):
    return next(c for c in C.exact_cases(cus) if c.id == id)


def run_order(dev, cus, ids):
    from test_gpu_w4a16 import assert_bits, launch
    out = {}
    for n, id in enumerate(ids):
        c = case(cus, id)
        b = C.build_exact(c)
        assert C.plan(c.M, c.N, c.K, c.g, cus)["lds_attr"] == (id in BIG)
        x = b.x.astype(c.xdts[0])
        got = launch(dev, x, *(np.array(a) for a in (b.packed, b.s16, b.z16, b.bias)), c.g, np.float32)
        assert_bits(got, C.want_f32(b, x, b.bias), "%s as call %d of %s" % (id, n, list(ids)))
        out["%s#%d" % (id, ids[:n].count(id))] = got
    return out


def capture_and_replay(dev, cus, id):
    """Captures ONE weight_only.w4a16_linear call (the output is allocated inside the capture) and replays it for the case's random x and
    for a second x, written into the captured input in between."""
    import torch
    from mobilequant_amd import weight_only
    from test_gpu_w4a16 import assert_bits
    c = case(cus, id)
    b = C.build_exact(c)
    qw, s, z, bias = _t(b.packed, dev), _t(b.s16, dev), _t(b.z16, dev), _t(b.bias, dev)
    xs = [b.x, b.x_hot if b.x_hot is not None else np.ascontiguousarray(b.x[:, ::-1])]
    xt = torch.zeros(c.M, c.K, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = weight_only.w4a16_linear(xt, qw, s, z, bias, c.g)
    out = {}
    for r, x in enumerate(xs):
        xt.copy_(_t(x, dev))
        graph.replay()
        torch.cuda.synchronize()
        got = y.cpu().numpy()
        assert_bits(got, C.want_f32(b, x, b.bias), "%s: replay %d of the captured call" % (id, r))
        out["%s@%d" % (id, r)] = got
    return out


def main(mode, path):
    import torch
    assert torch.cuda.is_available(), "needs a ROCm device"
    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if mode == "big-first":
        out = run_order(dev, cus, BIG + SMALL + BIG[:1])
    elif mode == "small-first":
        out = run_order(dev, cus, SMALL + BIG + BIG[:1])
    elif mode == "capture":
        out = {}
        for id in CAPTURED:
            out.update(capture_and_replay(dev, cus, id))
    else:
        raise SystemExit("unknown mode %r" % mode)
    np.savez(path, **out)
    print("ok: %s (%d outputs)" % (mode, len(out)))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
