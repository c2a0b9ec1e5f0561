"""Percentile activation ranges without a GPU: the numpy reference against the rule's own properties, calibration.percentile_range
against the reference, the argument checks of mq_hist_minmax_tensor and of the collector, and the data-parallel path of
get_act_range(method="percentile") over gloo ranks (the device op replaced by numpy stand-ins; the kernel itself: test_gpu_hist.py).
Every comparison is exact."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import hist_ref as R
from toy_models import CalibToy

MS = (0, 3, 5, 6)


def _edge_values(m):
    """Sorted fp32 values around every kind of bin bound: zeros, denormals, bounds and their neighbours, the extremes, infinities."""
    f32 = np.float32
    v = [0.0, 1e-45, 1e-40, 1.1754942e-38, 1.17549435e-38, np.finfo(f32).max, np.inf]
    for e in (-126, -30, -1, 0, 1, 7, 127):
        for k in range(0, 1 << m, max(1, (1 << m) // 4)):
            x = f32(2.0 ** e) * f32(1.0 + k * 2.0 ** -m)
            v += [x, np.nextafter(x, f32(np.inf)), np.nextafter(x, f32(0))]
    v = np.array(v, dtype=f32)
    v = np.unique(np.concatenate((v, -v, np.random.default_rng(m).standard_normal(4000).astype(f32))))
    return v[np.argsort(v, kind="stable")]


@pytest.mark.parametrize("m", MS)
def test_reference_bins_follow_value_order_and_bounds_hold_their_values(m):
    v = _edge_values(m)
    b, nan = R.bin_index(v, m)
    assert not nan.any() and (np.diff(b) >= 0).all()             # bin index monotone in value
    lo, hi = R.bin_bounds(m)
    assert lo.dtype == np.float32 and lo.size == 2 * R.nb_of(m)
    nb = R.nb_of(m)
    pos = b >= nb
    fin = np.isfinite(v)
    assert (v[pos & fin] >= lo[b[pos & fin]]).all() and (v[pos & fin] < hi[b[pos & fin]]).all()
    assert (v[~pos] > lo[b[~pos]])[fin[~pos]].all() and (v[~pos] <= hi[b[~pos]]).all()
    # +-inf are the only occupants of keys 255 << m, with equal bounds; -0 counts as +0
    assert b[-1] == nb + (255 << m) and lo[b[-1]] == np.inf == hi[b[-1]] and b[0] == nb - 1 - (255 << m) and hi[b[0]] == -np.inf
    assert (b[np.isinf(v)] == [b[0], b[-1]]).all() and np.isinf(v).sum() == 2
    assert R.bin_index(np.array([-0.0, 0.0], np.float32), m)[0].tolist() == [nb, nb]
    assert R.bin_index(np.array([-1e-45, 1e-45], np.float32), m)[0].tolist() == [nb - 1, nb]
    c, n = R.histogram(np.array([np.nan, 1.0, -np.nan, -0.0], np.float32), m)
    assert n == 2 and c.sum() == 2 and c[nb] == 1 and c[nb + (127 << m)] == 1
    # bounds are contiguous: every bin starts where its lower neighbour ends
    assert (lo[nb + 1:] == hi[nb:-1]).all() and (lo[1:nb] == hi[:nb - 1]).all() and lo[nb] == 0.0 and hi[nb - 1] == 0.0


@pytest.mark.parametrize("m", MS)
def test_bin_bounds_equal_the_reference(m):
    from mobilequant_amd.calibration import histogram_bin_bounds
    lo, hi = histogram_bin_bounds(m)
    rlo, rhi = R.bin_bounds(m)
    assert lo.dtype == torch.float32 and hi.dtype == torch.float32
    assert np.array_equal(lo.numpy().view(np.uint32), rlo.view(np.uint32)) and np.array_equal(hi.numpy().view(np.uint32), rhi.view(np.uint32))


def _count_vectors(m):
    """(name, counts, mn, mx): random histograms of real data and the adversarial ones."""
    rng = np.random.default_rng(100 + m)
    nb = R.nb_of(m)
    lo, hi = R.bin_bounds(m)
    out = []
    for k, n in enumerate((100003, 4097, 50)):
        x = (rng.standard_normal(n) * 10.0 ** (k - 1)).astype(np.float32)
        x[:4] = [40.0, -40.0, 55.0, -55.0]
        out.append((f"normal{n}", R.histogram(x, m)[0], float(x.min()), float(x.max())))
    x = np.abs(rng.standard_normal(3001)).astype(np.float32)          # one-sided (an activation's output)
    out.append(("onesided", R.histogram(x, m)[0], float(x.min()), float(x.max())))
    c = np.zeros(2 * nb, np.int64)
    c[nb + (127 << m)] = 12345                                          # all mass in one bin
    out.append(("onebin", c, 1.0, float(np.nextafter(np.float32(1.0), np.float32(2.0)))))
    c = np.zeros(2 * nb, np.int64)
    c[nb - 1 - (255 << m)], c[nb + (255 << m)] = 7, 9                   # mass only in the two extreme (infinity) bins
    out.append(("infbins", c, -np.inf, np.inf))
    c = np.zeros(2 * nb, np.int64)
    c[nb - 1 - (254 << m) - ((1 << m) - 1)], c[nb + (254 << m) + ((1 << m) - 1)] = 500, 3   # ... and in the two extreme finite bins
    out.append(("maxbins", c, -float(np.finfo(np.float32).max), float(np.finfo(np.float32).max)))
    for n in (1, 2, 3):
        x = rng.standard_normal(n).astype(np.float32)
        out.append((f"N{n}", R.histogram(x, m)[0], float(x.min()), float(x.max())))
    c = rng.integers(0, 1 << 40, 2 * nb).astype(np.int64) * (rng.random(2 * nb) < 0.01)       # sparse, counts past 32 bits
    c[: nb - 1 - (254 << m) - ((1 << m) - 1)] = 0
    c[nb + (255 << m):] = 0
    nz = np.nonzero(c)[0]
    out.append(("huge", c, float(np.nextafter(lo[nz[0]], np.float32(np.inf))), float(np.nextafter(hi[nz[-1]], np.float32(-np.inf)))))
    return out


@pytest.mark.parametrize("m", MS)
def test_percentile_range_equals_the_reference(m):
    from mobilequant_amd.calibration import percentile_range
    for name, c, mn, mx in _count_vectors(m):
        for p in (1.0, 0.9999, 0.999, 0.99, 0.9, 0.5, 0.34, 1e-9):
            got = percentile_range(c, mn, mx, p, m)
            want = R.percentile_range(c, mn, mx, p, m)
            assert isinstance(got[0], float) and isinstance(got[1], float)
            assert (np.float32(got[0]), np.float32(got[1])) == want and got == (float(want[0]), float(want[1])), (name, p, got, want)
            assert got[0] <= got[1] and np.float32(mn) <= got[0] and got[1] <= np.float32(mx), (name, p, got)
        assert percentile_range(c, mn, mx, 1.0, m) == (float(np.float32(mn)), float(np.float32(mx))), name    # p = 1: today's [min, max]
        assert percentile_range(torch.from_numpy(c), mn, mx, 0.99, m) == percentile_range(c.tolist(), mn, mx, 0.99, m)


@pytest.mark.parametrize("m", MS)
def test_percentile_range_keeps_its_coverage(m):
    """At least N - 2 tail of the counted values lie inside the result (the histogram and the range both from the reference data)."""
    from mobilequant_amd.calibration import percentile_range
    rng = np.random.default_rng(7)
    for n, scale in ((100003, 1.0), (2049, 30.0), (17, 1e-3)):
        x = (rng.standard_normal(n) * scale).astype(np.float32)
        x[:4] = np.array([40.0, -40.0, 55.0, -55.0], np.float32) * np.float32(scale)
        c, _ = R.histogram(x, m)
        for p in (1.0, 0.9999, 0.999, 0.99, 0.9, 0.5):
            lo, hi = percentile_range(c, float(x.min()), float(x.max()), p, m)
            _, _, tail, total = R.percentile_bins(c, p)
            inside = int(((x >= np.float32(lo)) & (x <= np.float32(hi))).sum())
            assert total == n and inside >= n - 2 * tail, (n, p, inside, tail)
    if m == 5:          # the worked example of the rule: 100 003 N(0, 1) values with planted +-40 / +-55, p = 0.999
        x = np.random.default_rng(0).standard_normal(100003).astype(np.float32)
        x[:4] = [40.0, -40.0, 55.0, -55.0]
        lo, hi = percentile_range(R.histogram(x, 5)[0], float(x.min()), float(x.max()), 0.999, 5)
        assert -4.0 < lo < -3.0 and 3.0 < hi < 4.0 and lo * 32 == int(lo * 32) and hi * 32 == int(hi * 32)    # clipped, on bin bounds


def test_percentile_range_argument_errors():
    from mobilequant_amd.calibration import histogram_bin_bounds, percentile_range
    c = np.ones(2 * R.nb_of(3), np.int64)
    for p in (0.0, -0.1, 1.0001, float("nan"), None, "0.9"):
        with pytest.raises(ValueError):
            percentile_range(c, -1.0, 1.0, p, 3)
    with pytest.raises(ValueError):
        percentile_range(c, -1.0, 1.0, 0.9, 5)          # 4096 counts are not a 16384-bin histogram
    for m in (-1, 7, 2.0):
        with pytest.raises(ValueError):
            histogram_bin_bounds(m)


def test_hist_argument_checks_fail_before_any_launch():
    """Null pointers, mantissa_bits outside 0..6 and a dtype other than fp32 / fp16 return MQ_EINVAL with a message before any HIP
    call: checkable without a GPU.  Pointers are fake, aligned and never dereferenced."""
    from mobilequant_amd import _lib as L
    lib = L.load()
    p = ctypes.c_void_p(0x10000)
    f = lib.mq_hist_minmax_tensor
    assert f(p, L.MQ_F32, 100, 5, None, p, p, p, None) == 1 and b"null pointer" in lib.mq_last_error()
    assert f(p, L.MQ_F32, 100, 5, p, None, p, p, None) == 1 and b"null pointer" in lib.mq_last_error()
    assert f(None, L.MQ_F32, 100, 5, p, p, p, p, None) == 1 and b"null pointer" in lib.mq_last_error()
    assert f(p, L.MQ_F32, 100, 5, p, p, None, p, None) == 1 and b"pair" in lib.mq_last_error()
    assert f(p, L.MQ_F32, 100, 5, p, p, p, None, None) == 1 and b"pair" in lib.mq_last_error()
    for m in (-1, 7):
        assert f(p, L.MQ_F32, 100, m, p, p, p, p, None) == 1 and b"mantissa_bits" in lib.mq_last_error()
    for dt in (L.MQ_I8, L.MQ_I32, 17):
        assert f(p, dt, 100, 5, p, p, p, p, None) == 1 and b"dtype" in lib.mq_last_error()
    assert f(p, L.MQ_F32, -1, 5, p, p, p, p, None) == 1 and f(p, L.MQ_F32, (1 << 40) + 1, 5, p, p, p, p, None) == 1 and b"numel" in lib.mq_last_error()
    assert f(None, L.MQ_F16, 0, 6, p, p, None, None, None) == 0          # an empty tensor: no launch, nothing touched
    with pytest.raises(L.MobileQuantLibraryError, match="mantissa_bits=9"):
        L.call("mq_hist_minmax_tensor", p, L.MQ_F32, 4, 9, p, p, p, p, None)


def test_torch_op_is_registered_with_a_meta_kernel():
    import mobilequant_amd.torch_ops as T
    assert "hist_minmax_update_" in T.OPS
    op = torch.ops.mobilequant_amd.hist_minmax_update_
    e = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device="meta")       # noqa: E731
    assert op(e(4096, dt=torch.int64), e(1, dt=torch.int64), e(2, 1), e(8, 8), 3) is None
    with pytest.raises(NotImplementedError):                                       # no CPU implementation here either
        op(torch.zeros(4096, dtype=torch.int64), torch.zeros(1, dtype=torch.int64), torch.zeros(2, 1), torch.zeros(8, 8), 3)


def test_collector_argument_errors():
    from mobilequant_amd.calibration import ActRangeCollector, get_act_range
    model = CalibToy()
    with pytest.raises(ValueError, match="per_channel"):
        ActRangeCollector(model, per_channel=True, device="cpu", method="percentile", percentile=0.99)
    for p in (0.0, -0.5, 1.5, float("nan"), None, "0.9"):
        with pytest.raises(ValueError, match="percentile"):
            ActRangeCollector(model, device="cpu", method="percentile", percentile=p)
    with pytest.raises(ValueError, match="method"):
        ActRangeCollector(model, device="cpu", method="entropy")
    with pytest.raises(ValueError, match="mantissa_bits"):
        ActRangeCollector(model, device="cpu", method="percentile", percentile=0.99, mantissa_bits=7)
    with pytest.raises(ValueError, match="percentile"):
        ActRangeCollector(model, device="cpu", percentile=0.99)          # read by method="percentile" only
    with pytest.raises(ValueError, match="method"):
        get_act_range(model, [], method="median")
    col = ActRangeCollector(model, device="cpu", method="percentile", percentile=lambda name, field: 2.0)
    col._mn[0], col._mx[0], col._cnt[0, 5000] = -1.0, 1.0, 3
    with pytest.raises(ValueError, match="percentile"):                  # a callable's answer is checked where it is used
        col.act_dict()
    # percentile mode runs the plain forward under the hooks: the fused statistics passes are off
    col = ActRangeCollector(model, device="cpu", method="percentile", percentile=1.0)
    assert col.fuse_layer_statistics is False and col.fuse_attention_statistics is False
    assert not col.can_fuse_layer(torch.zeros(4, 8)) and not col.can_fuse_attention((1, 4, 8, 8), torch.float32, col.device, None)
    assert col._cnt.shape == (len(col.slots), 16384) and col._cnt.dtype == torch.int64 and col.act_dict() == {}


# ---- the data-parallel path on CPU ranks -----------------------------------------------------------------------------------------
def _cpu_stand_ins(patch=setattr):
    """numpy stand-ins for the device ops get_act_range launches (covered on the GPU by test_gpu_hist.py), so that the whole path -- hooks
    on a model, round-robin shards, a rank without a sample, both collectives -- runs on CPU ranks."""
    from mobilequant_amd import ops

    def tensor_(x, mn, mx):
        mn.copy_(torch.minimum(mn, x.amin().reshape(1).float()))
        mx.copy_(torch.maximum(mx, x.amax().reshape(1).float()))

    def hist_(t, counts_row, nan_row, mn, mx, mantissa_bits):
        c, n = R.histogram(t.detach().contiguous().numpy(), mantissa_bits)
        counts_row += torch.from_numpy(c)
        nan_row += n
        tensor_(t, mn, mx)
    patch(ops, "minmax_tensor_", tensor_)
    patch(ops, "hist_minmax_tensor_", hist_)


def _model():
    torch.manual_seed(3)
    return CalibToy().eval().requires_grad_(False)


def _samples(n):
    g = torch.Generator().manual_seed(9)
    return [torch.randint(0, 50, (2, 24), generator=g) for _ in range(n)]


P = 0.9


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, method, n_samples, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        _cpu_stand_ins()
        from mobilequant_amd.calibration import get_act_range
        calls = {"all_reduce": 0, "other": 0}
        real, real_gather = dist.all_reduce, dist.all_gather_object

        def counting(*a, **k):
            calls["all_reduce"] += 1
            return real(*a, **k)

        def counting_gather(*a, **k):
            calls["other"] += 1
            return real_gather(*a, **k)
        dist.all_reduce, dist.all_gather_object = counting, counting_gather
        kw = dict(method="percentile", percentile=P) if method == "percentile" else {}
        act = get_act_range(_model(), _samples(n_samples), **kw)
        dist.all_reduce, dist.all_gather_object = real, real_gather
        q.put((rank, act, calls["all_reduce"], calls["other"]))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,method,n_samples", [(2, "percentile", 5), (2, "minmax", 5), (3, "percentile", 2)])
def test_gloo_ranks_equal_the_single_process_run(world, method, n_samples, monkeypatch):
    """Histograms merge by integer addition: every rank ends with exactly the dict a single process computes over all samples, after
    the MAX collective and ONE SUM collective (minmax mode: still one collective).  Three ranks over two samples: the rank without a
    sample runs none (counts are not idempotent) and still holds the same dict."""
    _cpu_stand_ins(monkeypatch.setattr)
    from mobilequant_amd.calibration import get_act_range
    kw = dict(method="percentile", percentile=P) if method == "percentile" else {}
    want = get_act_range(_model(), _samples(n_samples), **kw)
    plain = get_act_range(_model(), _samples(n_samples))
    assert want.keys() == plain.keys() and len(want) == 5 and all(isinstance(v, float) for d in want.values() for r in d.values() for v in r)
    if method == "percentile":          # the coverage clips: inside the observed extremes everywhere, strictly somewhere
        assert all(plain[n][f][0] <= want[n][f][0] <= want[n][f][1] <= plain[n][f][1] for n in want for f in want[n])
        assert sum(want[n][f] != plain[n][f] for n in want for f in want[n]) >= 8
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, method, n_samples, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=180) for _ in procs), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, act, n_ar, n_other in res:
        assert n_ar == (2 if method == "percentile" else 1) and n_other == 0, (rank, n_ar, n_other)
        assert act == want, (rank, [(n, f) for n in want for f in want[n] if act.get(n, {}).get(f) != want[n][f]][:5])


def test_collector_counts_its_collectives_and_reports_clipping(monkeypatch):
    """n_collectives on the collector itself (a forced 1-rank group), histogram() and clip_report() against the reference."""
    _cpu_stand_ins(monkeypatch.setattr)
    from mobilequant_amd.calibration import ActRangeCollector
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", str(_free_port()))
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        seen = {}
        model = _model()
        hooks = [m.register_forward_hook(lambda mod, xx, y, name=name: seen.setdefault(name, []).append((xx, y)))
                 for name, m in model.named_modules() if name in ("fc1", "act", "fc2", "bmm", "ln")]
        cols = {meth: ActRangeCollector(model, device="cpu", **kw).attach()
                for meth, kw in (("percentile", dict(method="percentile", percentile=P)), ("minmax", {}))}
        for s in _samples(3):
            model(s)
        for h in hooks:
            h.remove()
        for meth, col in cols.items():
            col.detach()
            col.all_reduce(force=True)
            assert col.n_collectives == (2 if meth == "percentile" else 1)
        col = cols["percentile"]
        rep, act = col.clip_report(), col.act_dict()
        assert rep.keys() == act.keys() == cols["minmax"].act_dict().keys()
        for name, calls in seen.items():
            tensors = {"input": [c[0][0] for c in calls], "output": [c[1] for c in calls]}
            if name == "bmm":
                tensors["input2"] = [c[0][1] for c in calls]
            assert rep[name].keys() == tensors.keys()
            for field, ts in tensors.items():
                x = np.concatenate([t.detach().contiguous().numpy().reshape(-1) for t in ts])
                c, n = R.histogram(x, 5)
                got_c, got_n = col.histogram(name, field)
                assert got_c.dtype == torch.int64 and np.array_equal(got_c.numpy(), c) and got_n == n == 0
                lo, hi = R.percentile_range(c, x.min(), x.max(), P, 5)
                r = rep[name][field]
                assert act[name][field] == [r["lo"], r["hi"]] == [float(lo), float(hi)]
                assert [r["min"], r["max"]] == cols["minmax"].act_dict()[name][field] == [float(x.min()), float(x.max())]
                assert r["clipped_low"] == int((x < lo).sum()) and r["clipped_high"] == int((x > hi).sum()) and r["nan"] == 0
                assert r["clipped_low"] <= R.percentile_bins(c, P)[2] >= r["clipped_high"]
    finally:
        dist.destroy_process_group()
