"""mq_hist_minmax_tensor on the GPU against the numpy reference (hist_ref.py, written from the rule): every count, the NaN counter and the
bits of the running min / max; contention, accumulation past 32 bits; the collector's percentile mode on a toy graph; downstream use of
the percentile dict.  Every comparison is exact."""
import functools

import numpy as np
import pytest
import torch

import hist_ref as R

pytestmark = pytest.mark.gpu

NUMELS = (1, 3, 4, 5, 255, 256, 257, 4099, 65543, 2 ** 20 + 13)
MS = (0, 3, 5, 6)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _data(numel, fp16):
    return R.planted_data(numel, 1000 + numel, fp16)


@functools.lru_cache(maxsize=None)
def _want(numel, fp16, m):
    x = _data(numel, fp16)
    return R.histogram(x, m), R.minmax(x)


def _bits(t):
    return t.detach().cpu().view(torch.int32).tolist()


def _run(ops, view, m, counts=None, nan=None, mn=None, mx=None):
    if counts is None:
        counts, nan = ops.hist_new(1, m, view.device)
        mn, mx = ops.minmax_new(1, view.device)
    ops.hist_minmax_tensor_(view, counts[0], nan[0:1], mn, mx, m)
    return counts, nan, mn, mx


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("numel", NUMELS)
@pytest.mark.parametrize("fp16", [False, True], ids=["f32", "f16"])
def test_kernel_equals_the_reference_at_every_alignment(dev, fp16, numel, m):
    """N(0, 1) with planted +-0, denormals, +-inf, NaNs, +-max finite, values on bin bounds and their neighbours; the base pointer offset
    by 0..3 (fp32) / 0..7 (fp16) elements from a 16-byte-aligned allocation: unaligned head, a tail shorter than a vector, one wave, one
    workgroup, several workgroups."""
    from mobilequant_amd import ops
    x = _data(numel, fp16)
    (want_c, want_nan), (want_mn, want_mx) = _want(numel, fp16, m)
    if numel >= 256:
        assert want_nan >= 3 and np.isnan(want_mn)          # the planted NaNs are in
    src = torch.from_numpy(x).to(dev)
    n_off = 8 if fp16 else 4
    buf = torch.zeros(numel + 16, dtype=src.dtype, device=dev)
    assert buf.data_ptr() % 16 == 0
    for off in range(n_off):
        view = buf[off:off + numel]
        view.copy_(src)
        assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + off * src.element_size()
        counts, nan, mn, mx = _run(ops, view, m)
        assert counts.shape == (1, 2 * R.nb_of(m)) and counts.dtype == torch.int64
        assert np.array_equal(counts[0].cpu().numpy(), want_c), (off, int(np.abs(counts[0].cpu().numpy() - want_c).sum()))
        assert int(nan[0]) == want_nan, off
        mn2, mx2 = ops.minmax_new(1, dev)
        ops.minmax_tensor_(view, mn2, mx2)
        assert _bits(mn) == _bits(mn2) and _bits(mx) == _bits(mx2), off                      # NaN sticky, -0 canonical: the same bits
        got = (float(mn), float(mx))
        assert (np.isnan(got[0]) and np.isnan(got[1])) if np.isnan(want_mn) else got == (float(want_mn), float(want_mx)), off
        c2, n2 = ops.hist_new(1, m, dev)                                                     # min / max are nullable as a pair
        ops.hist_minmax_tensor_(view, c2[0], n2[0:1], None, None, m)
        assert torch.equal(c2, counts) and torch.equal(n2, nan), off


@pytest.mark.parametrize("aggregate", [1, 0])
@pytest.mark.parametrize("pattern", ["equal", "alternating", "runs"])
def test_contention_patterns_count_exactly(dev, pattern, aggregate):
    """2^20 equal values (every LDS atomic of a wave on one address); values alternating between two bins; constant runs of odd lengths
    (waves partly uniform).  With and without the wave-uniform aggregation: the same counts."""
    from mobilequant_amd import _lib, ops
    n = 2 ** 20
    if pattern == "equal":
        x = np.full(n, 1.5, np.float32)
    elif pattern == "alternating":
        x = np.where(np.arange(n) % 2 == 0, np.float32(1.5), np.float32(-3.0)).astype(np.float32)
    else:
        x = np.repeat(np.random.default_rng(3).standard_normal(n // 251 + 1).astype(np.float32), 251)[:n]
    want_c, want_nan = R.histogram(x, 5)
    assert want_c.max() >= (n // 2 if pattern != "runs" else 251)
    lib = _lib.load()
    lib.mq_hist_set_aggregate(aggregate)
    try:
        counts, nan, mn, mx = _run(ops, torch.from_numpy(x).to(dev), 5)
        torch.cuda.synchronize()
    finally:
        lib.mq_hist_set_aggregate(1)
    assert np.array_equal(counts[0].cpu().numpy(), want_c) and int(nan[0]) == want_nan == 0
    assert (float(mn), float(mx)) == (float(x.min()), float(x.max()))


def test_calls_accumulate_and_carry_past_32_bits(dev):
    from mobilequant_amd import ops
    m = 5
    a, b = _data(4099, False), _data(65543, True)
    counts, nan, mn, mx = _run(ops, torch.from_numpy(a).to(dev), m)
    _run(ops, torch.from_numpy(b).to(dev), m, counts, nan, mn, mx)
    (ca, na), (cb, nb_) = R.histogram(a, m), R.histogram(b, m)
    assert np.array_equal(counts[0].cpu().numpy(), ca + cb) and int(nan[0]) == na + nb_
    # rows of a larger table: the neighbours stay untouched
    table, nans = ops.hist_new(3, m, dev)
    mn3, mx3 = ops.minmax_new(3, dev)
    x = torch.full((24,), 1.0, device=dev)
    bin1 = R.nb_of(m) + (127 << m)
    table[1, bin1] = 2 ** 32 - 3                                     # a 64-bit counter about to pass 32 bits
    nans[1] = 2 ** 32 - 1
    ops.hist_minmax_tensor_(torch.cat((x, torch.full((5,), float("nan"), device=dev))), table[1], nans[1:2], mn3[1:2], mx3[1:2], m)
    assert int(table[1, bin1]) == 2 ** 32 + 21 and int(nans[1]) == 2 ** 32 + 4
    assert int(table.sum()) == 2 ** 32 + 21 and int(table[0].sum()) == 0 == int(table[2].sum()) and nans.tolist() == [0, 2 ** 32 + 4, 0]
    assert torch.isinf(mn3[[0, 2]]).all() and torch.isinf(mx3[[0, 2]]).all() and _bits(mn3[1:2]) == [-1] and _bits(mx3[1:2]) == [0x7fffffff]
    # an empty tensor leaves everything as it is
    before = table.clone()
    ops.hist_minmax_tensor_(torch.empty(0, device=dev), table[0], nans[0:1], mn3[0:1], mx3[0:1], m)
    assert torch.equal(table, before)


def test_torch_op_is_the_same_kernel(dev):
    import mobilequant_amd.torch_ops  # noqa: F401
    from mobilequant_amd import ops
    x = torch.from_numpy(_data(4099, False)).to(dev)
    counts, nan = ops.hist_new(1, 3, dev)
    running = torch.stack(ops.minmax_new(1, dev))
    torch.ops.mobilequant_amd.hist_minmax_update_(counts[0], nan, running, x, 3)
    (want_c, want_nan), _ = _want(4099, False, 3)
    assert np.array_equal(counts[0].cpu().numpy(), want_c) and int(nan[0]) == want_nan and torch.isnan(running).all()


# ---- the collector on a toy graph whose qk_bmm takes a transposed, non-contiguous operand ---------------------------------------------
def _toy(dev):
    from toy_models import ToyLM
    torch.manual_seed(0)
    return ToyLM().to(dev).eval().requires_grad_(False)


def _toy_samples(n):
    g = torch.Generator().manual_seed(21)
    s = [torch.randn(2, 24, 32, generator=g) for _ in range(n)]
    s[1][0, 3, 5] = 9.0                                               # outliers the coverage is there to clip
    s[2][1, 7, 0] = -11.0
    return s


@pytest.fixture(scope="module")
def toy_run(dev):
    """ONE forward per sample with the collector's hooks and plain torch hooks side by side: the reference sees the very tensors."""
    from mobilequant_amd.calibration import ActRangeCollector, is_calibrated_leaf
    model, samples = _toy(dev), _toy_samples(4)
    seen = {}

    def grab(name):
        def fn(mod, xx, y):
            d = seen.setdefault(name, {"input": [], "output": [], "input2": []})
            d["input"].append(xx[0].detach().cpu().numpy().reshape(-1))          # (.cpu() of a transposed view keeps its values)
            d["output"].append(y.detach().cpu().numpy().reshape(-1))
            if len(xx) > 1:
                d["input2"].append(xx[1].detach().cpu().numpy().reshape(-1))
        return fn
    hooks = [mod.register_forward_hook(grab(name)) for name, mod in model.named_modules() if is_calibrated_leaf(name, mod)]
    col = ActRangeCollector(model, method="percentile", percentile=0.99).attach()
    noncontig = []
    hooks.append(model.layers[0].qk_bmm.register_forward_hook(lambda mod, xx, y: noncontig.append(not xx[1].is_contiguous())))
    with torch.no_grad():
        for s in samples:
            model(s.to(dev))
    col.detach()
    for h in hooks:
        h.remove()
    assert noncontig and all(noncontig)
    ref = {}
    for name, d in seen.items():
        for field, parts in d.items():
            if parts:
                x = np.concatenate(parts)
                ref[(name, field)] = (R.histogram(x, 5), R.minmax(x))
    return model, samples, col, ref


def test_collector_percentile_one_is_the_minmax_dict(dev, toy_run):
    from mobilequant_amd.calibration import get_act_range
    model, samples, _, _ = toy_run
    want = get_act_range(model, samples)
    got = get_act_range(model, samples, method="percentile", percentile=1.0)
    assert len(want) >= 20 and got == want
    assert get_act_range(model, samples, method="percentile", percentile=1.0, mantissa_bits=0) == want


def test_collector_percentile_equals_the_host_reference(dev, toy_run):
    model, samples, col, ref = toy_run
    act, rep = col.act_dict(), col.clip_report()
    assert {(n, f) for n in act for f in act[n]} == set(ref) and len(ref) >= 50
    clipped = 0
    for (name, field), ((c, nan), (mn, mx)) in ref.items():
        got_c, got_nan = col.histogram(name, field)
        assert np.array_equal(got_c.numpy(), c) and got_nan == nan == 0, (name, field)
        lo, hi = R.percentile_range(c, mn, mx, 0.99, 5)
        assert act[name][field] == [float(lo), float(hi)], (name, field)
        r = rep[name][field]
        assert (r["min"], r["max"], r["lo"], r["hi"], r["nan"]) == (float(mn), float(mx), float(lo), float(hi), 0)
        clipped += (r["clipped_low"] > 0) + (r["clipped_high"] > 0)
    assert clipped >= len(ref)                                        # the coverage does clip on this data


def test_histograms_of_shards_add_up(dev, toy_run):
    from mobilequant_amd.calibration import ActRangeCollector
    model, samples, col, _ = toy_run

    def collect(part):
        c = ActRangeCollector(model, method="percentile", percentile=0.99).attach()
        with torch.no_grad():
            for s in part:
                model(s.to(dev))
        c.detach()
        return c
    for cut in (2, 1):
        a, b = collect(samples[:cut]), collect(samples[cut:])
        for key in col.slots:
            (ca, na), (cb, nb_), (cw, nw) = a.histogram(*key), b.histogram(*key), col.histogram(*key)
            assert torch.equal(ca + cb, cw) and na + nb_ == nw, (cut, key)


def test_callable_percentile_is_honoured_per_slot(dev, toy_run):
    from mobilequant_amd.calibration import get_act_range
    model, samples, _, _ = toy_run
    full = get_act_range(model, samples)
    p90 = get_act_range(model, samples, method="percentile", percentile=0.9)
    asked = []

    def choose(name, field):
        asked.append((name, field))
        return 1.0 if ("qk_bmm" in name or field == "input") else 0.9
    got = get_act_range(model, samples, method="percentile", percentile=choose)
    assert got.keys() == full.keys() and set(asked) == {(n, f) for n in full for f in full[n]}
    n_full = n_p90 = 0
    for n in full:
        for f in full[n]:
            keep = "qk_bmm" in n or f == "input"
            assert got[n][f] == (full if keep else p90)[n][f], (n, f)
            assert p90[n][f] != full[n][f]
            n_full, n_p90 = n_full + keep, n_p90 + (not keep)
    assert n_full >= 10 and n_p90 >= 10


def test_alias_mirroring_shares_histograms(dev):
    """A graph that declares its alias groups (llama.LlamaForCausalLM): after the first pass has found the members equal -- extremes AND
    count rows -- the later passes reduce the first member only; every slot ends with the histogram it would have taken itself."""
    from mobilequant_amd.calibration import ActRangeCollector
    from mobilequant_amd.llama import LlamaForCausalLM, LlamaShape
    model = LlamaForCausalLM(LlamaShape(hidden=64, layers=2, heads=4, kv_heads=2, head_dim=16, ffn=128, vocab=50, max_pos=32))
    model.reset_parameters(seed=11, std=0.2)
    model = model.to(dev).eval().requires_grad_(False)
    g = torch.Generator().manual_seed(5)
    samples = [torch.randint(0, 50, (1, 24), generator=g) for _ in range(3)]
    on = ActRangeCollector(model, method="percentile", percentile=0.99)
    off = ActRangeCollector(model, method="percentile", percentile=0.99)
    off.mirror_declared_aliases = False
    on.attach(), off.attach()
    with torch.no_grad():
        for s in samples:
            model(s.to(dev))
    on.detach(), off.detach()
    assert len(on._mirror) >= 10 and on.bytes_aliased > 0 and not off._mirror and off.bytes_aliased == 0 and on.bytes_fused == 0
    for key in on.slots:
        (ca, na), (cb, nb_) = on.histogram(*key), off.histogram(*key)
        assert torch.equal(ca, cb) and na == nb_ == 0 and int(ca.sum()) > 0, key
    assert on.act_dict() == off.act_dict() and on.clip_report() == off.clip_report()
    # the masked zeros of the causal probabilities are counted: the hook sees them
    c, _ = on.histogram("layers.0.self_attn.pv_bmm", "input")
    assert int(c[R.nb_of(5)]) >= 3 * 4 * (24 * 23 // 2)


def test_percentile_dict_feeds_the_quantized_model(dev, toy_run):
    import mobilequant_amd as mq
    model, samples, col, _ = toy_run
    act = col.act_dict()
    m = _toy(dev)
    m.load_state_dict(model.state_dict())
    a8 = mq.QuantConfig(bitwidth=8)
    mq.create_sim_qmodel(m, a8, a8)
    mq.set_scale_and_offset(m, act, "buffer")
    with torch.no_grad():
        y = m(samples[0].to(dev))
        want = model(samples[0].to(dev))
    assert y.shape == want.shape and bool(torch.isfinite(y).all())
