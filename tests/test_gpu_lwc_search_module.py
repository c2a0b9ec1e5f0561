"""Quantizer.search_lwc, search_weight_clipping and torch.ops.mobilequant_amd.lwc_search on the GPU: what the search scored is what the
quantizer's own LWC forward then computes (bit for bit against the oracle at the chosen factors, and the reported cost is the forward's
error), the result is never worse than enable_lwc's state, the model helper searches the eligible QLinears and lists the others, folding
leaves plain clamped weights and a model that runs fused."""
import numpy as np
import pytest
import torch

import lwc_search_ref as R
from oracle import mq_oracle as O

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


def _qlinear(dev, n, k, group_size=-1, bits=4, sym=False, seed=0):
    import mobilequant_amd as mq
    wcfg = mq.QuantConfig(bitwidth=bits, is_per_channel=True, is_symmetric=sym, group_size=group_size)
    lin = mq.QLinear(dict(in_features=k, out_features=n, bias=False), None, wcfg, None)
    lin.weight.data = torch.from_numpy(R.make_weight(n, k, 300 + seed + n))
    return lin.to(dev).requires_grad_(False)


def _row_costs(y, w2):
    e = (np.asarray(y, F32).reshape(w2.shape) - w2).astype(F32).astype(np.float64)
    return np.array([np.sum(r) for r in e * e])


@pytest.mark.parametrize("n,k,g,sym", [(64, 256, -1, False), (16, 512, 128, False), (64, 256, -1, True), (16, 512, 128, True)],
                         ids=["64x256", "16x512g128", "64x256-sym", "16x512g128-sym"])
def test_what_was_scored_is_what_runs(dev, n, k, g, sym):
    lin = _qlinear(dev, n, k, g, sym=sym)
    wq, w = lin.weight_quantizer, lin.weight
    rep = wq.search_lwc(w)
    cols = k if g == -1 else g
    rows = n * k // cols
    assert rep.rows == rows and wq.lwc and wq.upbound_factor.shape == wq.lowbound_factor.shape == (rows, 1)
    assert isinstance(wq.upbound_factor, torch.nn.Parameter) and wq.upbound_factor.dtype == torch.float32
    assert 0 < rep.clipped_rows <= rows                                    # Student-t rows at 4 bits: clipping pays (the issue's sketch)
    w2 = w.detach().cpu().numpy().reshape(rows, cols)
    up, low = wq.upbound_factor.detach(), wq.lowbound_factor.detach()
    assert int((up != 4.0).sum()) == rep.clipped_rows and torch.equal(up, low)          # joint mode
    # the module's own LWC forward at the chosen factors == the oracle at the device's sigmoids of those factors, bit for bit
    y = wq(w).detach().cpu().numpy()
    sig_hi, sig_lo = torch.sigmoid(up).cpu().numpy().reshape(-1), torch.sigmoid(low).cpu().numpy().reshape(-1)
    want = O.lwc_fused_forward(w2, sig_lo, sig_hi, 4, sym)["y"]
    assert np.array_equal(y.reshape(rows, cols).view(np.uint32), want.view(np.uint32))
    # closure: the forward's error is the reported best cost
    got_rows = _row_costs(y, w2)
    tol = R.TOL(cols)
    assert abs(got_rows.sum() - rep.best_cost) <= 2 * tol * rep.best_cost, (got_rows.sum(), rep.best_cost)
    # a second quantizer with plain enable_lwc reproduces the base cost, row by row never better than the searched one
    lin0 = _qlinear(dev, n, k, g, sym=sym)
    lin0.weight_quantizer.enable_lwc(lin0.weight)
    base_rows = _row_costs(lin0.weight_quantizer(lin0.weight).detach().cpu().numpy(), w2)
    assert abs(base_rows.sum() - rep.base_cost) <= 2 * tol * rep.base_cost
    assert rep.best_cost <= rep.base_cost
    assert (got_rows <= base_rows * (1 + 2 * tol)).all()
    # the kernel's per-row report says the same
    from mobilequant_amd import ops
    f = torch.as_tensor(__import__("mobilequant_amd").lwc_factor_table()).to(dev)
    idx, best, base = ops.lwc_search(w.detach().reshape(rows, cols).contiguous(), torch.sigmoid(f), torch.sigmoid(f), 4, sym)
    assert torch.equal(f[idx.long()].reshape(-1, 1), up) and bool((best <= base).all())
    assert np.allclose(best.cpu().numpy(), got_rows, rtol=2 * tol, atol=0) and np.allclose(base.cpu().numpy(), base_rows, rtol=2 * tol, atol=0)
    assert float(best.sum()) == rep.best_cost and float(base.sum()) == rep.base_cost


def test_independent_mode_and_explicit_factors(dev):
    lin = _qlinear(dev, 32, 256, seed=3)
    wq, w = lin.weight_quantizer, lin.weight
    joint = wq.search_lwc(w, n_grid=32)
    indep = wq.search_lwc(w, mode="independent")                         # LWC already on: the factors are overwritten
    assert indep.base_cost == joint.base_cost and indep.best_cost <= joint.best_cost          # the diagonal of the cross product is the joint table
    assert not torch.equal(wq.upbound_factor, wq.lowbound_factor)
    table = set(__import__("mobilequant_amd").lwc_factor_table(32).tolist())
    assert set(wq.upbound_factor.flatten().tolist()) <= table and set(wq.lowbound_factor.flatten().tolist()) <= table
    one = wq.search_lwc(w, factors=torch.tensor([4.0]))
    assert one.clipped_rows == 0 and one.best_cost == one.base_cost == joint.base_cost and bool((wq.upbound_factor == 4.0).all())


def _toy_sim(dev):
    import mobilequant_amd as mq
    from toy_models import ToyLM
    torch.manual_seed(0)
    m = ToyLM().eval().requires_grad_(False)
    mq.create_sim_qmodel(m, mq.QuantConfig(bitwidth=8), mq.QuantConfig(bitwidth=8))
    for name, mod in m.named_modules():
        if isinstance(mod, mq.QLinear):
            if name.endswith(("q_proj", "w2")):
                mod.weight_quantizer.update_qcfg(mq.QuantConfig(bitwidth=4, is_per_channel=True))
            elif name.endswith("w1"):
                mod.weight_quantizer.update_qcfg(mq.QuantConfig(bitwidth=4, is_per_channel=True, group_size=16))
            elif name.endswith("k_proj"):
                mod.weight_quantizer.update_qcfg(mq.QuantConfig(bitwidth=16, is_per_channel=True))
    return m.to(dev)


def test_model_helper_searches_the_eligible_and_lists_the_rest(dev):
    import mobilequant_amd as mq
    m = _toy_sim(dev)
    scales = {f"layers.{i}.{n}_input": torch.rand(32 if n != "w2" else 48, device=dev) + 0.1 for i in range(2) for n in ("q_proj", "w1", "w2")}
    res = mq.search_weight_clipping(m, act_scales=scales)
    want = {f"layers.{i}.{n}" for i in range(2) for n in ("q_proj", "w1", "w2")}
    assert set(res) == want and all(isinstance(r, mq.LwcSearchReport) for r in res.values())
    assert res["layers.0.w1"].rows == 48 * 32 // 16 and res["layers.0.w2"].rows == 32
    sk = res.skipped
    assert "per-tensor" in sk["layers.0.v_proj"] and "16-bit" in sk["layers.1.k_proj"] and "per-tensor" in sk["layers.1.w3"]
    assert "not a QLinear" in sk["layers.0.input_layernorm"] and len(sk) == 2 * (4 + 2)
    assert not (set(sk) & want) and "6 QLinear weights searched" in res.summary
    # the weighted cost of one layer is the helper's at the chosen candidate
    lin = m.layers[1].w1
    w2 = lin.weight.detach().cpu().numpy().reshape(-1, 16)
    cw = (scales["layers.1.w1_input"] ** 2).cpu().numpy()
    sig = torch.sigmoid(mq.lwc_factor_table().to(dev)).cpu().numpy()
    costs = R.cost_table(w2, sig, sig, 4, False, cw)
    idx = R.first_min(costs)
    rep = res["layers.1.w1"]
    assert abs(costs[np.arange(len(idx)), idx].sum() - rep.best_cost) <= 2 * R.TOL(16) * rep.best_cost
    assert abs(costs[:, 0].sum() - rep.base_cost) <= 2 * R.TOL(16) * rep.base_cost and rep.clipped_rows == int((idx != 0).sum())
    assert torch.equal(lin.weight_quantizer.upbound_factor.flatten().cpu(), mq.lwc_factor_table()[torch.from_numpy(idx).long()])


def test_fold_leaves_clamped_weights_and_a_model_that_runs_fused(dev):
    import mobilequant_amd as mq
    m = _toy_sim(dev)
    before = {n: mod.weight.detach().clone() for n, mod in m.named_modules() if isinstance(mod, mq.QLinear)}
    res = mq.search_weight_clipping(m)                                   # first without fold: read the chosen factors
    chosen = {n: (m.get_submodule(n).weight_quantizer.upbound_factor.detach().cpu().numpy(),
                  m.get_submodule(n).weight_quantizer.lowbound_factor.detach().cpu().numpy()) for n in res}
    m2 = _toy_sim(dev)
    res2 = mq.search_weight_clipping(m2, fold=True)
    assert res2 == res and len(res) == 6
    for n, mod in m2.named_modules():
        if not isinstance(mod, mq.QLinear):
            continue
        wq = mod.weight_quantizer
        assert not wq.lwc and not hasattr(wq, "upbound_factor") and not hasattr(wq, "lowbound_factor")
        if n not in res:
            assert torch.equal(mod.weight, before[n])
            continue
        g = wq.qcfg.group_size
        w0 = before[n].cpu().numpy()
        w2 = w0.reshape(-1, g) if g != -1 else w0
        up, low = chosen[n]
        got = mod.weight.detach().cpu().numpy()
        # oracle.run_lwc's two lines at the DEVICE's sigmoids of the chosen factors, bit for bit (oracle.sigmoid_f32 and torch.sigmoid may
        # differ by an ulp, as the oracle says; run_lwc itself, on its own sigmoid, is then within that ulp of the range)
        mn, mx = O.min_max_from_tensor(w2, True, -1)
        dsig = lambda f: torch.sigmoid(torch.from_numpy(f).to(dev)).cpu().numpy()                 # noqa: E731
        want = np.clip(w2, (dsig(low) * mn).astype(F32), (dsig(up) * mx).astype(F32)).astype(F32).reshape(w0.shape)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), n
        assert np.allclose(got, O.run_lwc(w2, up, low, True).reshape(w0.shape), rtol=3e-7, atol=0), n
        assert not np.array_equal(got, w0), n                                                    # the fold did clamp something
    x = torch.randn(2, 24, 32, generator=torch.Generator().manual_seed(4)).to(dev)
    with torch.no_grad():
        plain = m2(x)
        assert mq.fuse_gated_mlp(m2) == 2
        fused = m2(x)
    assert torch.isfinite(fused).all() and fused.shape == plain.shape


def test_torch_op_equals_ops(dev):
    import mobilequant_amd.torch_ops  # noqa: F401
    from mobilequant_amd import ops
    w = torch.from_numpy(R.make_weight(6, 132, 9)).to(dev)
    t = torch.from_numpy(R.ratio_table(16)).to(dev)
    cw = torch.from_numpy(R.make_col_weight(132, "row", 1)).to(dev)
    for weight in (None, cw):
        a = torch.ops.mobilequant_amd.lwc_search(w, t, t, 4, True, weight)
        b = ops.lwc_search(w, t, t, 4, True, weight, return_costs=True)
        assert len(a) == 4 and all(torch.equal(x, y) for x, y in zip(a, b))
