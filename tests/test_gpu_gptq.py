"""mq_gptq_round on the GPU against the numpy restatement of its contract (gptq_ref.py): index, w_deq and loss bit for bit on every case of
the table, every row the same alone and at another position of a launch, each optional output without influence on the others, a
captured graph replayed with rewritten weights; then gptq_quantize_model on the toy LM (sim model, weight-only, after a clip search)."""
import copy
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gptq_ref as R  # noqa: E402
from gpu_buffers import Buf, check_bits  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


class Launch:
    """One call of the C entry: inputs as device tensors, every output between canary bytes."""

    def __init__(self, dev, w, scale, offset, qmin, qmax, u, g, perm, want_deq=True, want_loss=True):
        from mobilequant_amd import _lib
        t = lambda a: torch.from_numpy(np.array(a)).to(dev)      # noqa: E731  (a copy: the shared inputs are read-only)
        N, K = w.shape
        self.N, self.K = N, K
        self.w, self.s, self.o, self.u = t(w), t(scale), t(offset), t(u)
        self.perm = None if perm is None else t(perm)
        nbytes = int(_lib.load().mq_gptq_workspace_bytes(N, K))
        assert nbytes > 0
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.index = Buf(dev, N * K, data=np.full(N * K, 0xA5, np.uint8))
        self.deq = Buf(dev, N * K * 4, fill=F32(-7.0)) if want_deq else None
        self.loss = Buf(dev, N * 8, data=np.full(N, -3.0, np.float64)) if want_loss else None
        a = self.a = _lib.MqGptqArgs()
        a.w, a.N, a.K, a.group_size = self.w.data_ptr(), N, K, g
        a.scale, a.offset, a.qmin, a.qmax = self.s.data_ptr(), self.o.data_ptr(), float(qmin), float(qmax)
        a.u, a.perm = self.u.data_ptr(), (None if perm is None else self.perm.data_ptr())
        a.workspace, a.workspace_bytes = self.ws.data_ptr(), nbytes
        a.index = self.index.ptr
        a.w_deq = self.deq.ptr if want_deq else None
        a.loss = self.loss.ptr if want_loss else None

    def run(self):
        from mobilequant_amd import _lib
        _lib.call("mq_gptq_round", ctypes.byref(self.a), torch.cuda.current_stream().cuda_stream)

    def take(self):
        torch.cuda.synchronize()
        idx = self.index.take(np.uint8, "index").reshape(self.N, self.K)
        deq = None if self.deq is None else self.deq.take(F32, "w_deq").reshape(self.N, self.K)
        loss = None if self.loss is None else self.loss.take(np.float64, "loss")
        return idx, deq, loss


def _launch_case(dev, i, rows=None, **kw):
    c, d = R.CASES[i], R.inputs(i)
    sel = slice(None) if rows is None else rows
    L = Launch(dev, d["w"][sel], d["scale"][sel], d["offset"][sel], d["qmin"], d["qmax"], d["u"], c["g"], d["perm"], **kw)
    L.run()
    return L.take()


def _same_loss(got, want):
    return np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(want)].view(np.uint64), want[~np.isnan(want)].view(np.uint64))


def _check(got, want, w, what):
    idx, deq, loss = got
    widx, wdeq, wloss = want
    bad = np.argwhere(idx != widx)
    assert len(bad) == 0, "%s: %d of %d indices differ, first at %r: got %d want %d" % (
        what, len(bad), idx.size, tuple(bad[0]), idx[tuple(bad[0])], widx[tuple(bad[0])])
    if deq is not None:
        check_bits(deq, wdeq, w, what + " w_deq")
    if loss is not None:
        assert _same_loss(loss, wloss), (what, loss, wloss)


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=[R.case_id(c) for c in R.CASES])
def test_bit_equal_to_the_contract(dev, i):
    want = R.reference(i)
    _check(_launch_case(dev, i), want, R.inputs(i)["w"], R.case_id(R.CASES[i]))


def _probe_rows(N):
    return list(range(N)) if N <= 9 else sorted({0, 1, R.STRIP - 2, R.STRIP - 1, R.STRIP, N - 1} & set(range(N)))


@pytest.mark.parametrize("i", [i for i, c in enumerate(R.CASES) if c["N"] > 1], ids=[R.case_id(c) for c in R.CASES if c["N"] > 1])
def test_a_row_is_the_same_alone_and_at_any_position(dev, i):
    c = R.CASES[i]
    widx, wdeq, wloss = R.reference(i)
    w = R.inputs(i)["w"]
    for r in _probe_rows(c["N"]):
        _check(_launch_case(dev, i, rows=slice(r, r + 1)), (widx[r:r + 1], wdeq[r:r + 1], wloss[r:r + 1]), w[r:r + 1], "%s row %d alone" % (R.case_id(c), r))
    order = np.roll(np.arange(c["N"])[::-1], 3)                            # every row at another lane (and, past one strip, another strip)
    _check(_launch_case(dev, i, rows=order), (widx[order], wdeq[order], wloss[order]), w[order], R.case_id(c) + " reordered")


OPTIONAL = [i for i, c in enumerate(R.CASES) if (c["N"], c["K"]) in ((65, 64), (64, 128), (5, 96))]


@pytest.mark.parametrize("i", OPTIONAL, ids=[R.case_id(R.CASES[i]) for i in OPTIONAL])
def test_optional_outputs_do_not_change_the_others(dev, i):
    want = R.reference(i)
    w = R.inputs(i)["w"]
    idx, deq, loss = _launch_case(dev, i, want_deq=False)
    assert deq is None
    _check((idx, None, loss), want, w, "w_deq = NULL")
    idx, deq, loss = _launch_case(dev, i, want_loss=False)
    assert loss is None
    _check((idx, deq, None), want, w, "loss = NULL")
    idx, deq, loss = _launch_case(dev, i, want_deq=False, want_loss=False)
    _check((idx, None, None), want, w, "index alone")


def test_captured_graph_replays_with_rewritten_weights(dev):
    i = next(k for k, c in enumerate(R.CASES) if (c["N"], c["K"]) == (9, 160))      # perm, clipped grid
    c, d = R.CASES[i], R.inputs(i)
    assert c["perm"]
    widx, wdeq, wloss = R.reference(i)
    order = np.arange(c["N"])[::-1].copy()
    L = Launch(dev, d["w"], d["scale"], d["offset"], d["qmin"], d["qmax"], d["u"], c["g"], d["perm"])
    other_s, other_o = torch.from_numpy(d["scale"][order].copy()).to(dev), torch.from_numpy(d["offset"][order].copy()).to(dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        L.run()                                                             # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    _check(L.take(), (widx, wdeq, wloss), d["w"], "eager")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        L.run()
    for rep in range(2):
        rows = order if rep == 0 else np.arange(c["N"])
        L.w.copy_(torch.from_numpy(d["w"][rows].copy()).to(dev))
        L.s.copy_(other_s if rep == 0 else torch.from_numpy(d["scale"].copy()).to(dev))
        L.o.copy_(other_o if rep == 0 else torch.from_numpy(d["offset"].copy()).to(dev))
        L.index.dev_view(torch.uint8).fill_(0xA5)
        graph.replay()
        _check(L.take(), (widx[rows], wdeq[rows], wloss[rows]), d["w"][rows], "replay %d" % rep)


def test_wrapper_zeroes_dead_columns_and_leaves_w_alone(dev):
    from mobilequant_amd import gptq
    i = next(k for k, c in enumerate(R.CASES) if c["dead"])
    c, d = R.CASES[i], R.inputs(i)
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)      # noqa: E731  (a copy: the shared inputs are read-only)
    w = d["w"].copy()
    w[:, d["dead"]] = F32(7.5)                                             # what the wrapper must zero
    wt = t(w)
    res = gptq.gptq_round(wt, t(d["scale"]), t(d["offset"]), d["qmin"], d["qmax"], t(d["u"]), c["g"], t(d["perm"]), t(d["dead"]))
    torch.cuda.synchronize()
    _check((res.index.cpu().numpy(), res.dequantized.cpu().numpy(), res.loss.cpu().numpy()), R.reference(i), d["w"], "wrapper")
    assert np.array_equal(wt.cpu().numpy(), w)
    # gptq_factor on the device: the same dead mask and order, a factor within the host test's bound of the numpy one
    U, perm, dead = gptq.gptq_factor(t(d["H"]), 0.01, True)
    assert U.is_cuda and np.array_equal(dead.cpu().numpy(), d["dead"]) and np.array_equal(perm.cpu().numpy(), d["perm"])
    assert np.abs(U.cpu().numpy().astype(np.float64) - d["u"].astype(np.float64)).max() <= 2.0 ** -22 * np.abs(d["u"]).max()
    empty = gptq.gptq_round(torch.empty(0, 64, device=dev), torch.empty(0, 1, device=dev), torch.empty(0, 1, device=dev), 0, 15, torch.eye(64, device=dev))
    assert empty.index.shape == (0, 64) and empty.loss.shape == (0,)


# ---- model -----------------------------------------------------------------------------------------------------------------------------
def _ids(dev):
    return [x.to(dev) for x in R.toy_calib_ids()]


def _sim_model(dev):
    import mobilequant_amd.quantization.qmodule as Q
    m = Q.create_sim_qmodel(R.toy_model().to(dev), Q.QuantConfig(**R.TOY_CFG), Q.QuantConfig(bitwidth=32))
    return m.eval()


def _qlinears(m):
    import mobilequant_amd.quantization.qmodule as Q
    return {n: mod for n, mod in m.named_modules() if isinstance(mod, Q.QLinear)}


def _grid_of(wq, weight):
    with torch.no_grad():
        wq(weight)
    return wq.scale.detach().clone().reshape(weight.shape[0], -1), wq.offset.detach().clone().reshape(weight.shape[0], -1), int(wq.qmin), int(wq.qmax)


def _expected(dev, before, act_order=False, fp16_scale=False, plain_cfg=None):
    """name -> (GptqResult, scale, offset, qmin, H) from the pieces, on a copy of the model as it stood before the conversion."""
    import mobilequant_amd.quantization.qmodule as Q
    from mobilequant_amd import gptq
    m = copy.deepcopy(before)
    with torch.no_grad(), gptq.HessianCollector(m) as hc:
        for ids in _ids(dev):
            m(ids)
    out = {}
    for name, mod in hc.modules.items():
        w = mod.weight.detach().float().contiguous()
        if isinstance(mod, Q.QLinear):
            if not mod.weight_quantizer.qcfg.is_per_channel:
                continue
            s, o, qmin, qmax = _grid_of(mod.weight_quantizer, w)
        else:
            mn, mx = Q.compute_min_max_from_tensor(w, True, plain_cfg.group_size)
            s, o, _, _, qmin, qmax = Q.compute_scale_offset_from_min_max(mn, mx, plain_cfg.bitwidth, plain_cfg.is_symmetric)
            s, o = s.reshape(w.shape[0], -1), o.reshape(w.shape[0], -1)
        if fp16_scale:
            s = s.half().float()
        H = hc.hessian(name)
        U, perm, dead = gptq.gptq_factor(H, 0.01, act_order)
        out[name] = (gptq.gptq_round(w, s, o, qmin, qmax, U, R.TOY_CFG["group_size"], perm, dead if bool(dead.any()) else None), s, o, qmin, H)
    return out


@pytest.mark.parametrize("act_order", [False, True], ids=["walk", "act_order"])
def test_sim_model_holds_the_gptq_indices(dev, act_order):
    import mobilequant_amd.quantization.qmodule as Q
    from mobilequant_amd import _lib, gptq, ops
    m = _sim_model(dev)
    for mod in _qlinears(m).values():                                      # static grids, set before the conversion
        mod.weight_quantizer.set_scale_offset_from_tensor(mod.weight.detach(), "parameter")
    per_tensor = m.layers[1].mlp.w2
    per_tensor.weight_quantizer.update_qcfg(Q.QuantConfig(bitwidth=4))       # a per-tensor grid: listed, not converted
    w2_before = per_tensor.weight.detach().clone()
    want = _expected(dev, m, act_order)
    rep = gptq.gptq_quantize_model(m, _ids(dev), act_order=act_order)
    print(rep.summary)
    assert len(rep) == R.TOY_LINEARS - 1 and rep.skipped == {"lm_head": "lm_head stays in floating point", "layers.1.mlp.w2": "per-tensor weight grid"}
    assert torch.equal(per_tensor.weight, w2_before)
    g = R.TOY_CFG["group_size"]
    for name, line in rep.items():
        mod = _qlinears(m)[name]
        res, s, o, qmin, H = want[name]
        print(f"{name}: rtn {line.rtn_error:.5g} gptq {line.gptq_error:.5g} ratio {line.gptq_error / line.rtn_error:.3f} "
              f"loss {line.loss_sum:.5g} changed {line.changed_fraction:.3f}")
        assert line.gptq_error < line.rtn_error and 0 < line.changed_fraction < 1 and line.loss_sum == float(res.loss.sum())
        assert torch.equal(mod.weight.detach(), res.dequantized)
        wq = mod.weight_quantizer
        assert not wq.lwc and isinstance(wq.scale, torch.nn.Parameter) and torch.equal(wq.scale.detach().reshape(s.shape), s)
        N, K = mod.weight.shape
        idx = ops.quantize(mod.weight.detach().reshape(-1, g), wq.scale.detach(), wq.offset.detach(), wq.qmin, wq.qmax, q_dtype=_lib.MQ_U8,
                           shift=qmin, rows=N * K // g).view(N, K)
        assert torch.equal(idx, res.index), name                           # Quantizer(weight) IS the GPTQ rounding ...
        assert torch.equal(wq(mod.weight.detach()), mod.weight.detach()), name      # ... and its fake-quant leaves the weight as it is
    with torch.no_grad():
        assert torch.isfinite(m(_ids(dev)[0])).all()


def test_weight_only_model_deploys_the_gptq_indices(dev):
    import mobilequant_amd.quantization.qmodule as Q
    from mobilequant_amd import gptq
    cfg = Q.QuantConfig(**R.TOY_CFG)
    m = R.toy_model().to(dev)
    want = _expected(dev, m, fp16_scale=True, plain_cfg=cfg)
    rep = gptq.gptq_quantize_model(m, _ids(dev), cfg, weight_only=True)
    assert len(rep) == R.TOY_LINEARS and list(rep.skipped) == ["lm_head"]
    kinds = {n: type(mod).__name__ for n, mod in m.named_modules()}
    assert sum(k == "WeightOnlyLinear" for k in kinds.values()) == R.TOY_LINEARS and kinds["lm_head"] == "Linear"
    for name, line in rep.items():
        res, s, o, qmin, H = want[name]
        mod = m.get_submodule(name)
        assert line.gptq_error < line.rtn_error
        zero = o - float(qmin)
        w16 = (s.half().float().repeat_interleave(R.TOY_CFG["group_size"], 1) * (res.index.float() - zero.repeat_interleave(R.TOY_CFG["group_size"], 1))).half()
        assert torch.equal(mod.dequantize(), w16), name
        assert torch.equal(mod.scales, s.half())
    with torch.no_grad():
        assert torch.isfinite(m(_ids(dev)[0])).all()
    # a plain model without w_qcfg: nothing is converted, every linear is listed
    m2 = R.toy_model().to(dev)
    rep2 = gptq.gptq_quantize_model(m2, _ids(dev)[:1])
    assert len(rep2) == 0 and len(rep2.skipped) == R.TOY_LINEARS + 1 and rep2.skipped["layers.0.mlp.w1"] == "a plain nn.Linear needs w_qcfg"


def test_clip_searched_model_goes_through_and_ends_without_lwc(dev):
    import mobilequant_amd.quantization.qmodule as Q
    from mobilequant_amd import gptq
    from mobilequant_amd.quantization.clip_search import search_weight_clipping
    m = _sim_model(dev)
    plain = {n: _grid_of(copy.deepcopy(mod.weight_quantizer), mod.weight.detach().float())[0] for n, mod in _qlinears(m).items()}
    found = search_weight_clipping(m)
    assert len(found) == R.TOY_LINEARS and all(mod.weight_quantizer.lwc for mod in _qlinears(m).values())
    want = _expected(dev, m)
    rep = gptq.gptq_quantize_model(m, _ids(dev))
    assert len(rep) == R.TOY_LINEARS
    clipped = 0
    for name, mod in _qlinears(m).items():
        wq = mod.weight_quantizer
        assert not wq.lwc and not hasattr(wq, "upbound_factor") and not hasattr(wq, "lowbound_factor")
        res, s, o, qmin, H = want[name]
        assert torch.equal(mod.weight.detach(), res.dequantized) and torch.equal(wq.scale.detach().reshape(s.shape), s)
        assert bool((s <= plain[name]).all())
        clipped += int((s < plain[name]).sum())
        assert rep[name].gptq_error < rep[name].rtn_error
    assert clipped > 0                                                     # the grid GPTQ rounded onto is the clipped one
    with torch.no_grad():
        assert torch.isfinite(m(_ids(dev)[0])).all()
