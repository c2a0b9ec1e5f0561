"""CPU: the GPTQ rounding's numpy restatement (tests/gptq_ref.py) does what GPTQ is for, gptq_factor agrees with the float64 factor,
the wrapper and the C entry refuse what they do not serve, and the Hessian collector accumulates what it says.  No GPU."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gptq_ref as R  # noqa: E402
from mobilequant_amd import _lib, gptq, ops  # noqa: E402

F32 = np.float32


def test_launch_constants_are_the_sources():
    assert R.source_constants() == R.CONSTANTS
    assert R.SLICE == R.WAVES * R.CHUNK and R.CHUNK == 16 and R.WAVES * 64 * 2 == R.BLOCK * R.BLOCK


def test_the_case_table_stands_on_both_sides_of_every_switch():
    Ns = {c["N"] for c in R.CASES}
    assert {1, 63, 64, 65, 130} <= Ns
    Ks = {c["K"] for c in R.CASES}
    assert min(Ks) == 16 and max(k for k in Ks if k <= 1024) == 1024 and 4096 in Ks
    assert any(k < R.BLOCK for k in Ks) and R.BLOCK in Ks and any(k % R.BLOCK for k in Ks if k > R.BLOCK)
    trailing = {c["K"] - R.BLOCK for c in R.CASES if c["K"] > R.BLOCK}
    assert any(0 < t < R.SLICE for t in trailing) and R.SLICE in trailing and any(R.SLICE < t < R.SLICE + R.CHUNK for t in trailing)
    assert {t % R.CHUNK for t in trailing} == {0, 4, 8, 12}               # every length of the last chunk
    gs = [(c["g"], c["K"]) for c in R.CASES]
    assert any(g < R.BLOCK for g, _ in gs) and any(g == R.BLOCK for g, _ in gs) and any(R.BLOCK < g < k for g, k in gs) and any(g == k for g, k in gs)
    assert {(c["bits"], c["sym"]) for c in R.CASES} >= {(b, s) for b in (2, 3, 4, 8) for s in (False, True)}
    assert any(c["perm"] and c["g"] <= R.BLOCK and c["K"] > c["g"] for c in R.CASES)        # a perm walk crosses groups inside one block
    assert any(c["clip"] < 1 for c in R.CASES) and any(c["dead"] for c in R.CASES) and any(c["nan"] for c in R.CASES)
    assert any(c["K"] // c["g"] > R.TILE for c in R.CASES) and any(c["K"] > R.TILE and c["K"] % R.TILE for c in R.CASES)
    assert any(c["N"] == 2 and c["K"] == 4096 for c in R.CASES)
    for c in R.CASES:
        assert c["K"] % 4 == 0 and c["g"] % 4 == 0 and c["K"] % c["g"] == 0


def test_perm_cases_walk_across_groups_inside_a_block():
    for i, c in enumerate(R.CASES):
        if c["perm"] and c["g"] < c["K"]:
            p = R.inputs(i)["perm"]
            first = p[:R.BLOCK] // c["g"]
            assert len(set(first.tolist())) > 1, R.case_id(c)


def test_saturating_and_nan_cases_are_what_they_say():
    for i, c in enumerate(R.CASES):
        d = R.inputs(i)
        idx, deq, loss = R.reference(i)
        if c["clip"] < 1:
            top = d["qmax"] - d["qmin"]
            assert ((idx == 0) | (idx == top)).mean() > 0.05, R.case_id(c)
        if c["nan"]:
            r, k = c["N"] // 2, c["K"] // 4
            walk = np.arange(c["K"]) if d["perm"] is None else d["perm"]
            at = int(np.nonzero(walk == k)[0][0])
            assert np.isnan(loss[r]) and not np.isnan(np.delete(loss, r)).any()
            assert np.isnan(deq[r, walk[at:]]).all() and (idx[r, walk[at:]] == 0).all()          # poisons the later columns of its own row
            assert not np.isnan(deq[r, walk[:at]]).any() and not np.isnan(np.delete(deq, r, axis=0)).any()
        if c["dead"]:
            assert (d["w"][:, c["K"] // 3] == 0).all()


FIXTURES = [("t", 64, 256, 64, 4, False), ("t", 96, 512, 128, 4, True), ("t", 32, 256, 256, 3, False),
            ("gauss", 64, 256, 64, 4, False), ("gauss", 48, 384, 128, 4, True), ("gauss", 32, 256, 32, 3, True)]


@pytest.mark.parametrize("dist, N, K, g, bits, sym", FIXTURES)
def test_gptq_lowers_the_layer_objective(dist, N, K, g, bits, sym):
    """tr(dW H dW^T) of the helper's GPTQ weights is below round-to-nearest's, in walk order and with act_order: the bar is 1.0 (a
    condition, not a tolerance); the fixtures are chosen where the ratio stays below about 0.8."""
    seed = 5 * K + N + bits
    w = R.make_weight(N, K, seed, dist)
    H = R.make_hessian(K, seed, tokens=1024)
    s, o, qmin, qmax = R.grid_from_minmax(w, bits, sym, g)
    ridx, rdeq = R.rtn(w, s, o, qmin, qmax, g)
    base = R.objective(rdeq, w, H)
    for act_order in (False, True):
        u, perm, dead, cond = R.factor(H, 0.01, act_order)
        assert not dead.any()
        idx, deq, loss = R.gptq_round(w, s, o, qmin, qmax, u, g, perm)
        ratio = R.objective(deq, w, H) / base
        print(f"{dist} {N}x{K} g{g} w{bits}{'s' if sym else 'a'} act_order={act_order}: objective / rtn = {ratio:.3f}, "
              f"{(idx != ridx).mean():.3f} of the indices changed")
        assert ratio < 1.0
        assert np.isfinite(loss).all() and (loss > 0).all()
        # re-quantizing the dequantized weights returns the indices exactly
        again, _ = R.rtn(deq, s, o, qmin, qmax, g)
        assert np.array_equal(again, idx)


def test_toy_model_linears_gain_on_a_cpu_hessian():
    """What the GPU model test asserts of the kernel holds for the helper: on the toy LM's weights and the Hessians of its own
    calibration inputs (collected on the CPU), every linear's GPTQ objective is below round-to-nearest's."""
    m = R.toy_model()
    with torch.no_grad(), gptq.HessianCollector(m) as hc:
        for ids in R.toy_calib_ids():
            m(ids)
    assert len(hc.modules) == R.TOY_LINEARS and "lm_head" not in hc.modules
    assert hc.shares("layers.0.self_attn.q_proj", "layers.0.self_attn.k_proj") and hc.shares("layers.0.self_attn.q_proj", "layers.0.self_attn.v_proj")
    assert hc.shares("layers.1.mlp.w1", "layers.1.mlp.w3") and not hc.shares("layers.0.mlp.w1", "layers.0.mlp.w2")
    assert not hc.shares("layers.0.self_attn.q_proj", "layers.1.self_attn.q_proj")
    g = R.TOY_CFG["group_size"]
    for name, mod in hc.modules.items():
        assert hc.tokens(name) == 512, name
        w = mod.weight.detach().numpy().astype(F32)
        H = hc.hessian(name).double().numpy()
        s, o, qmin, qmax = R.grid_from_minmax(w, 4, False, g)
        u, perm, dead, _ = R.factor(H, 0.01, False)
        _, deq, _ = R.gptq_round(w, s, o, qmin, qmax, u, g, perm)
        _, rdeq = R.rtn(w, s, o, qmin, qmax, g)
        a, b = R.objective(deq, w, H), R.objective(rdeq, w, H)
        print(f"{name}: {a / b:.3f}")
        assert a < b, name


def test_hessian_collector_is_two_xtx_over_tokens():
    torch.manual_seed(0)
    lin_a, lin_b, head = torch.nn.Linear(24, 8), torch.nn.Linear(24, 12), torch.nn.Linear(8, 5)

    class M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a, self.b, self.lm_head = lin_a, lin_b, head

        def forward(self, x):
            return self.lm_head(self.a(x)) + self.b(x).sum()

    m = M()
    xs = [torch.randn(3, 7, 24), torch.randn(2, 5, 24)]
    with torch.no_grad(), gptq.HessianCollector(m) as hc:
        for x in xs:
            m(x)
    assert sorted(hc.modules) == ["a", "b"] and hc.shares("a", "b") and hc.tokens("a") == 31
    flat = torch.cat([x.reshape(-1, 24) for x in xs]).double()
    want = 2.0 * (flat.t() @ flat) / 31
    assert torch.allclose(hc.hessian("a").double(), want, rtol=1e-5, atol=1e-6)
    with pytest.raises(KeyError):
        hc.hessian("lm_head")
    with gptq.HessianCollector(m, names=["lm_head"]) as hc2, torch.no_grad():
        m(xs[0])
    assert list(hc2.modules) == ["lm_head"] and hc2.tokens("lm_head") == 21
    with pytest.raises(KeyError):
        gptq.HessianCollector(m, names=["nope"])
    assert not lin_a._forward_pre_hooks and not head._forward_pre_hooks          # the hooks are gone


# ---- gptq_factor -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K, act_order", [(64, False), (64, True), (256, False), (256, True)])
def test_factor_agrees_with_the_float64_factor(K, act_order):
    """Both sides round a float64 result once to fp32; the float64 error is about cond(H damped) * 2^-52, below an fp32 ulp while the
    condition number is below 2^20 (asserted): elementwise within 2^-22 * max|U| (half an ulp of the largest entry on each side)."""
    H = R.make_hessian(K, 3 * K + 1)
    H[K // 5, :] = 0.0
    H[:, K // 5] = 0.0
    u, perm, dead, cond = R.factor(H, 0.01, act_order)
    print(f"K={K} act_order={act_order}: cond(H damped) = 2^{np.log2(cond):.1f}")
    assert cond < 2.0 ** 20
    U, p, d = gptq.gptq_factor(torch.from_numpy(H), 0.01, act_order)
    assert U.dtype == torch.float32 and U.shape == (K, K) and d.dtype == torch.bool
    assert np.array_equal(d.numpy(), dead) and dead.sum() == 1 and dead[K // 5]
    if act_order:
        assert p.dtype == torch.int32 and np.array_equal(p.numpy(), perm) and sorted(perm.tolist()) == list(range(K))
    else:
        assert p is None and perm is None
    got = U.numpy()
    assert (np.tril(got, -1) == 0).all() and (np.diagonal(got) > 0).all()
    assert np.abs(got.astype(np.float64) - u.astype(np.float64)).max() <= 2.0 ** -22 * np.abs(u).max()
    # float32 input: converted, the same result
    U32, _, _ = gptq.gptq_factor(torch.from_numpy(H.astype(F32)), 0.01, act_order)
    assert U32.shape == (K, K)


def test_factor_orders_equal_diagonals_stably():
    K = 16
    rng = np.random.default_rng(0)
    A = rng.standard_normal((64, K))
    H = A.T @ A
    d = np.array([3, 1, 3, 2, 1, 3, 2, 2, 5, 1, 5, 3, 2, 1, 4, 4], np.float64) * 100
    H[np.arange(K), np.arange(K)] = d
    _, p, _ = gptq.gptq_factor(torch.from_numpy(H), 0.05, True)
    assert p.tolist() == [8, 10, 14, 15, 0, 2, 5, 11, 3, 6, 7, 12, 1, 4, 9, 13]
    _, perm, _, _ = R.factor(H, 0.05, True)
    assert perm.tolist() == p.tolist()


def test_factor_raises_when_the_damping_is_too_small():
    K = 32
    rng = np.random.default_rng(1)
    A = rng.standard_normal((4, K))
    H = A.T @ A                                                         # rank 4
    H[0, 1] = H[1, 0] = H[0, 0] * 10                                     # and not positive semi-definite
    with pytest.raises(ValueError, match="percdamp"):
        gptq.gptq_factor(torch.from_numpy(H), 0.0, False)
    with pytest.raises(ValueError, match="square"):
        gptq.gptq_factor(torch.zeros(4, 5))
    gptq.gptq_factor(torch.from_numpy(A.T @ A), 0.01, False)             # a rank-deficient H is what the damping is for


# ---- the wrapper's refusals ----------------------------------------------------------------------------------------------------------------
@pytest.fixture
def recorder(monkeypatch):
    """CPU tensors stand in for device tensors: the device check, the stream and the C call are replaced, everything else runs."""
    calls = []
    monkeypatch.setattr(ops, "_dev", lambda t, what: t)
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    monkeypatch.setattr(_lib, "call", lambda name, *args: calls.append((name, args)))
    return calls


def _operands(N=8, K=64, g=32):
    w = torch.randn(N, K)
    s, o = torch.rand(N, K // g) + 0.1, torch.zeros(N, K // g)
    U = torch.eye(K)
    return w, s, o, U


def test_wrapper_passes_the_contracts_arguments(recorder):
    w, s, o, U = _operands()
    perm = torch.arange(63, -1, -1, dtype=torch.int32)
    dead = torch.zeros(64, dtype=torch.bool)
    dead[5] = True
    res = gptq.gptq_round(w, s, o, 0, 15, U, 32, perm, dead)
    assert len(recorder) == 1 and recorder[0][0] == "mq_gptq_round"
    a = ctypes.cast(recorder[0][1][0], ctypes.POINTER(_lib.MqGptqArgs)).contents
    assert (a.N, a.K, a.group_size, a.qmin, a.qmax) == (8, 64, 32, 0.0, 15.0)
    assert a.w != w.data_ptr()                                           # dead columns: a working copy, w itself is not modified
    assert a.u == U.data_ptr() and a.perm == perm.data_ptr() and a.scale == s.data_ptr() and a.offset == o.data_ptr()
    assert a.index == res.index.data_ptr() and a.w_deq == res.dequantized.data_ptr() and a.loss == res.loss.data_ptr()
    assert a.workspace_bytes == _lib.load().mq_gptq_workspace_bytes(8, 64) > 0 and a.workspace
    assert res.index.dtype == torch.uint8 and res.index.shape == (8, 64) and res.loss.dtype == torch.float64 and res.loss.shape == (8,)
    recorder.clear()
    with pytest.raises(RuntimeError, match="8 x 1"):                     # group_size -1 = K: the grid holds one entry a row
        gptq.gptq_round(w, s, o, -8, 7, U)
    assert not recorder
    gptq.gptq_round(w, s[:, :1].half(), o[:, :1].double(), -8, 7, U)     # grids of any floating dtype are read as fp32
    a = ctypes.cast(recorder[0][1][0], ctypes.POINTER(_lib.MqGptqArgs)).contents
    assert a.group_size == 64 and a.perm is None and a.w == w.data_ptr() and (a.qmin, a.qmax) == (-8.0, 7.0)


def test_wrapper_refusals(recorder, monkeypatch):
    w, s, o, U = _operands()
    perm = torch.arange(64, dtype=torch.int32)
    bad = [
        (RuntimeError, "float32", dict(w=w.double())),
        (RuntimeError, "float32", dict(w=w.half())),
        (RuntimeError, "contiguous", dict(w=torch.randn(64, 8).t())),
        (RuntimeError, r"\[N, K\]", dict(w=w.reshape(-1))),
        (RuntimeError, "one \\(scale, offset\\) per row and group", dict(scale=s[:-1])),
        (RuntimeError, "one \\(scale, offset\\) per row and group", dict(offset=torch.zeros(8, 1))),
        (RuntimeError, "floating-point", dict(scale=torch.ones(8, 2, dtype=torch.int32))),
        (RuntimeError, "float32", dict(U=U.double())),
        (RuntimeError, "contiguous", dict(U=torch.eye(128)[::2, ::2])),
        (RuntimeError, "4096 elements", dict(U=torch.eye(32))),
        (RuntimeError, "int32", dict(perm=perm.long())),
        (RuntimeError, "64 elements", dict(perm=perm[:-1])),
        (ValueError, "not a permutation", dict(perm=torch.cat((perm[:-1], perm[:1])))),
        (ValueError, "not a permutation", dict(perm=perm + 1)),
        (ValueError, "does not divide", dict(group_size=24)),
        (ValueError, "multiple of 4", dict(group_size=2)),
        (ValueError, "qmin < qmax", dict(qmin=0, qmax=256)),
        (ValueError, "qmin < qmax", dict(qmin=3, qmax=3)),
        (RuntimeError, "bool", dict(dead=torch.zeros(64))),
        (RuntimeError, "64 elements", dict(dead=torch.zeros(63, dtype=torch.bool))),
    ]
    for exc, text, change in bad:
        kw = dict(w=w, scale=s, offset=o, qmin=0, qmax=15, U=U, group_size=32, perm=None, dead=None)
        kw.update(change)
        with pytest.raises(exc, match=text):
            gptq.gptq_round(**kw)
    for exc, text, shape in ((ValueError, "16 to 16384", (4, 8)), (ValueError, "16 to 16384", (4, 18))):
        with pytest.raises(exc, match=text):
            gptq.gptq_round(torch.randn(*shape), torch.ones(4, 1), torch.zeros(4, 1), 0, 15, torch.eye(shape[1]))
    assert not recorder
    monkeypatch.undo()                                                   # the real device check: a CPU tensor is refused first
    with pytest.raises(RuntimeError, match="ROCm device tensor"):
        gptq.gptq_round(w, s, o, 0, 15, U, 32)


# ---- the C entry's refusals ----------------------------------------------------------------------------------------------------------------
def test_entry_refuses_before_any_launch():
    """MQ_EINVAL + a message before any HIP call: pointers are fake, aligned and never dereferenced."""
    lib = _lib.load()
    P = 0x10000

    def args(**kw):
        a = _lib.MqGptqArgs()
        a.w = a.scale = a.offset = a.u = a.perm = a.workspace = a.index = a.w_deq = a.loss = P
        a.N, a.K, a.group_size, a.qmin, a.qmax = 8, 64, 32, 0.0, 15.0
        a.workspace_bytes = lib.mq_gptq_workspace_bytes(8, 64)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def rc(a):
        return lib.mq_gptq_round(ctypes.byref(a), None), lib.mq_last_error().decode()

    assert lib.mq_gptq_round(None, None) == 1 and b"null argument block" in lib.mq_last_error()
    for kw, text in (
        (dict(K=12), "16 to 16384"), (dict(K=16388, group_size=4), "16 to 16384"), (dict(K=66, group_size=66), "multiple of 4"),
        (dict(group_size=24), "group_size"), (dict(group_size=2), "group_size"), (dict(group_size=0), "group_size"),
        (dict(qmax=256.0), "qmax - qmin <= 255"), (dict(qmin=-128.0, qmax=128.0), "qmax - qmin <= 255"), (dict(qmin=0.5), "integer qmin"),
        (dict(qmin=15.0), "qmin < qmax"), (dict(N=-1), "bad row count"), (dict(N=1 << 31), "bad row count"),
        (dict(N=(1 << 31) - 64, K=16, group_size=16), "below 2\\^31"),
        (dict(u=None, perm=None), "null pointer"), (dict(w=None), "null pointer"), (dict(scale=None), "null pointer"), (dict(offset=None), "null pointer"),
        (dict(index=None), "null pointer"), (dict(workspace=None), "null pointer"), (dict(u=None, perm=P), "perm given without u"),
        (dict(w=P + 4), "16-byte aligned"), (dict(u=P + 8), "16-byte aligned"), (dict(perm=P + 4), "16-byte aligned"),
        (dict(index=P + 1), "16-byte aligned"), (dict(w_deq=P + 4), "16-byte aligned"), (dict(loss=P + 8), "16-byte aligned"),
        (dict(scale=P + 4), "16-byte aligned"), (dict(workspace_bytes=1024), "workspace of 1024 bytes"),
    ):
        code, msg = rc(args(**kw))
        assert code == 1 and re.search(text, msg), (kw, code, msg)
    # N == 0: MQ_OK without a launch, whatever the pointers
    assert lib.mq_gptq_round(ctypes.byref(args(N=0, w=None, index=None, workspace=None, u=None, perm=None)), None) == 0
    # the workspace query: the shape alone decides, -1 for a shape not served
    assert lib.mq_gptq_workspace_bytes(0, 64) == 0 and lib.mq_gptq_workspace_bytes(8, 12) == -1 and lib.mq_gptq_workspace_bytes(8, 16388) == -1
    assert lib.mq_gptq_workspace_bytes(1, 64) == lib.mq_gptq_workspace_bytes(64, 64) < lib.mq_gptq_workspace_bytes(65, 64)
    assert lib.mq_gptq_workspace_bytes(64, 64) >= 64 * 64 * 5 + 2 * 16 * 64 * 4
    assert lib.mq_gptq_workspace_bytes((1 << 31) - 64, 16) == -1


def test_report_reads_like_the_clip_searchs():
    r = gptq.GptqReport()
    assert r.summary == "0 linears rounded by GPTQ, 0 modules skipped"
    r["a"] = gptq.GptqLine(2.0, 1.0, 0.5, 0.25)
    r.skipped["lm_head"] = "lm_head stays in floating point"
    assert r.summary == "1 linears rounded by GPTQ, layer objective 2 -> 1, 1 modules skipped"
