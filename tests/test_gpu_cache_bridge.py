"""GPU: mq_attention_cache_import / mq_attention_cache_export (through ops.attention_cache_import / ops.attention_cache_export) against
the element-by-element reference of the header's layout formulas (cache_bridge_ref.py) on every case of cache_bridge_cases.py: head_dim
64 / 128 / 256, 1 / 2 / 3 kv heads, cache_len below and at the images' rows, plain and chunked values, dense and padded head strides,
1 .. 33 imported blocks, export ranges that cut 16-position chunks at either end.  The bridge is data movement and exact integer
arithmetic, so every comparison is an equality of whole tensors: what the launch must write equals the reference, and every other
byte -- image rows >= n, positions outside the exported range, pad bytes behind a head, the source side -- equals its seeded random
state before the launch."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cache_bridge_cases as C  # noqa: E402
import cache_bridge_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

CFG = pytest.mark.parametrize("cfg", C.CONFIGS, ids=lambda c: c.id)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ---- plumbing ----------------------------------------------------------------------------------------------------------------------
class Caches:
    """One configuration's decode caches on the device: the allocations (pad rows / chunks behind every head included) and the
    [:, :cache_len] views the ops take."""

    def __init__(self, cfg, k_np, v_np, dev):
        g = cfg.geo
        assert k_np.shape == cfg.k_alloc() and v_np.shape == cfg.v_alloc()
        self.cfg, self.k_np, self.v_np = cfg, k_np, v_np
        self.k_full, self.v_full = torch.from_numpy(k_np).to(dev), torch.from_numpy(v_np).to(dev)
        self.k = self.k_full[:, :g.cache_len]
        self.v = self.v_full[:, :g.cache_len // 16] if cfg.chunked else self.v_full[:, :g.cache_len]
        assert (self.k.stride(0), self.v.stride(0)) == cfg.head_strides()

    def set(self, k_np, v_np):
        self.k_np, self.v_np = k_np, v_np
        self.k_full.copy_(torch.from_numpy(k_np))
        self.v_full.copy_(torch.from_numpy(v_np))

    def host(self):
        return self.k_full.cpu().numpy(), self.v_full.cpu().numpy()

    def unchanged(self):
        k, v = self.host()
        return np.array_equal(k, self.k_np) and np.array_equal(v, self.v_np)


def _alloc_arrays(cfg, k_logical, v_logical, *seed):
    """The allocations holding k / v [KV, cache_len, D] in the configuration's layout, seeded random bytes in the pad."""
    L = cfg.geo.cache_len
    k = C.random_bytes(cfg.k_alloc(), cfg.id, "k", *seed)
    v = C.random_bytes(cfg.v_alloc(), cfg.id, "v", *seed)
    k[:, :L] = k_logical
    if cfg.chunked:
        v = R.to_chunked(v_logical, chunks=v.shape[1], before=v)
    else:
        v[:, :L] = v_logical
    return k, v


def _random_caches(cfg, dev, *seed):
    return Caches(cfg, C.random_bytes(cfg.k_alloc(), cfg.id, "k", *seed), C.random_bytes(cfg.v_alloc(), cfg.id, "v", *seed), dev)


def _filled_caches(cfg, fill, dev):
    return Caches(cfg, *_alloc_arrays(cfg, *C.logical_kv(cfg.geo, fill), fill), dev)


def _names(c):
    return [name for name in C.IMAGE_NAMES if c[name] is not None]


def _random_images(geo, dev, *seed):
    """An image cache whose every tensor holds seeded random bytes, and clones of that state."""
    from mobilequant_amd import ops
    c = ops.attention_image_cache(geo.KV, geo.D, geo.rows, dev)
    assert c["rows"] == geo.rows
    for name in _names(c):
        raw = c[name].view(torch.int8)
        raw.copy_(torch.from_numpy(C.random_bytes(tuple(raw.shape), geo.id, name, *seed)))
    return c, {name: c[name].clone() for name in _names(c)}


def _restore(c, state):
    for name, t in state.items():
        c[name].copy_(t)


def _host(t):
    """A device tensor as a numpy array; fp16 as its bit patterns."""
    if t.dtype == torch.float16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def _host_images(tensors, rows=None):
    out = {name: _host(t) for name, t in tensors.items() if isinstance(t, torch.Tensor)}
    if rows is not None:
        out["rows"] = rows
    return out


def _grids(zq, zk, dev):
    one = torch.ones(1, device=dev)
    return {"qk_a": (one, torch.full((1,), float(zq), device=dev), 0.0, 255.0), "qk_b": (one, torch.full((1,), float(zk), device=dev), 0.0, 255.0)}


def _exact(zk):
    return R.F16_WINDOW[0] <= zk <= R.F16_WINDOW[1]


def _assert_images(c, want, where):
    got = _host_images({name: c[name] for name in _names(c)})
    assert set(got) == set(want), where
    for name in want:
        assert got[name].shape == want[name].shape and np.array_equal(got[name], want[name]), (where, name)


def _logical(cfg, v):
    """[KV, cache_len, D] of a value cache in either layout (a torch permute: not the reference's index arithmetic)."""
    g = cfg.geo
    return v.permute(0, 1, 3, 2).reshape(g.KV, g.cache_len, g.D) if cfg.chunked else v


# ---- import ------------------------------------------------------------------------------------------------------------------------
@CFG
def test_import_equals_the_reference(dev, cfg):
    from mobilequant_amd import ops
    geo = cfg.geo
    c, state = _random_images(geo, dev, "import")
    before = _host_images(state)
    caches = {}
    for n, fill, zq, zk in C.import_cases(geo):
        where = f"{cfg.id} n={n} fill={fill} zq={zq} zk={zk}"
        if fill not in caches:
            caches[fill] = _filled_caches(cfg, fill, dev)
        dc = caches[fill]
        _restore(c, state)
        ops.attention_cache_import(c, dc.k, dc.v, n, _grids(zq, zk, dev), v_chunked=cfg.chunked)
        torch.cuda.synchronize()
        # rows < n are the reference's, rows >= n the state before: the images as wholes
        _assert_images(c, C.expected_images(geo, fill, n, zq, zk, before), where)
        assert c["k_f16_valid"] is (geo.D == 64 and _exact(zk)), where
        assert dc.unchanged(), where


@pytest.mark.parametrize("cfg", [c for c in C.CONFIGS if c.geo.D == 64], ids=lambda c: c.id)
def test_k_f16_is_exact_inside_the_window_and_poisoned_outside(dev, cfg):
    from mobilequant_amd import ops
    geo = cfg.geo
    n = C.import_ns(geo)[-1]
    dc = _filled_caches(cfg, "random", dev)
    c, state = _random_images(geo, dev, "f16")
    before = _host(state["k_f16"]).reshape(geo.KV, geo.rows // 64, 4096)
    for zk in C.ZK_EXACT + C.ZK_POISONED:
        _restore(c, state)
        ops.attention_cache_import(c, dc.k, dc.v, n, _grids(128.0, zk, dev), v_chunked=cfg.chunked)
        torch.cuda.synchronize()
        got = _host(c["k_f16"]).reshape(geo.KV, geo.rows // 64, 4096)
        assert np.array_equal(got[:, n // 64:], before[:, n // 64:]), zk
        if _exact(zk):
            assert c["k_f16_valid"] is True
            want = C.reference_images(geo, "random", n, 128.0, zk)["k_f16"].reshape(before.shape)
            assert np.array_equal(got[:, :n // 64], want[:, :n // 64]), zk
        else:
            assert c["k_f16_valid"] is False
            assert (got[:, :n // 64] == R.NAN_HALF).all(), zk


@pytest.mark.parametrize("cfg", [c for c in C.CONFIGS if c.geo.D == 64], ids=lambda c: c.id)
def test_import_without_k_f16_leaves_the_other_images_as_with_it(dev, cfg):
    from mobilequant_amd import ops
    geo = cfg.geo
    n = C.import_ns(geo)[-1]
    dc = _filled_caches(cfg, "random", dev)
    c, state = _random_images(geo, dev, "no-f16")
    before = _host_images(state)
    ops.attention_cache_import(c, dc.k, dc.v, n, _grids(255.0, 128.0, dev), v_chunked=cfg.chunked)
    torch.cuda.synchronize()
    with_f16 = {name: c[name].clone() for name in ("k_i8", "vt_i8", "k_rs")}
    assert c["k_f16_valid"] is True
    _restore(c, state)
    f16 = c["k_f16"]
    c["k_f16"] = None
    ops.attention_cache_import(c, dc.k, dc.v, n, _grids(255.0, 128.0, dev), v_chunked=cfg.chunked)
    torch.cuda.synchronize()
    assert c["k_f16_valid"] is False
    for name, t in with_f16.items():
        assert torch.equal(c[name], t), name
    assert torch.equal(f16.view(torch.int16), state["k_f16"].view(torch.int16))
    want = C.expected_images(geo, "random", n, 255.0, 128.0, before)
    del want["k_f16"]
    _assert_images(c, want, cfg.id)
    assert dc.unchanged()


# ---- export ------------------------------------------------------------------------------------------------------------------------
@CFG
def test_export_equals_the_reference(dev, cfg):
    from mobilequant_amd import ops
    geo = cfg.geo
    c, state = _random_images(geo, dev, "export")
    images = _host_images(state, rows=geo.rows)
    dc = _random_caches(cfg, dev, "export-before")
    k0, v0 = dc.k_np, dc.v_np
    for p0, n in C.export_ranges(geo):
        dc.set(k0, v0)
        ops.attention_cache_export(c, dc.k, dc.v, p0, n, v_chunked=cfg.chunked)
        torch.cuda.synchronize()
        want_k, want_v = R.export_caches(images, k0, v0, p0, n, cfg.chunked)
        got_k, got_v = dc.host()
        assert np.array_equal(got_k, want_k), (cfg.id, p0, n, "k")
        assert np.array_equal(got_v, want_v), (cfg.id, p0, n, "v")
        for name, t in state.items():
            assert torch.equal(c[name].view(torch.int8), t.view(torch.int8)), (cfg.id, p0, n, name)


# ---- round trips on the device -------------------------------------------------------------------------------------------------------
@CFG
def test_import_then_export_reproduces_the_caches(dev, cfg):
    from mobilequant_amd import ops
    geo = cfg.geo
    n = C.import_ns(geo)[-1]
    src = _filled_caches(cfg, "random", dev)
    c, _ = _random_images(geo, dev, "round")
    ops.attention_cache_import(c, src.k, src.v, n, _grids(128.0, 128.0, dev), v_chunked=cfg.chunked)
    dst = _random_caches(cfg, dev, "round-before")
    k0, v0 = dst.k_full.clone(), dst.v_full.clone()
    ops.attention_cache_export(c, dst.k, dst.v, 0, n, v_chunked=cfg.chunked)
    torch.cuda.synchronize()
    assert torch.equal(dst.k[:, :n], src.k[:, :n]) and torch.equal(_logical(cfg, dst.v)[:, :n], _logical(cfg, src.v)[:, :n])
    # everything else of the allocation -- later positions, pad -- is as it was: undo rows [0, n) and compare whole
    dst.k_full[:, :n] = k0[:, :n]
    if cfg.chunked:
        dst.v_full[:, :n // 16] = v0[:, :n // 16]
    else:
        dst.v_full[:, :n] = v0[:, :n]
    assert torch.equal(dst.k_full, k0) and torch.equal(dst.v_full, v0)


@CFG
def test_export_then_import_reproduces_the_images(dev, cfg):
    from mobilequant_amd import ops
    geo = cfg.geo
    n = C.import_ns(geo)[-1]
    a, _ = _random_images(geo, dev, "images-a")
    dc = _random_caches(cfg, dev, "between")
    ops.attention_cache_export(a, dc.k, dc.v, 0, n, v_chunked=cfg.chunked)
    b, state = _random_images(geo, dev, "images-b")
    ops.attention_cache_import(b, dc.k, dc.v, n, _grids(0.0, 0.0, dev), v_chunked=cfg.chunked)
    torch.cuda.synchronize()
    KV, D, rows = geo.KV, geo.D, geo.rows
    for name, shape in (("k_i8", (KV, rows, D)), ("vt_i8", (KV, rows // 64, D * 64))):
        cut = n if name == "k_i8" else n // 64
        got, src, old = b[name].view(shape), a[name].view(shape), state[name].view(shape)
        assert torch.equal(got[:, :cut], src[:, :cut]) and torch.equal(got[:, cut:], old[:, cut:]), name


# ---- one captured import serves later grids and later bytes ------------------------------------------------------------------------
@pytest.mark.parametrize("chunked", [False, True])
@pytest.mark.parametrize("geo", [C.GEOMETRIES[1], C.GEOMETRIES[3]], ids=lambda g: g.id)
def test_a_captured_import_follows_the_offsets_and_the_bytes(dev, geo, chunked):
    """The offsets are read by pointer at launch: a replay after the offset tensors and the decode caches were rewritten in place gives
    the images of the new grids and bytes, k_f16's poisoning included when zk moves across the window's edge."""
    from mobilequant_amd import ops
    cfg = C.Config(geo, chunked, False)
    n = C.import_ns(geo)[-1]
    dc = _filled_caches(cfg, "random", dev)
    c, state = _random_images(geo, dev, "capture")
    before = _host_images(state)
    grids = _grids(128.0, 0.0, dev)
    ops.attention_cache_import(c, dc.k, dc.v, n, grids, v_chunked=chunked, k_f16_exact=True)       # loads the code object before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.attention_cache_import(c, dc.k, dc.v, n, grids, v_chunked=chunked, k_f16_exact=True)
    for fill, zq, zk in (("random", 128.0, 0.0), ("min", -382.0, 511.0), ("max", 255.0, 512.0), ("one_hot", 0.0, -256.0), ("random", 0.0, -257.0),
                         ("max", 255.0, -256.0)):
        dc.set(*_alloc_arrays(cfg, *C.logical_kv(geo, fill), fill))
        grids["qk_a"][1].fill_(zq)
        grids["qk_b"][1].fill_(zk)
        _restore(c, state)
        graph.replay()
        torch.cuda.synchronize()
        _assert_images(c, C.expected_images(geo, fill, n, zq, zk, before), f"{cfg.id} replay fill={fill} zq={zq} zk={zk}")
        assert dc.unchanged()
