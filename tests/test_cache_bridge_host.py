"""Host side of the cache bridge tests: the element-by-element reference (cache_bridge_ref.py) agrees with the two other statements of
the header's layouts that the suite holds, it round-trips, and the case table (cache_bridge_cases.py) is legal and covers the chunk /
block situations its ranges are listed for.  numpy / CPU torch only."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cache_bridge_cases as C  # noqa: E402
import cache_bridge_ref as R  # noqa: E402
from test_gpu_prefill_append import _k_f16_of, _v_of, _vt_of  # noqa: E402
from test_gpu_prefill_attention import _cache_check  # noqa: E402

I32 = (-2 ** 31, 2 ** 31 - 1)


def _data(KV, L, D, seed):
    return C.random_bytes((KV, L, D), "host", seed, "k"), C.random_bytes((KV, L, D), "host", seed, "v")


# ---- the two statements agree ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,KV,n,rows,zq,zk", [(64, 3, 192, 256, -382.0, -256.0), (64, 1, 64, 64, 255.0, 511.0), (128, 2, 192, 256, 0.0, 0.0),
                                               (256, 3, 128, 256, 128.0, 0.0)])
def test_reference_agrees_with_the_permute_and_view_statements(D, KV, n, rows, zq, zk):
    k, v = _data(KV, 208 if rows == 256 else rows, D, D + KV)
    im = R.import_images(k, v, n, zq, zk, D, True, rows=rows)
    tk, tv = torch.from_numpy(k[:, :n].copy()), torch.from_numpy(v[:, :n].copy())
    nb, B = n // 64, rows // 64
    vt = torch.from_numpy(im["vt_i8"]).view(KV, B, D, 64)
    # test_gpu_prefill_append.py's permutes
    assert torch.equal(vt[:, :nb], _vt_of(tv))
    assert torch.equal(_v_of(vt)[:, :n], tv)
    assert torch.equal(torch.from_numpy(im["k_i8"]).view(KV, rows, D)[:, :n], tk)
    assert np.array_equal(im["k_rs"].reshape(KV, rows)[:, :n], -(int(zq) - 128) * k[:, :n].astype(np.int64).sum(-1))
    if D == 64:
        want = _k_f16_of(tk, zk).view(torch.int16).numpy().view(np.uint16)
        assert np.array_equal(im["k_f16"].reshape(KV, B, 8, 64, 8)[:, :nb], want)
    else:
        assert np.array_equal(im["v_pre"].reshape(KV, B, D)[:, :nb], v[:, :n].astype(np.int64).reshape(KV, nb, 64, D).sum(2).cumsum(1))
    # test_gpu_prefill_attention.py's views: _cache_check asserts every image of positions 0 .. n - 1
    cache = {"rows": rows, "k_i8": torch.from_numpy(im["k_i8"]), "vt_i8": torch.from_numpy(im["vt_i8"]),
             "k_rs": torch.from_numpy(im["k_rs"].astype(np.int32)),
             "k_f16": None if im["k_f16"] is None else torch.from_numpy(im["k_f16"].view(np.int16)).view(torch.float16),
             "v_pre": None if im["v_pre"] is None else torch.from_numpy(im["v_pre"].astype(np.int32))}
    qk = (types.SimpleNamespace(offset=zq), types.SimpleNamespace(offset=zk))
    _cache_check(cache, {"ik8": k, "iv8": v}, qk, types.SimpleNamespace(KV=KV, D=D), n, f16=True)
    # rows >= n of every image are the state before (zero here)
    for name, per_row in (("k_i8", D), ("k_rs", 1)):
        assert not im[name].reshape(KV, rows, per_row)[:, n:].any()
    assert not im["vt_i8"].reshape(KV, B, D * 64)[:, nb:].any()


@pytest.mark.parametrize("zk", C.ZK_POISONED)
def test_reference_poisons_k_f16_outside_the_window(zk):
    k, v = _data(2, 128, 64, 5)
    before = {"k_f16": np.full(2 * 128 * 64, 0x1234, np.uint16)}
    im = R.import_images(k, v, 64, 128.0, zk, 64, True, rows=128, before=before)
    h = im["k_f16"].reshape(2, 2, 4096)
    assert (h[:, 0] == R.NAN_HALF).all() and (h[:, 1] == 0x1234).all()
    assert np.isnan(h[:, 0].view(np.float16)).all()
    assert R.import_images(k, v, 64, 128.0, zk, 64, False)["k_f16"] is None


def test_chunked_layout_is_sixteen_positions_per_dimension():
    _, v = _data(2, 48, 64, 9)
    c = R.to_chunked(v)
    assert c.shape == (2, 3, 64, 16)
    assert np.array_equal(c, v.reshape(2, 3, 16, 64).transpose(0, 1, 3, 2))
    assert np.array_equal(R.from_chunked(c, 48), v) and np.array_equal(R.from_chunked(c, 21), v[:, :21])
    pad = np.full((2, 5, 64, 16), 7, np.int8)
    p = R.to_chunked(v, chunks=5, before=pad)
    assert np.array_equal(p[:, :3], c) and (p[:, 3:] == 7).all()


# ---- round trip --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunked", [False, True])
@pytest.mark.parametrize("D,KV,n", [(64, 2, 128), (128, 1, 192), (256, 3, 64)])
def test_export_of_import_returns_the_caches(D, KV, n, chunked):
    L, rows = 208, 256
    k, v = _data(KV, L, D, 3 * D + KV)
    im = R.import_images(k, v, n, 255.0, 0.0, D, True, rows=rows)
    kb, vb_logical = _data(KV, L, D, 77)
    vb = R.to_chunked(vb_logical) if chunked else vb_logical
    ke, ve = R.export_caches(im, kb, vb, 0, n, chunked)
    ve_logical = R.from_chunked(ve, L) if chunked else ve
    assert np.array_equal(ke[:, :n], k[:, :n]) and np.array_equal(ve_logical[:, :n], v[:, :n])
    assert np.array_equal(ke[:, n:], kb[:, n:]) and np.array_equal(ve_logical[:, n:], vb_logical[:, n:])
    # a partial range writes those rows and no other
    ke, ve = R.export_caches(im, kb, vb, 17, 30, chunked)
    ve_logical = R.from_chunked(ve, L) if chunked else ve
    for got, src, old in ((ke, k, kb), (ve_logical, v, vb_logical)):
        assert np.array_equal(got[:, 17:47], src[:, 17:47]) and np.array_equal(got[:, :17], old[:, :17]) and np.array_equal(got[:, 47:], old[:, 47:])


# ---- the case table is legal -------------------------------------------------------------------------------------------------------
def _violations(cfg, p0, n, is_import, v_prefix, k_f16):
    """check_cache_args's conditions (csrc/mq_attention_cache.hip), restated for a case of the table; the pointers' alignment is the
    allocator's.  Returns the conditions that do not hold."""
    g = cfg.geo
    ks, vs = cfg.head_strides()
    head_bytes = g.cache_len * g.D
    conds = {"head_dim": g.D in (64, 128, 256),
             "kv_heads": 0 < g.KV <= 65535,
             "cache_seq": g.rows > 0 and g.rows % 64 == 0 and g.rows <= 65536,
             "cache_len": g.cache_len > 0 and (not cfg.chunked or g.cache_len % 16 == 0),
             "positions": (p0 == 0 and n > 0 and n % 64 == 0) if is_import else (p0 >= 0 and n > 0),
             "inside": p0 + n <= g.rows and p0 + n <= g.cache_len,
             "strides": ks >= head_bytes and vs >= head_bytes and ks % 16 == 0 and vs % 16 == 0}
    if is_import:
        conds["v_prefix"] = (not v_prefix) if g.D == 64 else v_prefix
        conds["k_f16"] = not k_f16 or g.D == 64
    return [name for name, ok in conds.items() if not ok]


def test_every_case_passes_the_entrys_conditions():
    assert len(C.CONFIGS) == 4 * len(C.GEOMETRIES) == 28
    seen_n = set()
    for cfg in C.CONFIGS:
        g = cfg.geo
        ks, vs = cfg.head_strides()
        assert (ks > g.cache_len * g.D) == cfg.padded and (vs > g.cache_len * g.D) == cfg.padded
        cases = C.import_cases(g)
        assert cases
        for n, fill, zq, zk in cases:
            assert _violations(cfg, 0, n, True, g.D != 64, g.D == 64) == [], (cfg.id, n)
            assert fill in C.FILLS and zq in C.ZQ and zk in C.ZK_EXACT + C.ZK_POISONED
            seen_n.add(n)
        assert {(f, zq) for _, f, zq, _ in cases} == {(f, zq) for f in C.FILLS for zq in C.ZQ}
        if g.D == 64:
            assert _violations(cfg, 0, cases[0][0], True, False, False) == []                  # the import with k_f16 = None
            assert {(f, zk) for _, f, _, zk in cases} >= {(f, zk) for f in C.FILLS for zk in C.ZK_EXACT + C.ZK_POISONED}
        for p0, n in C.export_ranges(g):
            assert _violations(cfg, p0, n, False, False, False) == [], (cfg.id, p0, n)
    assert seen_n == set(C.IMPORT_N)
    assert {g.cache_len for g in C.GEOMETRIES} == set(C.EXPORT_RANGES)
    # the scan walks more than two blocks, with fewer blocks than the cache holds, at every head dim that has a prefix
    assert {g.D for g in C.GEOMETRIES if 2112 in C.import_ns(g)} == {128, 256}
    assert {g.KV for g in C.GEOMETRIES} == {1, 2, 3}


@pytest.mark.parametrize("geo", C.GEOMETRIES, ids=lambda g: g.id)
def test_row_sums_and_prefixes_stay_inside_int32(geo):
    worst_rs = worst_pre = 0
    for n, fill, zq, zk in C.import_cases(geo):
        im = C.reference_images(geo, fill, n, zq, zk)
        assert im["k_rs"].dtype == np.int64 and I32[0] <= im["k_rs"].min() and im["k_rs"].max() <= I32[1], (n, fill, zq)
        worst_rs = max(worst_rs, int(np.abs(im["k_rs"]).max()))
        if geo.D != 64:
            assert im["v_pre"].dtype == np.int64 and I32[0] <= im["v_pre"].min() and im["v_pre"].max() <= I32[1], (n, fill)
            worst_pre = max(worst_pre, int(np.abs(im["v_pre"]).max()))
    # the extreme fills reach the largest values the formulas allow at this geometry: |zq - 128| * 128 * D and 128 * 64 * blocks
    assert worst_rs == 510 * 128 * geo.D
    if geo.D != 64:
        assert worst_pre == 128 * max(C.import_ns(geo))
    assert 510 * 128 * 256 <= I32[1] and 128 * 64 * 34 <= I32[1]


def test_every_export_range_hits_what_it_is_listed_for():
    for cache_len, table in C.EXPORT_RANGES.items():
        for (p0, n), listed in table.items():
            assert p0 >= 0 and n > 0 and p0 + n <= cache_len
            hit = C.situations(p0, n, cache_len)
            assert listed <= hit, (cache_len, p0, n, sorted(listed - hit))
    covered = set().union(*(C.situations(p0, n, 208) for p0, n in C.EXPORT_RANGES[208]))
    assert C.REQUIRED_SITUATIONS <= covered, sorted(C.REQUIRED_SITUATIONS - covered)
    assert set(C.EXPORT_RANGES[208]) == {(0, 1), (0, 208), (15, 1), (15, 2), (16, 16), (17, 30), (37, 1), (63, 2), (60, 100), (192, 16), (207, 1)}
    assert set(C.EXPORT_RANGES[2176]) == {(1000, 1111), (2175, 1)}
    big = set().union(*(C.situations(p0, n, 2176) for p0, n in C.EXPORT_RANGES[2176]))
    assert {"three_blocks", "whole_chunk_between_cut_ends", "last_position"} <= big


def test_situations_are_computed_from_the_range():
    """Hand-worked ranges on a cache of 208 positions."""
    assert C.situations(32, 16, 208) == {"chunk_exactly"}
    assert C.situations(37, 1, 208) == {"strictly_inside_one_chunk", "low_end_in_chunk", "high_end_in_chunk", "inside_one_chunk"}
    assert C.situations(63, 2, 208) == {"low_end_in_chunk", "high_end_in_chunk", "both_ends_in_chunks", "block_boundary"}
    assert "last_position_unaligned_len" in C.situations(207, 1, 208) and "last_position" in C.situations(63, 1, 64)
