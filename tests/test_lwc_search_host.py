"""Host side of the clip search (mq_lwc_search, Quantizer.search_lwc): the numpy helper against a scalar restatement, the default factor
table, the refusals that are decided before any launch, and the condition under which the GPU test may compare chosen indices."""
import ctypes
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import lwc_search_ref as R

F32 = np.float32


def _brute_cost(row, slo, shi, bits, sym, cw_row):
    """One (row, candidate) of the definition with scalar fp32 operations and an exact rational sum."""
    qmin, qmax = (-(2 ** (bits - 1)), 2 ** (bits - 1) - 1) if sym else (0, 2 ** bits - 1)
    with np.errstate(all="ignore"):
        mn, mx = F32(min(row)), F32(max(row))
        if any(math.isnan(float(v)) for v in row):
            return float("nan")
        lo, hi = F32(F32(slo) * mn), F32(F32(shi) * mx)
        alpha, beta = (F32(max(abs(lo), abs(hi))), F32(0)) if sym else (F32(hi - lo), lo)
        scale = F32(min(max(F32(alpha / F32(qmax)), F32(1e-5)), F32(1e6)))
        offset = F32(-np.rint(F32(beta / scale)))
        total = Fraction(0)
        for k, x in enumerate(row):
            t = F32(x / scale)
            r = F32(F32(np.rint(t) - t) + t)
            q = F32(r + offset)
            qc = F32(min(max(q, F32(qmin)), F32(qmax)))
            y = F32(F32(qc - offset) * scale)
            e = float(F32(y - x))
            term = e * e                                   # exact in fp64: two 24-bit significands
            assert Fraction(term) == Fraction(e) * Fraction(e)
            if cw_row is not None:
                term = term * float(cw_row[k])
            total += Fraction(term)
    return float(total)                                     # Fraction -> float rounds correctly, as fsum does


@pytest.mark.parametrize("bits,sym", [(2, False), (4, False), (4, True), (8, True)])
def test_helper_equals_a_scalar_restatement(bits, sym):
    rows, cols, C = 5, 16, 6
    w = R.make_weight(rows, cols, 77 + bits)
    w[1] = 0.0
    w[2, 3] = np.nan
    lo, hi = R.ratio_table(C), R.ratio_table(C, 0.7)
    cw = R.make_col_weight(cols, "grouped", 3)
    for weight in (None, cw):
        got = R.cost_table(w, lo, hi, bits, sym, weight)
        ix = None if weight is None else R.row_cw_index(rows, cols, weight.size)
        for r in range(rows):
            for c in range(C):
                want = _brute_cost(w[r], lo[c], hi[c], bits, sym, None if weight is None else weight[ix[r]])
                assert (math.isnan(want) and math.isnan(got[r, c])) or got[r, c] == want, (r, c, got[r, c], want)
        assert np.isnan(got[2]).all() and (got[1] == 0).all()
        assert R.first_min(got)[2] == 0 and R.first_min(got)[1] == 0
    assert (R.row_cw_index(6, 16, 64)[5] == np.arange(16, 32)).all()        # row 5 of a 4-block vector uses block 5 % 4


def test_first_min_is_the_strict_rule():
    nan = float("nan")
    t = np.array([[3.0, 2.0, 2.0, 5.0], [1.0, 1.0, 1.0, 1.0], [nan, 1.0, 0.5, 2.0], [4.0, nan, 3.0, 3.0], [2.0, 3.0, 1.0, 0.5]])
    assert R.first_min(t).tolist() == [1, 0, 0, 2, 3]
    assert R.classify(t, 16) == ["clear", "tie", "nan", "nan", "clear"]
    assert R.classify(np.array([[1.0, 1.0 + 2 ** -50, 7.0]]), 1024) == ["ambiguous"]


def test_default_factor_table():
    import mobilequant_amd as mq
    for n, lo in ((64, 0.5), (32, 0.5), (17, 0.3), (1, 0.5), (2, 0.9)):
        f = mq.lwc_factor_table(n, lo)
        assert f.dtype == torch.float32 and f.shape == (n,) and float(f[0]) == 4.0
        assert bool((f[1:] < f[:-1]).all())
        if n > 1:
            last = float(torch.sigmoid(f[-1:])[0])
            assert abs(last - lo) <= float(np.spacing(F32(lo))), (n, lo, last)
    with pytest.raises(ValueError):
        mq.lwc_factor_table(0)
    with pytest.raises(ValueError):
        mq.lwc_factor_table(8, 0.99)


def test_c_entry_refuses_before_any_launch():
    from mobilequant_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)

    def call(rows=8, cols=64, C=4, bits=4, cw=None, cw_len=0, w=p, out=p):
        return lib.mq_lwc_search(w, rows, cols, p, p, C, bits, 0, cw, cw_len, out, out, out, None, None)
    for kw, text in ((dict(cols=30), b"multiple of 4"), (dict(cols=12), b"16 to 16384"), (dict(cols=16388), b"16 to 16384"),
                     (dict(C=0), b"candidates"), (dict(C=1025), b"candidates"), (dict(bits=1), b"bitwidth"), (dict(bits=17), b"bitwidth"),
                     (dict(cw=p, cw_len=96), b"col_weight"), (dict(cw=p, cw_len=0), b"col_weight"), (dict(rows=-1), b"row count"),
                     (dict(w=None), b"null pointer"), (dict(out=None), b"null pointer"), (dict(w=ctypes.c_void_p(4100)), b"aligned"),
                     (dict(cw=ctypes.c_void_p(4100), cw_len=64), b"aligned")):
        assert call(**kw) == 1, kw
        err = lib.mq_last_error()
        assert err.startswith(b"mq_lwc_search:") and text in err, (kw, err)
    assert lib.mq_lwc_search(None, 0, 64, None, None, 4, 4, 0, None, 0, None, None, None, None, None) == 0


def test_ops_refuses_before_any_launch():
    from mobilequant_amd import ops
    w, t = torch.zeros(8, 64), torch.full((4,), 0.9)
    for args, text in (((w.double(), t, t, 4, False), "float32"), ((w, t.half(), t, 4, False), "float32"), ((w[:, :30], t, t, 4, False), "contiguous"),
                       ((torch.zeros(8, 30), t, t, 4, False), "multiple of 4"), ((w.reshape(-1), t, t, 4, False), r"\[rows, cols\]"),
                       ((w, t, t[:3], 4, False), "one length"), ((w, torch.zeros(1025), torch.zeros(1025), 4, False), "1 to 1024"),
                       ((w, t, t, 17, False), "bitwidth"), ((w, t, t, 4, False, torch.ones(96)), "col_weight"),
                       ((w, t, t, 4, False, torch.ones(2, 64)), "col_weight"), ((w, t, t, 4, False, torch.ones(64).double()), "float32")):
        with pytest.raises(RuntimeError, match=text):
            ops.lwc_search(*args)
    with pytest.raises(RuntimeError, match="ROCm device tensor"):          # everything else in order: only the device is missing
        ops.lwc_search(w, t, t, 4, False, torch.ones(128))


def _quantizer(**kw):
    import mobilequant_amd as mq
    cfg = dict(bitwidth=4, is_per_channel=True, is_symmetric=False)
    cfg.update(kw)
    return mq.Quantizer(mq.QuantConfig(**cfg))


def test_search_lwc_refuses_before_any_launch():
    w = torch.zeros(8, 64)
    for kw, text in ((dict(is_per_channel=False), "per-tensor"), (dict(bitwidth=16), "16-bit"), (dict(is_dynamic=True), "dynamic"),
                     (dict(group_size=48), "does not divide"), (dict(group_size=8), "columns")):
        q = _quantizer(**kw)
        with pytest.raises(ValueError, match=text):
            q.search_lwc(w)
        assert not q.lwc and not hasattr(q, "upbound_factor")
    q = _quantizer()
    with pytest.raises(ValueError, match="2-D"):
        q.search_lwc(torch.zeros(2, 8, 64))
    with pytest.raises(ValueError, match="columns"):
        q.search_lwc(torch.zeros(8, 30))
    with pytest.raises(ValueError, match=r"factors\[0\]"):
        q.search_lwc(w, factors=torch.tensor([3.0, 2.0]))
    with pytest.raises(ValueError, match="float32 vector"):
        q.search_lwc(w, factors=torch.tensor([4.0, 2.0], dtype=torch.float64))
    with pytest.raises(ValueError, match="at most 1024"):
        q.search_lwc(w, factors=torch.linspace(4.0, 0.0, 1025))
    with pytest.raises(ValueError, match="at most 1024"):
        q.search_lwc(w, factors=torch.linspace(4.0, 0.0, 33), mode="independent")
    with pytest.raises(ValueError, match="mode"):
        q.search_lwc(w, mode="both")
    with pytest.raises(ValueError, match="col_weight"):
        q.search_lwc(w, col_weight=torch.ones(32))
    assert not q.lwc                                                        # nothing was enabled by a refused call
    with pytest.raises(RuntimeError, match="ROCm device tensor"):          # an eligible call reaches the kernel wrapper, which has no CPU path
        q.search_lwc(w)


def test_torch_op_is_registered_with_a_meta_kernel():
    import mobilequant_amd.torch_ops as T
    assert "lwc_search" in T.OPS
    w, t = torch.empty(6, 64, device="meta"), torch.empty(9, device="meta")
    idx, best, base, costs = torch.ops.mobilequant_amd.lwc_search(w, t, t, 4, False)
    assert (idx.dtype, idx.shape, best.dtype, best.shape, base.shape, costs.dtype, costs.shape) == \
        (torch.int32, (6,), torch.float64, (6,), (6,), torch.float64, (6, 9))
    with pytest.raises(NotImplementedError):
        torch.ops.mobilequant_amd.lwc_search(torch.zeros(6, 64), torch.ones(2), torch.ones(2), 4, False)


def test_case_list_reaches_every_branch():
    cs = R.CASES
    ids = [R.case_id(c) for c in cs]
    assert len(set(ids)) == len(ids)
    cols = {c["cols"] for c in cs}
    assert {16, 64, 128, 1024, 2052, 16384} <= cols
    for sw in R.SWITCHES:
        assert {sw - 4, sw, sw + 4} <= cols
    geo = lambda n: sum(n > s for s in R.SWITCHES)                                # noqa: E731
    for g in range(4):
        mine = [c for c in cs if geo(c["cols"]) == g]
        assert {(c["bits"], c["sym"]) for c in mine} == set(R.GRIDS), g
        assert {c["C"] for c in mine} >= {1, 2, 64, 1024}, g
        assert {c["cw"] for c in mine} == set(R.CW_MODES), g
        assert any(c["specials"] for c in mine), g
    assert any(c["rows"] % 64 and c["rows"] > 64 and c["cols"] <= 128 for c in cs)          # lane form: a partly filled second workgroup
    assert any(c["rows"] % 4 and 128 < c["cols"] <= 1024 for c in cs)                       # wave form: a partly filled workgroup
    assert sum(c["mode"] == "independent" for c in cs) >= 1


def test_chosen_indices_are_comparable_on_the_gpu_cases():
    """What test_gpu_lwc_search relies on, from the helper alone: rows whose best cost is neither an exact tie of all candidates nor more than
    4 * TOL(L) below the best different cost are at most 1 % of the rows; the special rows behave as the definition says."""
    n_rows = n_amb = 0
    for i, c in enumerate(R.CASES):
        costs, idx, cls = R.reference(i)
        if c["C"] == 1:
            assert (idx == 0).all()
            continue
        n_rows += len(cls)
        n_amb += cls.count("ambiguous")
        if c["specials"]:
            assert cls[0] == "tie" and idx[0] == 0 and (costs[0] == 0).all()                # all-zero: scale at its lower clamp, every cost 0
            assert cls[4] == "nan" and idx[4] == 0 and np.isnan(costs[4]).all()
            assert idx[1] == 0                                                              # constant: any shrink only adds error
            if c["bits"] <= 4 and c["cols"] >= 1024:
                assert idx[3] > 0, R.case_id(c)                                             # the outlier row: clipping pays
    assert n_rows > 500 and n_amb <= 0.01 * n_rows, (n_amb, n_rows)
