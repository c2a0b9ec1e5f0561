"""mq_lwc_search on the GPU against the numpy restatement of its definition (lwc_search_ref.py): every entry of the cost table within the
derived summation bound TOL(cols), the reported vectors exactly consistent with the kernel's own table, the chosen index equal to the
helper's wherever the helper's costs leave no doubt.  Cases: every geometry of the kernel, both sides of every switch, partly filled
workgroups, 2 / 4 / 8-bit grids, C in {1, 2, 64, 1024}, a cross-product table, col_weight per row and per group, the special rows."""
import numpy as np
import pytest
import torch

import lwc_search_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


def _run(dev, i, return_costs):
    from mobilequant_amd import ops
    c = R.CASES[i]
    w, lo, hi, cw = R.case_inputs(c)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    out = ops.lwc_search(t(w), t(lo), t(hi), c["bits"], c["sym"], t(cw), return_costs=return_costs)
    return [o.cpu().numpy() for o in out]


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=[R.case_id(c) for c in R.CASES])
def test_costs_and_choice_equal_the_definition(dev, i):
    c = R.CASES[i]
    want, want_idx, cls = R.reference(i)
    idx, best, base, costs = _run(dev, i, True)
    rows, C, L = c["rows"], want.shape[1], c["cols"]
    assert costs.shape == (rows, C) and costs.dtype == np.float64 and idx.dtype == np.int32 and best.dtype == base.dtype == np.float64
    # every entry of the table within the summation bound (NaN exactly where the helper has NaN)
    assert np.array_equal(np.isnan(costs), np.isnan(want))
    ok = ~np.isnan(want)
    err = np.abs(costs[ok] - want[ok])
    worst = float((err / np.where(want[ok] > 0, want[ok], 1.0)).max()) if err.size else 0.0
    print(f"{R.case_id(c)}: worst relative cost error {worst:.3e} (TOL {R.TOL(L):.3e}), rows by class "
          f"{ {k: cls.count(k) for k in sorted(set(cls))} }")
    assert (err <= R.TOL(L) * want[ok]).all(), worst
    # the three vectors against the kernel's OWN table, exactly
    assert np.array_equal(base, costs[:, 0], equal_nan=True)
    assert np.array_equal(best, costs[np.arange(rows), idx], equal_nan=True)
    assert np.array_equal(idx, R.first_min(costs))
    # against the helper: the same index wherever the helper's table is unambiguous, and never a worse candidate than the tolerance allows
    for r in range(rows):
        if cls[r] == "nan":
            assert idx[r] == 0 and np.isnan(best[r]) and np.isnan(base[r])
            continue
        if cls[r] in ("clear", "tie"):
            assert idx[r] == want_idx[r], (r, idx[r], want_idx[r])
        assert want[r, idx[r]] <= want[r].min() * (1.0 + 4.0 * R.TOL(L)), r
    if c["specials"]:
        assert idx[0] == 0 and (costs[0] == 0).all() and idx[1] == 0 and idx[4] == 0
        if c["bits"] <= 4 and c["cols"] >= 1024 and C >= 64:
            assert idx[3] > 0
    # without the table: the same three vectors
    idx2, best2, base2 = _run(dev, i, False)
    assert np.array_equal(idx2, idx) and np.array_equal(best2, best, equal_nan=True) and np.array_equal(base2, base, equal_nan=True)


def test_empty_weight_and_offset_rows(dev):
    """rows == 0 launches nothing; a weight that starts 16 bytes into an allocation (a row view of a larger weight) is read where it is."""
    from mobilequant_amd import ops
    t = torch.from_numpy(R.ratio_table(8)).to(dev)
    idx, best, base = ops.lwc_search(torch.empty(0, 64, device=dev), t, t, 4, False)
    assert idx.shape == best.shape == base.shape == (0,)
    w = torch.from_numpy(R.make_weight(9, 132, 5)).to(dev)
    whole = ops.lwc_search(w, t, t, 4, True, return_costs=True)
    part = ops.lwc_search(w[3:], t, t, 4, True, return_costs=True)
    for a, b in zip(whole, part):
        assert torch.equal(a[3:], b)
