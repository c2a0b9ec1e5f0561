"""GPU: the full-workgroup path of quantize_tiled8_kernel (csrc/mq_quantize.hip) -- the staged fp32 -> int8 image kernel takes it in
every workgroup whose rows all lie below `rows`, with unclamped addresses, no per-vector condition and every load requested up front.
quantize_cases.TILED_CASES reach the staged kernel almost only at ragged row counts (77, 70, 65), so the path gets its own smallest
shapes here: launches of full workgroups only (every V = cols / 1024, both rows-per-workgroup forms) and launches that mix full with
ragged (a workgroup that straddles `rows`) or padding workgroups.

Each shape runs on the three TILED_GRIDS, with and without row_sum, and is held EXACTLY to oracle.quantize_storage /
oracle.tiled_image_bytes (the expectations of test_gpu_quantize.py, built from quantize_cases.tiled_inputs); one shape carries
non-finite inputs.  The same launch with the staged kernel switched off (mq_quantize_tiled_set_staged(0): the lane-per-fragment
kernel) has to give the same image, padding rows included, and the same row sums byte for byte.  Canaries around every output."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import quantize_cases as C  # noqa: E402
from oracle import mq_oracle as O  # noqa: E402
from test_gpu_quantize import _call, check_image, check_sums, dev, run_tiled  # noqa: E402,F401

T = C.TCase
FULLWG_CASES = [
    # full workgroups only: rows a multiple of 16 (four rows per workgroup up to 2048 columns, eight beyond, or forced)
    T("full-64x1024", 64, 1024), T("full-64x2048", 64, 2048), T("full-64x3072", 64, 3072), T("full-64x4096", 64, 4096),
    T("full-80x2048-rows8", 80, 2048, knob_rows=8), T("full-64x4096-rows4", 64, 4096, knob_rows=4),
    # full and ragged / padding workgroups in one launch
    T("mixed-68x2048", 68, 2048),                    # rows 64-67 full, 68-79 padding workgroups
    T("mixed-66x2048", 66, 2048),                    # the workgroup of rows 64-67 straddles `rows`
    T("mixed-72x4096", 72, 4096),                    # eight rows: 64-71 full, 72-79 padding
    T("mixed-68x4096-rows4", 68, 4096, knob_rows=4),
    T("mixed-68x2048-nonfinite", 68, 2048, nonfinite=True),
]


def test_the_cases_reach_what_they_are_for():
    """Without a device: every case takes the staged kernel; the lists hold every V in both forms, launches without and with a
    workgroup past or across `rows`, and a non-finite one."""
    seen = set()
    for c in FULLWG_CASES:
        b = C.tiled_branch(c)
        assert b["kernel"].startswith("staged-V"), c.id
        rw = int(b["kernel"].rsplit("rows", 1)[1])
        assert c.rows // rw >= 1                                  # at least one full workgroup
        full_only = c.rows % 16 == 0
        assert full_only == c.id.startswith("full"), c.id
        seen.add((b["kernel"], "full" if full_only else ("straddle" if c.rows % rw else "padding")))
    for v in (1, 2, 3, 4):
        assert any(k.startswith("staged-V%d-" % v) and w == "full" for k, w in seen), v
    for k in ("staged-V2-rows4", "staged-V2-rows8", "staged-V4-rows4", "staged-V4-rows8"):
        assert any(kk == k for kk, _ in seen), k
    assert {"straddle", "padding"} <= {w for _, w in seen}
    assert any(c.nonfinite for c in FULLWG_CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("c", FULLWG_CASES, ids=lambda c: c.id)
def test_quantize_tiled_full_workgroups(dev, c):  # noqa: F811
    try:
        _call("mq_quantize_tiled_set_rows", c.knob_rows)
        for grid, shift in C.TILED_GRIDS:
            x, sc, of, qmin, qmax, cs = C.tiled_inputs(c, grid)
            stored, want_rs = O.quantize_storage(x, sc, of, qmin, qmax, shift, cs)
            for row_sum in (True, False):
                what = "%s %s%s" % (c.id, grid, " +row_sum" if row_sum else "")
                _call("mq_quantize_tiled_set_staged", 1)
                got, got_rs = run_tiled(dev, c, grid, shift, row_sum)
                check_image(got, c, grid, shift, stored, what)
                if row_sum:
                    check_sums(got_rs, want_rs, what)
                _call("mq_quantize_tiled_set_staged", 0)
                lane, lane_rs = run_tiled(dev, c, grid, shift, row_sum)
                assert got.tobytes() == lane.tobytes(), "%s: the image differs from the lane-per-fragment kernel's at byte %d" % (
                    what, int(np.flatnonzero(got != lane)[0]))
                if row_sum:
                    assert got_rs.tobytes() == lane_rs.tobytes(), what + ": row sums differ from the lane-per-fragment kernel's"
    finally:
        _call("mq_quantize_tiled_set_rows", 0)
        _call("mq_quantize_tiled_set_staged", 1)
