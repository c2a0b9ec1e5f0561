"""bench.py end to end on an MI355X: a plain run does only what its headline needs, within its time budget."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import ROOT

M, K, N = 2048, 2048, 5632
PLAIN_BUDGET_S = 30.0          # wall time of a plain run outside its warm-up and timed steps


@pytest.mark.gpu
def test_plain_bench_run_prints_the_headline_alone_within_its_budget(tmp_path):
    steps, warmup = 20, 5
    t0 = time.perf_counter()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--dump-outputs", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    wall = time.perf_counter() - t0
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-3000:]
    d = json.loads(lines[0])
    assert (d["unit"], d["dtype"], d["higher_is_better"], d["steps"], d["warmup"], d["n_gpus"]) == ("TOPS", "i8", True, steps, warmup, 1)
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(2.0 * M * K * N / (d["ms_per_step"] * 1e-3) / 1e12, rel=1e-3)
    # the legs of --full did not run
    assert d["roofline"] is None and d["cpu_baseline"] is None and d["decode"] is None and d["variants"] == {}
    out = np.load(tmp_path / "qlinear_out.npy")
    assert out.dtype == np.float32 and out.shape == (M, N)
    assert out.min() >= 0 and out.max() <= 255 and np.array_equal(out, np.round(out)) and out.std() > 1.0      # u8 output indices
    outside = wall - (steps + warmup) * d["ms_per_step"] * 1e-3
    assert outside < PLAIN_BUDGET_S, f"a plain bench.py run spent {outside:.1f} s outside its steps (budget {PLAIN_BUDGET_S} s)"
