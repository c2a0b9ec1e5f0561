#!/usr/bin/env python3
"""Placement of the headline GEMM's workgroups on the XCDs, launch after launch.

Needs a DIAGNOSTIC build of the library (never the production one):
    MQ_FR_PROBE_XCC=1 python tools/gen_fr_asm.py fr        # the clock probe stores HW_REG_XCC_ID in place of the real-time ticks
    python -c "from mobilequant_amd import build; build.build(tag='xcc', only=['mq_gemm.hip'])"
    python tools/gen_fr_asm.py fr                          # back to the committed program
    MQ_LIB_PATH=mobilequant_amd/lib/xcc/libmobilequant_amd.so python tools/xcc_phase_probe.py

One hipGraph holds STEPS consecutive steps of bench.py's headline workload (quantize, GEMM), each GEMM with a probe buffer of its own;
the graph is replayed REPLAYS times back to back and the buffers of the last replay are read.  Prints, per step, the XCD of workgroups
0..15 and whether XCD == (workgroup + phase) % 8 for ONE phase over the whole launch, then whether that phase is the same in every step:
a weight panel stays in one XCD's L2 from step to step only if it is."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from mobilequant_amd import _lib  # noqa: E402

STEPS, REPLAYS = 8, 5


def main():
    dev = torch.device("cuda:0")
    lib = _lib.load()
    step = bench.Step(dev, _lib.MQ_U8, 0)
    bufs = [torch.zeros(256 * 8 * 2, dtype=torch.int32, device=dev) for _ in range(STEPS)]
    for i in range(3):
        step(i)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(0)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(g):
            for i in range(STEPS):
                lib.mq_gemm_set_clock_probe(bufs[i].data_ptr())
                step(i)
    finally:
        lib.mq_gemm_set_clock_probe(None)
    for _ in range(REPLAYS):
        g.replay()
    torch.cuda.synchronize()
    phases = []
    for i, b in enumerate(bufs):
        x = b.cpu().numpy().reshape(256, 8, 2)[:, :, 1] & 15          # [workgroup, wave] -> XCC_ID
        one_per_wg = bool((x == x[:, :1]).all())
        wg = x[:, 0]
        ph = int((wg[0] - 0) % 8)
        round_robin = bool(((np.arange(256) + ph) % 8 == wg).all())
        phases.append(ph if round_robin else None)
        print(f"step {i}: XCD of workgroups 0..15 {wg[:16].tolist()} | all waves of a workgroup on one XCD: {one_per_wg} | "
              f"XCD == (workgroup + {ph}) % 8 for all 256: {round_robin}")
    print("phase per step:", phases, "| stable:", len(set(phases)) == 1 and phases[0] is not None)


if __name__ == "__main__":
    main()
