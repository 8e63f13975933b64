#!/usr/bin/env python3
"""Analysis (GPU box): one library (WBC_HIP_LIB), bench protocol per case: 1 s ramp, 20 warm-up launches, then K = 200 timed launches (HIP events), five such blocks.
Prints per case the first block, the median and the minimum of the five, iterations per tick, sum|tau| and the torque checksum."""
import os, sys, time
sys.path.insert(0, os.getcwd())
import numpy as np, torch
import bench
from quadruped_drake_amd import IDController, MPTCController, workloads
for case in sys.argv[1:]:
    kind, cfg, n = case.split(":"); cfg = int(cfg); n = int(n)
    cls = {"id": IDController, "mptc": MPTCController}[kind]
    b = workloads.make_batch(cfg, n=n)
    c = cls(model=b["model"], max_batch=n, device=0)
    up = lambda x: None if x is None else torch.tensor(x, device="cuda:0")
    args = [up(b[k]) for k in ("q", "v", "targets", "mask", "mu", "mass_scale")]
    out = (torch.empty((12, n), dtype=torch.float64, device="cuda:0"), torch.empty((4, n), dtype=torch.float64, device="cuda:0"), torch.empty((n,), dtype=torch.int32, device="cuda:0"))
    t0 = time.time()
    while time.time() - t0 < 1.0: c.time_steps(100, *args, out=out)
    c.time_steps(20, *args, out=out)
    c.stats(reset=True)
    blocks = [c.time_steps(200, *args, out=out)[0] * 1e3 for _ in range(5)]
    st = c.stats()
    h = "%016x" % bench.fnv1a64(out[0].cpu().numpy().tobytes()) if n <= 4096 else "-"
    print("%s cfg %d n %d: first %.3f median %.3f min %.3f us per launch | %.3f iterations per tick, status != 0: %d, sum|tau| %.9e, tau fnv1a64 %s" % (
        kind, cfg, n, blocks[0], float(np.median(blocks)), min(blocks), st["iters_sum"] / st["ticks"], st["status_nonzero"], st["tau_abs_sum"] / 1000, h), flush=True)
    c.close()
