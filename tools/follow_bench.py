#!/usr/bin/env python3
"""Measurements of the follow law (include/wbc_ground.h, "Following the ground") for profiles/r12/follow.md.

    python tools/follow_bench.py kernel [--n 4096] [--bursts 30] [--burst 20]
    python tools/follow_bench.py loop --follow off|lift|fit [--n 4096] [--steps 300] [--repeats 5]

  kernel: device time per launch of wbc_ground_follow_kernel (LIFT and FIT) on the sixteen-profile batch of tests/follow_oracle.py,
    and of the target-lookup kernel beside it: HIP events around bursts of back-to-back launches after a warm-up, the median over
    the bursts.  The follow law works in place, so the targets are put back before every burst (outside the events); within a burst
    it is applied to its own output, which changes the numbers it works on and not the work.
  loop: time per 1 ms tick of wbc_ground_rollout at 16 substeps, MPTC on tools/ground_bench.py's trot, with the terrain flat(0)
    set on the plant: following that ground changes no target bit, so `off` and `fit` run the same ticks and differ by the follow
    launch alone.  One figure per process; an older library (WBC_HIP_LIB) is measured with `--follow off`, which calls nothing it
    lacks, and the processes of the versions to compare are run in turn by the caller.
Both print one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _burst_us(fn, restore, bursts, burst, warm=3):
    import torch
    out = []
    for k in range(warm + bursts):
        restore()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(burst):
            fn()
        e1.record()
        torch.cuda.synchronize()
        if k >= warm:
            out.append(e0.elapsed_time(e1) * 1e3 / burst)
    return {"median_us": statistics.median(out), "min_us": min(out), "max_us": max(out), "bursts": bursts, "burst": burst}


def kernel(a):
    import numpy as np
    import torch
    import follow_oracle as fo
    from quadruped_drake_amd import GroundContactPlant, workloads
    from quadruped_drake_amd.trajectory import TrunkTrajectory
    dev = "cuda:0"
    profiles, tid, tsc, t = fo.draw(a.n, 31)
    plant = GroundContactPlant("mini_cheetah", device=0)
    plant.set_terrain(profiles, torch.tensor(tid, device=dev), torch.tensor(tsc, device=dev))
    pristine = torch.tensor(np.ascontiguousarray(t), device=dev)
    tg = pristine.clone()
    res = {"n": a.n, "kernel": plant.follow_kernel_info()}
    for mode in ("lift", "fit"):
        res[mode] = _burst_us(lambda: plant.follow_targets(tg, mode), lambda: tg.copy_(pristine), a.bursts, a.burst)
    st_t = workloads.standing_targets("mini_cheetah", 1)[:, 0]
    K = 4000
    traj = TrunkTrajectory(np.arange(K) * 1e-3, np.tile(st_t, (K, 1)), np.full(K, 15, np.uint8), wait_time=0.0, device=0,
                           standing_targets=st_t, standing_mask=0b1111)
    tm = torch.tensor(np.random.default_rng(1).uniform(0.0, 3.9, a.n), device=dev)
    out = traj.lookup(tm)
    res["lookup"] = _burst_us(lambda: traj.lookup(tm, out=out), lambda: None, a.bursts, a.burst)
    plant.close(); traj.close()
    print(json.dumps(res), flush=True)


def loop(a):
    import numpy as np
    import torch
    import ground_oracle as go
    from quadruped_drake_amd import GroundContactPlant, MPTCController, closed_loop, terrain, workloads
    from quadruped_drake_amd.trajectory import TrunkTrajectory
    n, dt, dev = a.n, 1e-3, "cuda:0"
    st_t = workloads.standing_targets("mini_cheetah", 1)[:, 0]
    K = 4000
    ts = np.arange(K) * 1e-3
    tg = np.tile(st_t, (K, 1))
    tg[:, 0] += 0.01 * np.sin(2 * np.pi * ts / 0.3); tg[:, 3] = 0.01 * 2 * np.pi / 0.3 * np.cos(2 * np.pi * ts / 0.3)
    masks = np.where((np.arange(K) // 150) % 2 == 0, 0b1001, 0b0110).astype(np.uint8)
    for f in range(4):
        tg[((masks >> f) & 1) == 0, 18 + 9 * f + 2] += 0.02
    traj = TrunkTrajectory(ts, tg, masks, wait_time=0.0, device=0, standing_targets=st_t, standing_mask=0b1111)
    _, q0, v0 = go.drop_state("mini_cheetah", height=0.0, n=n)
    t0 = np.random.default_rng(1).uniform(0.0, 0.6, n)
    ctrl = MPTCController(max_batch=n, device=0)
    plant = GroundContactPlant("mini_cheetah", device=0)
    plant.set_terrain([terrain.flat(0.0)])
    if a.follow != "off":
        plant.set_follow(a.follow)
    us = []
    for _ in range(a.repeats + 1):               # every repeat from the same start: the same ticks; the first is the warm-up
        q, v, t = torch.tensor(q0, device=dev), torch.tensor(v0, device=dev), torch.tensor(t0, device=dev)
        closed_loop(ctrl, plant, traj, 20, dt, q, v, t)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        closed_loop(ctrl, plant, traj, a.steps, dt, q, v, t)
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / a.steps)
    us = us[1:]
    res = {"follow": a.follow, "lib": os.environ.get("WBC_HIP_LIB", "built"), "n": n, "steps": a.steps, "substeps": plant.substeps(dt),
           "us_per_tick_median": statistics.median(us), "us_per_tick_all": us,
           "state_checksum": float(q.sum() + v.sum()), "finite": bool(torch.isfinite(q).all())}
    plant.close(); ctrl.close(); traj.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("kernel", "loop"))
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--bursts", type=int, default=30)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--follow", default="off", choices=("off", "lift", "fit"))
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    kernel(a) if a.what == "kernel" else loop(a)


if __name__ == "__main__":
    main()
