#!/usr/bin/env python3
"""Measurements of the gait planner (include/wbc_gait.h) for profiles/r13/gait.md and of its terrain
(include/wbc_gait_terrain.h) for profiles/r14/gait_terrain.md.

    python tools/gait_bench.py kernel [--n 4096] [--bursts 30] [--burst 20]
    python tools/gait_bench.py loop --source traj|gait|gait_terrain|gait_follow|gait_schedule|gait_feedback [--n 4096] [--steps 300] [--repeats 5]

  kernel: device time per launch of wbc_gait_targets_kernel (a trot, per-instance commands, scales and starts, times spread over
    3 s) and of the target-lookup kernel beside it: HIP events around bursts of back-to-back launches after a warm-up, the median
    over the bursts.  A library with the gait's terrain also gets wbc_gait_terrain_targets_kernel timed in the same process: the same
    planner on sixteen kerbs and stairs, each instance with its own profile and scale, FIT.  A library with the command schedules
    (include/wbc_gait_schedule.h) also gets wbc_gait_schedule_targets_kernel and wbc_gait_schedule_terrain_targets_kernel
    timed: the same planner, every instance with its own three switches inside the 3 s of sampled times, blend 0.5 -- and the plain
    kernels again once the schedule is cleared.  A library with the foot-placement feedback (include/wbc_gait_feedback.h)
    gets wbc_gait_targets_measured timed, which is the plain kernel and wbc_gait_feedback_kernel after it: two launches; the pass's
    own time is that pair's less the plain kernel's.
  loop: time per 1 ms tick of wbc_ground_rollout at 16 substeps, MPTC, with the targets looked up in a recorded trot
    (tools/follow_bench.py's; `traj`: the launches the rollout issued before it could take a gait) or computed by the gait (`gait`:
    a trot at stride scale 0.5, commands over +-0.3 m/s and +-0.5 rad/s).  One figure per process; the caller runs them in turn.  A
    library from before the gait planner (WBC_HIP_LIB) is measured with `--source traj`, which calls nothing it lacks.
    `gait_terrain`: the plant on sixteen kerbs and stairs and the gait on the same terrain (one terrain kernel per tick);
    `gait_follow`: the same ground under the plain gait with the follow law in FIT after it (two kernels per tick), the path a
    terrain gait replaces.  `gait_schedule`: `gait` steered by three switches per instance (one schedule kernel per tick).  `gait_feedback`: `gait` with the default feedback set, fed with the
    rollout's q and v (the plain kernel and the feedback kernel per tick); its state is reset before every repeat.
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

from follow_bench import _burst_us  # noqa: E402


def _planner(n, seed=1):
    import numpy as np
    import torch
    from quadruped_drake_amd.gait import GaitPlanner
    rng = np.random.default_rng(seed)
    cmd = np.stack([rng.uniform(-0.3, 0.3, n), rng.uniform(-0.1, 0.1, n), rng.uniform(-0.5, 0.5, n)])
    p = GaitPlanner("mini_cheetah", strides=("trot",), device=0)
    p.set_commands(torch.tensor(cmd, device="cuda:0"), stride_scale=torch.full((n,), 0.5, dtype=torch.float64, device="cuda:0"))
    return p


def _terrains(n, seed=2):
    """sixteen kerbs and stairs, 0.3 m ahead, and per instance a profile and a scale in 0.5 .. 1.5"""
    import numpy as np
    import torch
    from quadruped_drake_amd import terrain
    profiles = [terrain.ramp_step(0.3, 0.02 + 0.01 * k) if k % 2 == 0 else terrain.stairs(0.3, 0.2, [0.02 + 0.005 * k] * 3) for k in range(16)]
    rng = np.random.default_rng(seed)
    tid = torch.tensor((np.arange(n) % 16).astype(np.uint8), device="cuda:0")
    tsc = torch.tensor(rng.uniform(0.5, 1.5, n), device="cuda:0")
    return profiles, tid, tsc


def _schedule(p, n, seed=3):
    """three switches per instance inside the 3 s of sampled times, blend 0.5"""
    import numpy as np
    rng = np.random.default_rng(seed)
    times = np.stack([rng.uniform(0.5, 0.8, n), rng.uniform(1.4, 1.7, n), rng.uniform(2.3, 2.6, n)])
    cmds = np.stack([np.stack([rng.uniform(-0.3, 0.3, n), rng.uniform(-0.1, 0.1, n), rng.uniform(-0.5, 0.5, n)]) for _ in range(3)])
    p.set_schedule(times, cmds, blend=0.5)


def kernel(a):
    import numpy as np
    import torch
    from quadruped_drake_amd import workloads
    from quadruped_drake_amd.trajectory import TrunkTrajectory
    dev = "cuda:0"
    tm = torch.tensor(np.random.default_rng(1).uniform(0.0, 3.0, a.n), device=dev)
    p = _planner(a.n)
    out = p.targets(tm)
    res = {"n": a.n, "kernel": p.kernel_info()}
    res["gait"] = _burst_us(lambda: p.targets(tm, out=out), lambda: None, a.bursts, a.burst)
    if hasattr(p._L, "wbc_gait_set_terrain"):
        profiles, tid, tsc = _terrains(a.n)
        p.set_terrain(profiles, terrain_id=tid, terrain_scale=tsc, body="fit")
        res["terrain_kernel"] = p.terrain_kernel_info()
        res["gait_terrain"] = _burst_us(lambda: p.targets(tm, out=out), lambda: None, a.bursts, a.burst)
        p.clear_terrain()
        res["gait_after_clear"] = _burst_us(lambda: p.targets(tm, out=out), lambda: None, a.bursts, a.burst)
    if hasattr(p._L, "wbc_gait_set_schedule"):
        _schedule(p, a.n)
        res["schedule_kernel"] = p.schedule_kernel_info()
        res["gait_schedule"] = _burst_us(lambda: p.targets(tm, out=out), lambda: None, a.bursts, a.burst)
        profiles, tid, tsc = _terrains(a.n)
        p.set_terrain(profiles, terrain_id=tid, terrain_scale=tsc, body="fit")
        res["schedule_terrain_kernel"] = p.schedule_kernel_info(terrain=True)
        res["gait_schedule_terrain"] = _burst_us(lambda: p.targets(tm, out=out), lambda: None, a.bursts, a.burst)
        p.clear_schedule()
        res["gait_terrain_after_clear_schedule"] = _burst_us(lambda: p.targets(tm, out=out), lambda: None, a.bursts, a.burst)
        p.clear_terrain()
        res["gait_after_clear_schedule"] = _burst_us(lambda: p.targets(tm, out=out), lambda: None, a.bursts, a.burst)
    if hasattr(p._L, "wbc_gait_targets_measured"):
        q0, v0 = workloads.nominal_state("mini_cheetah", a.n)
        q, v = torch.tensor(q0, device=dev), torch.tensor(v0, device=dev)
        v[3] = 0.2; v[4] = 0.1                                    # a trunk off its plan: the offsets are not zero
        off = torch.zeros((8, a.n), dtype=torch.float64, device=dev)
        p.set_feedback(a.n)
        res["feedback_kernel"] = p.feedback_kernel_info()
        res["gait_measured_pair"] = _burst_us(lambda: p.targets_measured(tm, q, v, out=out), lambda: None, a.bursts, a.burst)
        res["gait_measured_pair_with_offsets"] = _burst_us(lambda: p.targets_measured(tm, q, v, out=out, offsets=off), lambda: None, a.bursts, a.burst)
        p.clear_feedback()
        res["gait_after_clear_feedback"] = _burst_us(lambda: p.targets(tm, out=out), lambda: None, a.bursts, a.burst)
    st_t = workloads.standing_targets("mini_cheetah", 1)[:, 0]
    K = 4000
    traj = TrunkTrajectory(np.arange(K) * 1e-3, np.tile(st_t, (K, 1)), np.full(K, 15, np.uint8), wait_time=0.0, device=0,
                           standing_targets=st_t, standing_mask=0b1111)
    out2 = traj.lookup(tm)
    res["lookup"] = _burst_us(lambda: traj.lookup(tm, out=out2), lambda: None, a.bursts, a.burst)
    p.close(); traj.close()
    print(json.dumps(res), flush=True)


def loop(a):
    import numpy as np
    import torch
    import ground_oracle as go
    from quadruped_drake_amd import GroundContactPlant, MPTCController, closed_loop, workloads
    from quadruped_drake_amd.trajectory import TrunkTrajectory
    n, dt, dev = a.n, 1e-3, "cuda:0"
    if a.source.startswith("gait"):
        src = _planner(n)
        if a.source == "gait_schedule":
            _schedule(src, n)
    else:
        st_t = workloads.standing_targets("mini_cheetah", 1)[:, 0]
        K = 4000
        ts = np.arange(K) * 1e-3
        tg = np.tile(st_t, (K, 1))
        tg[:, 0] += 0.01 * np.sin(2 * np.pi * ts / 0.3); tg[:, 3] = 0.01 * 2 * np.pi / 0.3 * np.cos(2 * np.pi * ts / 0.3)
        masks = np.where((np.arange(K) // 150) % 2 == 0, 0b1001, 0b0110).astype(np.uint8)
        for f in range(4):
            tg[((masks >> f) & 1) == 0, 18 + 9 * f + 2] += 0.02
        src = TrunkTrajectory(ts, tg, masks, wait_time=0.0, device=0, standing_targets=st_t, standing_mask=0b1111)
    _, q0, v0 = go.drop_state("mini_cheetah", height=0.0, n=n)
    t0 = np.random.default_rng(1).uniform(0.0, 0.6, n)
    ctrl = MPTCController(max_batch=n, device=0)
    plant = GroundContactPlant("mini_cheetah", device=0)
    if a.source in ("gait_terrain", "gait_follow"):
        profiles, tid, tsc = _terrains(n)
        plant.set_terrain(profiles, terrain_id=tid, terrain_scale=tsc)
        if a.source == "gait_terrain":
            src.set_terrain(profiles, terrain_id=tid, terrain_scale=tsc, body="fit")
        else:
            plant.set_follow("fit")
    us = []
    for _ in range(a.repeats + 1):               # every repeat from the same start: the same ticks; the first is the warm-up
        q, v, t = torch.tensor(q0, device=dev), torch.tensor(v0, device=dev), torch.tensor(t0, device=dev)
        if a.source == "gait_feedback":
            src.set_feedback(n)
        closed_loop(ctrl, plant, src, 20, dt, q, v, t)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        closed_loop(ctrl, plant, src, a.steps, dt, q, v, t)
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / a.steps)
    us = us[1:]
    res = {"source": a.source, "lib": os.environ.get("WBC_HIP_LIB", "built"), "n": n, "steps": a.steps, "substeps": plant.substeps(dt), "us_per_tick_median": statistics.median(us),
           "us_per_tick_all": us, "finite": bool(torch.isfinite(q).all())}
    plant.close(); ctrl.close(); src.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("kernel", "loop"))
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--bursts", type=int, default=30)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--source", default="traj", choices=("traj", "gait", "gait_terrain", "gait_follow", "gait_schedule", "gait_feedback"))
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    kernel(a) if a.what == "kernel" else loop(a)


if __name__ == "__main__":
    main()
