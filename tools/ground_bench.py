#!/usr/bin/env python3
"""Measurements of the compliant-ground plant (include/wbc_ground.h) for profiles/r08/ground.md.

    python tools/ground_bench.py [--launches 100] [--loop-steps 300] [--json out.json] [--terrain NAME[:PARAM]]

  * wbc_ground_step device time at N = 4096 and 32768 (Mini Cheetah standing on the ground, zero torque) with S = 8 and S = 16
    substeps of a 1 ms period: HIP events around back-to-back launches after a warm-up.  Per step, and per substep as
    (t(S = 16) - t(S = 8)) / 8, which leaves out the launch and the one load / store of the state;
  * the yardstick, timed in the same run: the rigid plant's wbc_plant_step (tools/plant_bench.py's time_plant_step);
  * time per 1 ms closed-loop tick at N = 4096, MPTC on plant_bench's trot trajectory: wbc_ground_rollout (default 16 substeps)
    against wbc_plant_rollout (the three-launch loop with the rigid plant) and the persistent wbc_rollout.
With --terrain (terrain.SPECS, e.g. slope:0.1) only the N = 4096 step is timed, flat and on the terrain back to back, with
the per-substep ratio of the two and the resources of both step kernels.
For the rocprofv3 figure run the same script under `rocprofv3 --kernel-trace --stats -- python tools/ground_bench.py`."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def time_ground_step(n, substeps, launches, warm=10, dt=1e-3, model="mini_cheetah", terrain=None):
    import numpy as np
    import torch
    import ground_oracle as go
    from quadruped_drake_amd import GroundContactPlant
    _, q0, v0 = go.drop_state(model, height=0.0, n=n)
    if terrain is not None:      # square on the terrain, spread along it, every second robot on a ground scaled by 0.5
        from quadruped_drake_amd import terrain as tr
        prof = tr.from_spec(terrain)
        scale = np.where(np.arange(n) % 2 == 0, 1.0, 0.5)
        for i, x in enumerate(np.linspace(-1.0, 1.0, n)):
            quat, pos = tr.stance_pose(prof, x, 0.0, q0[6, i], scale[i])
            q0[0:4, i], q0[4:7, i] = quat, pos
    q0[7:] += np.random.default_rng(1).uniform(-0.02, 0.02, (12, n))
    dev = "cuda:0"
    q, v = torch.tensor(q0, device=dev), torch.tensor(v0, device=dev)
    tau = torch.zeros((12, n), dtype=torch.float64, device=dev)
    plant = GroundContactPlant(model, device=0, max_substep=dt / substeps)
    assert plant.substeps(dt) == substeps
    if terrain is not None:
        plant.set_terrain([tr.flat(0.0), prof], torch.ones(n, dtype=torch.uint8, device=dev), torch.tensor(scale, device=dev))
    out = plant.step(q, v, tau, dt)
    for _ in range(warm):
        plant.step(q, v, tau, dt, out=out)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        plant.step(q, v, tau, dt, out=out)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / launches
    flags = out[2].cpu().numpy()
    info = plant.kernel_info() if terrain is None else plant.terrain_kernel_info()
    plant.close()
    return {"n": n, "substeps": substeps, "terrain": terrain, "us_per_step": us, "launches": launches, "bad": int(((flags & 8) != 0).sum()),
            "fell": int(((flags & 2) != 0).sum()), "kernel": info}


def time_ground_loop(n, steps, dt=1e-3):
    """MPTC on plant_bench's trot trajectory over the compliant ground (default parameters: 16 substeps per tick)."""
    import numpy as np
    import torch
    import ground_oracle as go
    from quadruped_drake_amd import GroundContactPlant, MPTCController, closed_loop, workloads
    from quadruped_drake_amd.trajectory import TrunkTrajectory
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
    dev = "cuda:0"
    ctrl = MPTCController(max_batch=n, device=0)
    plant = GroundContactPlant("mini_cheetah", device=0)
    q, v, t = torch.tensor(q0, device=dev), torch.tensor(v0, device=dev), torch.tensor(t0, device=dev)
    counts = torch.zeros((4, n), dtype=torch.int32, device=dev)
    closed_loop(ctrl, plant, traj, 20, dt, q, v, t, counts=counts)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    closed_loop(ctrl, plant, traj, steps, dt, q, v, t, counts=counts)
    e1.record()
    torch.cuda.synchronize()
    c = counts.cpu().numpy()
    res = {"us_per_tick": e0.elapsed_time(e1) * 1e3 / steps, "steps": steps, "substeps": plant.substeps(dt),
           "final_height_mean": float(q[6].mean()), "finite": bool(torch.isfinite(q).all()),
           "instances_with": {"slip": int((c[0] > 0).sum()), "fell": int((c[1] > 0).sum()), "bad": int((c[3] > 0).sum())}}
    plant.close(); ctrl.close()
    return res


def main():
    import plant_bench
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--loop-steps", type=int, default=300)
    ap.add_argument("--json", default=None)
    ap.add_argument("--terrain", default=None, help="NAME[:PARAM] of quadruped_drake_amd.terrain.SPECS: time the N = 4096 step flat and on it")
    a = ap.parse_args()
    out = {}
    if a.terrain:
        per = {}
        for rep_ in range(2):                    # flat, terrain, flat, terrain: the second pair is the figure, the first shows the drift
            for name, ter in (("flat", None), ("terrain", a.terrain)):
                s = {sub: time_ground_step(4096, sub, a.launches, terrain=ter) for sub in (8, 16)}
                per[name] = (s[16]["us_per_step"] - s[8]["us_per_step"]) / 8.0
                for sub in (8, 16):
                    out["%s_step_4096_S%d_run%d" % (name, sub, rep_)] = s[sub]
                    print(json.dumps(s[sub]), flush=True)
            out["substep_4096_run%d" % rep_] = {"flat_us": per["flat"], "terrain_us": per["terrain"], "ratio": per["terrain"] / per["flat"]}
            print(json.dumps(out["substep_4096_run%d" % rep_]), flush=True)
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, "w") as f:
                json.dump(out, f, indent=1)
        return
    for n in (4096, 32768):
        r = plant_bench.time_plant_step(n, 4 * a.launches)
        out["plant_step_%d" % n] = r
        print(json.dumps(r), flush=True)
        s = {}
        for sub in (8, 16):
            s[sub] = time_ground_step(n, sub, a.launches)
            out["ground_step_%d_S%d" % (n, sub)] = s[sub]
            print(json.dumps(s[sub]), flush=True)
        per = (s[16]["us_per_step"] - s[8]["us_per_step"]) / 8.0
        out["substep_%d" % n] = {"us_per_substep": per, "plant_step_us": r["us_per_step"], "ratio_to_plant_step": per / r["us_per_step"]}
        print(json.dumps(out["substep_%d" % n]), flush=True)
    out["rigid_loops_4096_mptc"] = plant_bench.time_loops(4096, a.loop_steps)
    print(json.dumps(out["rigid_loops_4096_mptc"]), flush=True)
    out["ground_loop_4096_mptc"] = time_ground_loop(4096, a.loop_steps)
    print(json.dumps(out["ground_loop_4096_mptc"]), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
