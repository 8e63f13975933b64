#!/usr/bin/env python3
"""Which commands can the controllers walk?  One closed_loop of N = 4096 robots per case: a 64 x 64 grid of commands (vx, yaw rate),
a trot of gait.GaitPlanner, 3 s on the compliant ground -- per law (ID at dt 5 ms, MPTC at 1 ms), per stride scale (TOWR's 1.0 s trot
and half of it), on the plane and on `slope:0.2` with `--follow fit`.

    python tools/gait_sweep.py [--out profiles/r13/gait_sweep.md] [--sim-time 3] [--vx 0.8] [--wz 2.0] [--laws ID,MPTC]

Writes a markdown file with one map per case: a row per yaw rate (top: +wz), a column per vx (left: -vx); `.` ended without FELL or
BAD and within 0.03 m of its planned (x, y), `o` likewise but farther from the plan, `F` fell, `B` turned BAD, `s` answered a
non-zero status at the last tick (and nothing worse).  One JSON line per case goes to stdout."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIDE = 64


def case(law, dt, scale, spec, a):
    """-> (summary dict, the map's lines)"""
    import numpy as np
    import torch
    from quadruped_drake_amd import GroundContactPlant, IDController, MPTCController, closed_loop, terrain, workloads
    from quadruped_drake_amd.gait import GaitPlanner
    n, dev = SIDE * SIDE, "cuda:0"
    vx = np.linspace(-a.vx, a.vx, SIDE)
    wz = np.linspace(a.wz, -a.wz, SIDE)
    cmd = np.stack([np.tile(vx, SIDE), np.zeros(n), np.repeat(wz, SIDE)])
    q0, v0 = workloads.nominal_state(a.model, n)
    plant = GroundContactPlant(a.model, device=0)
    if spec is not None:
        prof = terrain.from_spec(spec)
        plant.set_terrain([prof])
        plant.set_follow("fit")
        quat, pos = terrain.stance_pose(prof, 0.0, 0.0, float(q0[6, 0]))
        q0[0:4] = quat[:, None]; q0[4:7] = pos[:, None]
    planner = GaitPlanner(a.model, strides=("trot",), device=0)
    start = np.stack([q0[4], q0[5], np.zeros(n)])               # the plan starts where the trunk stands
    planner.set_commands(torch.tensor(cmd, device=dev), stride_scale=torch.full((n,), scale, dtype=torch.float64, device=dev),
                         start=torch.tensor(start, device=dev))
    ctrl = (IDController if law == "ID" else MPTCController)(model=a.model, max_batch=n, device=0)
    q, v, tm = torch.tensor(q0, device=dev), torch.tensor(v0, device=dev), torch.zeros(n, dtype=torch.float64, device=dev)
    counts = torch.zeros((4, n), dtype=torch.int32, device=dev)
    steps = int(round(a.sim_time / dt))
    out = closed_loop(ctrl, plant, planner, steps, dt, q, v, tm, counts=counts)
    torch.cuda.synchronize()
    plan = planner.targets(tm)[0][0:2]
    off = torch.linalg.norm(q[4:6] - plan, dim=0).cpu().numpy()
    c, status = counts.cpu().numpy(), out[2].cpu().numpy()
    fell, bad = c[1] > 0, c[3] > 0
    mark = np.where(bad, "B", np.where(fell, "F", np.where(status != 0, "s", np.where(off < 0.03, ".", "o"))))
    lines = ["".join(mark[r * SIDE:(r + 1) * SIDE]) for r in range(SIDE)]
    ok = ~(bad | fell)
    walked = ok & (status == 0) & (off < 0.03)
    res = {"law": law, "dt": dt, "stride_scale": scale, "terrain": spec, "n": n, "steps": steps, "walked": int(walked.sum()),
           "fell": int(fell.sum()), "bad": int(bad.sum()), "slip": int((c[0] > 0).sum()),
           "vx_walked": [float(cmd[0][walked].min()), float(cmd[0][walked].max())] if walked.any() else None,
           "wz0_row": lines[SIDE // 2]}
    plant.close(); planner.close(); ctrl.close()
    return res, lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13", "gait_sweep.md"))
    ap.add_argument("--sim-time", type=float, default=3.0)
    ap.add_argument("--vx", type=float, default=0.8)
    ap.add_argument("--wz", type=float, default=2.0)
    ap.add_argument("--model", default="mini_cheetah")
    ap.add_argument("--laws", default="ID,MPTC")
    a = ap.parse_args()
    text = ["# Commands the controllers can walk: a trot on the compliant ground, %g s, %s" % (a.sim_time, a.model), "",
            "Written by `tools/gait_sweep.py`.  Rows: yaw rate from +%g (top) to -%g rad/s; columns: vx from -%g (left) to +%g m/s; vy = 0."
            % (a.wz, a.wz, a.vx, a.vx),
            "`.` no FELL, no BAD, within 0.03 m of the plan; `o` the same but farther from the plan; `F` fell; `B` BAD; `s` a non-zero status at the last tick.", ""]
    for law in a.laws.split(","):
        dt = 5e-3 if law == "ID" else 1e-3
        for scale in (1.0, 0.5):
            for spec in (None, "slope:0.2"):
                res, lines = case(law, dt, scale, spec, a)
                print(json.dumps(res), flush=True)
                text += ["## %s, dt %g ms, stride scale %g (period %g s), %s" % (law, dt * 1e3, scale, scale,
                                                                                "the plane" if spec is None else spec + ", follow fit"), "",
                         "walked %d of %d; fell %d, BAD %d" % (res["walked"], res["n"], res["fell"], res["bad"]), "", "```"] + lines + ["```", ""]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(text))


if __name__ == "__main__":
    main()
