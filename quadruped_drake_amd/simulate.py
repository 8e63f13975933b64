"""Batch counterpart of the reference's entry script (simulate.py): the same "common parameters" -- planning method,
control method, sim_time, dt -- and the same log (`output_metrics` = [V, err, res, Vdot], simulate.py:142,184-215), for
N robot instances at once on one MI355X, closed loop on the device.

    python -m quadruped_drake_amd.simulate --control ID --planner basic --scenario raise_foot --n 4096 --sim-time 2

What replaces what: the initial state is simulate.py:171-179; `--planner basic` serves one of the reference's scenarios
(planners/simple.py), `--planner towr --messages FILE` a recorded stream of 549-byte `trunk_state` messages
(planners/towr.py; TOWR itself is out of scope); the controller is the fused tick; Drake's MultibodyPlant(time_step=dt)
and contact solver (simulate.py:38-64) are replaced by the rigid-contact forward step of `wbc_rollout` (DESIGN.md
section 9: stance feet are held by the QP's contact rows, nothing slips or lifts on its own) -- a harness for the
controllers, not a physics engine.  No visualiser, no LCM.

`--plant` chooses what the torques act on: `plan` (the default, the above), `rigid` (plant.RigidContactPlant: stance feet held,
PULL / CONE reported) or `ground` (plant.GroundContactPlant: a compliant ground on which feet lift, land and slip and a robot
can fall).  `--terrain NAME[:PARAM]` (with `--plant ground` only; terrain.SPECS) puts a slope, a ramp step, stairs or a ridge
under the feet.  `--follow lift|fit` (with `--terrain` only; default `off`) makes the planner's level-ground targets follow that ground
between the lookup and the tick: `lift` raises the foot and trunk heights, `fit` also turns the trunk's attitude with the line
fitted through the planned footholds (include/wbc_ground.h).  The footholds are not re-planned and the controllers' friction pyramids
stay about world z.

`--planner gait --gait NAME --cmd VX,VY,WZ [--cmd-spread DVX,DVY,DWZ] [--stride-scale S]` (every `--plant` but `plan`) makes the robots
WALK: gait.GaitPlanner computes each tick's targets on the device from a velocity command in the heading frame and a yaw rate
(include/wbc_gait.h).  Instance i gets a command drawn uniformly in cmd +- spread from `--seed`.  NAME is one of TOWR's strides
(gait.STRIDES); S scales the stride's durations and defaults to 0.5: ID at TOWR's own 1.0 s trot falls when it steps in place, walks
backwards or climbs a slope of grade 0.2, and walks all of them at half that period (profiles/r13/gait.md, gait_sweep.md).  With
`--plant ground` the result line also has the mean and the worst distance of the trunks from their planned (x, y).
`--cmd-schedule "T:VX,VY,WZ;..." [--cmd-blend B]` (with `--planner gait`) steers every robot: from T seconds on it walks VX,VY,WZ, with a
smooth turn of length B (default 0.5) after each of up to seven switches (include/wbc_gait_schedule.h); `--cmd-spread`
spreads the first command only.
`--gait-terrain lift|fit` (with `--planner gait` and `--terrain`; default `off`; excludes `--follow`) gives the plant's terrain to the
planner (include/wbc_gait_terrain.h): footholds on the surface and off the risers, swings that clear what lies between
their footholds, a body that follows the feet (`fit`: also in pitch and roll).  That is what walks a kerb of 0.1 m.
`--gait-feedback [KV,KP,DMAX,UHOLD]` (with `--planner gait`, without `--gait-terrain`) lets the footholds react to the measured trunk
(include/wbc_gait_feedback.h): a velocity gain [s], a position gain, the largest offset [m] and the swing fraction up to
which a landing point still moves; without a value, wbc_gait_feedback_params_default's.  `--push T0:T1:FX,FY` (with `--plant ground`)
applies the world force FX,FY [N] to every trunk during [T0, T1) seconds, by splitting the rollout into calls at T0 and T1."""
import argparse
import json
import sys

import numpy as np

CONTROL = ("ID", "MPTC", "PC", "CLF")


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--control", default="ID", choices=CONTROL, help="control_method (simulate.py:13)")
    ap.add_argument("--planner", default="basic", choices=("basic", "towr", "gait"),
                    help="planning_method (simulate.py:12); gait: walking targets from a velocity command, computed on the device")
    ap.add_argument("--scenario", default="standing", help="basic planner: standing | orientation | raise_foot | edge")
    ap.add_argument("--messages", default=None, help="towr planner: file of concatenated 549-byte trunk_state messages")
    ap.add_argument("--gait", default="trot", help="gait planner: the stride, one of gait.STRIDES (TOWR's stride tables)")
    ap.add_argument("--cmd", default="0.2,0,0", help="gait planner: VX,VY,WZ -- velocity in the heading frame [m/s] and yaw rate [rad/s]")
    ap.add_argument("--cmd-spread", default="0,0,0", help="gait planner: DVX,DVY,DWZ -- instance i's command is uniform in cmd +- spread")
    ap.add_argument("--stride-scale", type=float, default=0.5,
                    help="gait planner: the stride's durations times this; 0.5 because ID falls at TOWR's 1.0 s trot when it steps in "
                         "place, walks backwards or climbs, and walks all of them at 0.5 s (module docstring)")
    ap.add_argument("--sim-time", type=float, default=6.0, help="sim_time (simulate.py:20)")
    ap.add_argument("--dt", type=float, default=None, help="dt (simulate.py:21: 5e-3; MPTC / PC default to 1e-3, DESIGN.md section 9)")
    ap.add_argument("--n", type=int, default=1, help="robot instances")
    ap.add_argument("--perturb", type=float, default=0.0, help="uniform joint-angle perturbation of instances 1.. (rad)")
    ap.add_argument("--model", default="mini_cheetah")
    ap.add_argument("--log-every", type=int, default=10, help="ticks between two samples of the metrics log")
    ap.add_argument("--log", default=None, help="write the log (t, V, err, res, Vdot of every instance) to this .npz")
    ap.add_argument("--plant", default="plan", choices=("plan", "rigid", "ground"),
                    help="what the torques act on: the controller's own plan, the rigid-contact plant or the compliant-ground plant")
    ap.add_argument("--terrain", default=None, help="--plant ground only: NAME[:PARAM], e.g. slope:0.2 (flat, slope, ramp_step, stairs, ridge)")
    ap.add_argument("--follow", default="off", choices=("off", "lift", "fit"),
                    help="--terrain only: make the targets follow the ground (lift: heights; fit: heights and the trunk's attitude)")
    ap.add_argument("--cmd-schedule", default=None,
                    help="gait planner: T:VX,VY,WZ;... -- from T [s] on walk VX,VY,WZ; up to 7 switches, at rising times from 0.5 s (the ramp) on")
    ap.add_argument("--cmd-blend", type=float, default=0.5, help="--cmd-schedule: the length of the smooth turn after a switch [s]")
    ap.add_argument("--gait-terrain", default="off", choices=("off", "lift", "fit"),
                    help="--planner gait with --terrain only: the planner walks ON the terrain (lift: body height; fit: and its attitude)")
    ap.add_argument("--gait-feedback", nargs="?", const="default", default=None,
                    help="gait planner: footholds react to the measured trunk; optional KV,KP,DMAX,UHOLD (default: the capture-point gain)")
    ap.add_argument("--push", default=None, help="--plant ground only: T0:T1:FX,FY -- a world force [N] on every trunk during [T0, T1) s")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)
    if a.dt is None:
        a.dt = 5e-3 if a.control in ("ID", "CLF") else 1e-3
    if a.planner == "towr" and not a.messages:
        ap.error("--planner towr needs --messages FILE (a recorded trunk_state stream)")
    if a.planner == "gait":
        from . import gait
        if a.plant == "plan":
            ap.error("--planner gait needs --plant rigid or --plant ground (the plan's own rollout looks its targets up in a trajectory)")
        if a.gait not in gait.STRIDES:
            ap.error("--gait %s: expected one of %s" % (a.gait, ", ".join(gait.STRIDES)))
        for name in ("cmd", "cmd_spread"):
            try:
                val = tuple(float(x) for x in getattr(a, name).split(","))
            except ValueError:
                val = ()
            if len(val) != 3 or not all(np.isfinite(val)) or (name == "cmd_spread" and min(val) < 0):
                ap.error("--%s: expected three finite numbers A,B,C%s" % (name.replace("_", "-"), " >= 0" if name == "cmd_spread" else ""))
            setattr(a, name, val)
        if not (a.stride_scale > 0 and np.isfinite(a.stride_scale)):
            ap.error("--stride-scale must be positive and finite")
        if a.cmd_schedule is not None:
            try:
                items = [(float(t), tuple(float(x) for x in c.split(","))) for t, c in (item.split(":") for item in a.cmd_schedule.split(";"))]
            except ValueError:
                items = []
            ok = 1 <= len(items) <= gait.MAX_SWITCHES and all(len(c) == 3 and np.isfinite(t) and all(np.isfinite(c)) for t, c in items)
            if not ok or not (a.cmd_blend >= 0 and np.isfinite(a.cmd_blend)):
                ap.error("--cmd-schedule: expected 1 .. 7 items T:VX,VY,WZ separated by ';', and --cmd-blend >= 0")
            if items[0][0] < 0.5 or any(t1 < t0 + a.cmd_blend for (t0, _), (t1, _) in zip(items, items[1:])):
                ap.error("--cmd-schedule: the first switch at 0.5 s (the ramp) or later, every other at least --cmd-blend after the one before")
            a.cmd_schedule = items
    if a.cmd_schedule is not None and a.planner != "gait":
        ap.error("--cmd-schedule needs --planner gait")
    if a.gait_feedback is not None:
        if a.planner != "gait":
            ap.error("--gait-feedback needs --planner gait")
        if a.gait_terrain != "off":
            ap.error("--gait-feedback excludes --gait-terrain: the feedback knows no terrain")
        if a.gait_feedback == "default":
            a.gait_feedback = {}
        else:
            try:
                val = tuple(float(x) for x in a.gait_feedback.split(","))
            except ValueError:
                val = ()
            if len(val) != 4 or not all(np.isfinite(val)) or min(val) < 0 or val[2] == 0 or val[3] > 1:
                ap.error("--gait-feedback: expected KV,KP,DMAX,UHOLD, finite and >= 0, DMAX > 0, UHOLD <= 1")
            a.gait_feedback = dict(zip(("k_v", "k_p", "d_max", "u_hold"), val))
    if a.push is not None:
        if a.plant != "ground":
            ap.error("--push needs --plant ground")
        try:
            t0, t1, f = a.push.split(":")
            val = (float(t0), float(t1)) + tuple(float(x) for x in f.split(","))
        except ValueError:
            val = ()
        if len(val) != 4 or not all(np.isfinite(val)) or not 0 <= val[0] < val[1]:
            ap.error("--push: expected T0:T1:FX,FY with 0 <= T0 < T1, all finite")
        a.push = val
    if a.terrain is not None:
        if a.plant != "ground":
            ap.error("--terrain needs --plant ground")
        from . import terrain
        try:
            terrain.from_spec(a.terrain)
        except ValueError as e:
            ap.error(str(e))
    if a.follow != "off" and a.terrain is None:
        ap.error("--follow needs --terrain")
    if a.gait_terrain != "off":
        if a.planner != "gait" or a.terrain is None:
            ap.error("--gait-terrain needs --planner gait and --terrain")
        if a.follow != "off":
            ap.error("--gait-terrain excludes --follow: the planner's targets are finished, following would lift them twice")
    if a.n < 1 or a.sim_time <= 0 or a.dt <= 0 or a.log_every < 1:
        ap.error("--n, --sim-time, --dt and --log-every must be positive")
    return a


def draw_commands(a, n):
    """cmd [3, n]: instance i's (vx, vy, yaw rate), uniform in a.cmd +- a.cmd_spread from a.seed"""
    u = np.random.default_rng([a.seed, 0x6A17]).uniform(-1.0, 1.0, (3, n))
    return np.array(a.cmd)[:, None] + np.array(a.cmd_spread)[:, None] * u


def run(a):
    """-> dict(t [S], metrics [S, 4, n], status_nonzero, ticks, q [19, n], v [18, n], ticks_per_second)"""
    import time as _time
    import torch
    from . import CLFController, IDController, MPTCController, PCController, workloads
    from .planners import TowrTrunkPlanner, scenario_trajectory
    cls = {"ID": IDController, "MPTC": MPTCController, "PC": PCController, "CLF": CLFController}[a.control]
    dev = "cuda:%d" % a.device
    cmd = None
    if a.planner == "gait":
        from .gait import GaitPlanner
        traj = GaitPlanner(a.model, strides=(a.gait,), device=a.device)
        cmd = draw_commands(a, a.n)
    elif a.planner == "basic":
        traj = scenario_trajectory(a.scenario, a.sim_time, a.dt, model=a.model, device=a.device)
    else:
        raw = open(a.messages, "rb").read()
        if len(raw) % 549:
            raise ValueError("%s: not a whole number of 549-byte trunk_state messages" % a.messages)
        traj = TowrTrunkPlanner([raw[i:i + 549] for i in range(0, len(raw), 549)], model=a.model).trajectory(a.device)
    q0, v0 = workloads.nominal_state(a.model, a.n)                      # simulate.py:171-179
    if a.perturb > 0 and a.n > 1:
        q0[7:, 1:] += np.random.default_rng(a.seed).uniform(-a.perturb, a.perturb, (12, a.n - 1))
    ctrl = cls(model=a.model, max_batch=a.n, device=a.device)
    plant = counts = None
    if a.plant != "plan":
        from . import plant as plant_mod
        if a.plant == "rigid":
            plant = plant_mod.RigidContactPlant(a.model, device=a.device)
        else:
            plant = plant_mod.GroundContactPlant(a.model, device=a.device)
            if a.terrain is not None:
                from . import terrain
                prof = terrain.from_spec(a.terrain)
                plant.set_terrain([prof])
                plant.set_follow(a.follow)
                quat, pos = terrain.stance_pose(prof, 0.0, 0.0, float(q0[6, 0]))     # square on the ground under the start
                q0[0:4] = quat[:, None]; q0[4:7] = pos[:, None]
                if a.gait_terrain != "off":
                    traj.set_terrain([prof], body=a.gait_terrain)
        counts = torch.zeros((4, a.n), dtype=torch.int32, device=dev)
    q, v = torch.tensor(q0, device=dev), torch.tensor(v0, device=dev)
    time = torch.zeros(a.n, dtype=torch.float64, device=dev)
    if cmd is not None:                 # the plan starts where the trunk stands (on a terrain: off the origin, along the normal)
        traj.set_commands(torch.tensor(cmd, device=dev), stride_scale=torch.full((a.n,), a.stride_scale, dtype=torch.float64, device=dev),
                          start=torch.tensor(np.stack([q0[4], q0[5], np.zeros(a.n)]), device=dev))
        if a.cmd_schedule is not None:
            traj.set_schedule([t for t, _ in a.cmd_schedule], [c for _, c in a.cmd_schedule], blend=a.cmd_blend)
        if a.gait_feedback is not None:
            traj.set_feedback(a.n, **a.gait_feedback)
    steps = int(round(a.sim_time / a.dt))
    push, edges = None, ()
    if a.push is not None:              # the force is an argument of a rollout call: the calls are split at its two ends
        edges = (int(round(a.push[0] / a.dt)), int(round(a.push[1] / a.dt)))
        w = np.zeros((6, a.n)); w[3] = a.push[2]; w[4] = a.push[3]
        push = torch.tensor(w, device=dev)
    ts, mets = [], []
    ctrl.stats(reset=True)
    ctrl.sync(); t0 = _time.perf_counter()
    done = 0
    while done < steps:
        k = min([a.log_every, steps - done] + [e - done for e in edges if e > done])
        pushing = push is not None and edges[0] <= done < edges[1]
        if plant is None:
            tau, met, st, tg, mk = ctrl.rollout(traj, k, a.dt, q, v, time)
        else:
            met = plant_mod.closed_loop(ctrl, plant, traj, k, a.dt, q, v, time, counts=counts, **(dict(ext_wrench=push) if pushing else {}))[1]
        done += k
        ts.append(done * a.dt); mets.append(met.clone())
    ctrl.sync(); wall = _time.perf_counter() - t0
    s = ctrl.stats()
    out = dict(t=np.array(ts), metrics=torch.stack(mets).cpu().numpy(), status_nonzero=int(s["status_nonzero"]),
               ticks=int(s["ticks"]), q=q.cpu().numpy(), v=v.cpu().numpy(), ticks_per_second=s["ticks"] / wall,
               iters_mean=s["iters_sum"] / max(s["ticks"], 1.0))
    if plant is not None:
        c = counts.cpu().numpy()
        names = ("slip", "fell", "clip", "bad") if a.plant == "ground" else ("pull", "cone", "clip", "bad")
        out["plant_flags"] = {nm: int((c[b] > 0).sum()) for b, nm in enumerate(names)}      # instances that ever raised the flag
        plant.close()
    if cmd is not None:                 # the distance of every trunk from where the law puts the body at the final time
        plan = traj.targets(time)[0][0:2]
        off = torch.linalg.norm(q[4:6] - plan, dim=0).cpu().numpy()
        out["plan_offset"] = {"mean": float(np.nanmean(off)), "worst": float(np.nanmax(off))}
    ctrl.close(); traj.close()
    return out


def main(argv=None):
    a = parse(argv)
    r = run(a)
    if a.log:
        np.savez_compressed(a.log, t=r["t"], V=r["metrics"][:, 0], err=r["metrics"][:, 1], res=r["metrics"][:, 2],
                            Vdot=r["metrics"][:, 3], q=r["q"], v=r["v"])
    m = r["metrics"]
    extra = {}
    if a.plant != "plan":
        extra = {"plant": a.plant, "terrain": a.terrain, "plant_flags": r["plant_flags"]}
        if a.plant == "ground":
            extra.update(follow=a.follow, gait_terrain=a.gait_terrain, FELL=r["plant_flags"]["fell"], SLIP=r["plant_flags"]["slip"])
        if "plan_offset" in r:
            extra.update(gait=a.gait, cmd=list(a.cmd), cmd_spread=list(a.cmd_spread), stride_scale=a.stride_scale,
                         plan_offset_mean=r["plan_offset"]["mean"], plan_offset_worst=r["plan_offset"]["worst"])
            if a.cmd_schedule is not None:
                extra.update(cmd_schedule=[[t] + list(c) for t, c in a.cmd_schedule], cmd_blend=a.cmd_blend)
            if a.gait_feedback is not None:
                extra.update(gait_feedback=a.gait_feedback)
        if a.push is not None:
            extra.update(push=list(a.push))
    print(json.dumps({"control": a.control, "planner": a.planner, "scenario": a.scenario if a.planner == "basic" else a.gait if a.planner == "gait" else a.messages,
                      "n": a.n, "sim_time": a.sim_time, "dt": a.dt, "ticks": r["ticks"], "status_nonzero": r["status_nonzero"],
                      "ticks_per_second": r["ticks_per_second"], "active_set_iterations_mean": r["iters_mean"],
                      "final": {"V": float(m[-1, 0].mean()), "err": float(m[-1, 1].mean()), "Vdot": float(m[-1, 3].mean())},
                      "body_height_final": [float(r["q"][6].min()), float(r["q"][6].max())], **extra}))
    return 0 if r["status_nonzero"] == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
