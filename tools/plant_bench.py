#!/usr/bin/env python3
"""Measurements of the rigid-contact plant step (include/wbc_plant.h) for profiles/r07/plant.md.

    python tools/plant_bench.py [--launches 400] [--json out.json]

  * wbc_plant_step device time at N = 4096 and 32768 (Mini Cheetah, trot masks): HIP events around >= 200 back-to-back launches
    after a warm-up (torch.cuda.Event on the launch stream; q and v are integrated in place, so every launch sees a new state);
  * the achieved FP64 rate from the kernel's FP64 instruction count (flops_per_robot(): the straight-line device assembly of
    wbc_plant_step_kernel that build() leaves in build/, every FP64 VALU instruction weighted by its flops, times the four lanes
    of a robot -- the base work replicated on the quad counts four times: an ISSUED figure, not the algorithm's minimum);
  * time per closed-loop tick of wbc_plant_rollout (lookup -> tick -> plant step, three launches) against the persistent
    wbc_rollout (lookup -> tick -> integrate in one launch) at N = 4096, MPTC, on bench.py's trot trajectory.
For the rocprofv3 figure run the same script under `rocprofv3 --kernel-trace --stats -- python tools/plant_bench.py --launches 200`."""
import argparse
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ASM = os.path.join(ROOT, "build", "wbc_plant-hip-amdgcn-amd-amdhsa-gfx950.s")
# flops per FP64 VALU instruction (fma = 2); transcendental seeds and conversions count 1
FP64_WEIGHT = {"v_fma_f64": 2, "v_fmac_f64": 2, "v_mul_f64": 1, "v_add_f64": 1, "v_rcp_f64": 1, "v_rsq_f64": 1, "v_sqrt_f64": 1,
               "v_div_scale_f64": 1, "v_div_fmas_f64": 2, "v_div_fixup_f64": 1, "v_ldexp_f64": 1, "v_fract_f64": 1,
               "v_max_f64": 1, "v_min_f64": 1, "v_trig_preop_f64": 1}


def flops_per_robot(asm_path=ASM, kernel="wbc_plant_step_kernel"):
    """-> (issued FP64 flops per robot, FP64 VALU instructions per lane, total instructions per lane) of the kernel body."""
    with open(asm_path) as f:
        text = f.read()
    m = re.search(r"^(_Z\d+%s\w*):" % kernel, text, re.M)
    body = text[m.end():text.index(".Lfunc_end", m.end())]
    fl = n64 = tot = 0
    for line in body.splitlines():
        tok = line.strip().split()
        if not tok or tok[0].startswith((".", ";")) or tok[0].endswith(":"):
            continue
        tot += 1
        op = re.sub(r"_e(32|64)$", "", tok[0])
        if op in FP64_WEIGHT:
            fl += FP64_WEIGHT[op]; n64 += 1
    return 4 * fl, n64, tot


def trot_case(n, model="mini_cheetah", seed=3):
    import numpy as np
    from quadruped_drake_amd import workloads
    b = workloads.make_batch(3, n=n, seed=seed, model=model)
    tau = np.random.default_rng(seed).uniform(-20.0, 20.0, (12, n))
    return b, tau


def time_plant_step(n, launches, warm=20):
    import torch
    from quadruped_drake_amd import RigidContactPlant
    b, tau = trot_case(n)
    dev = "cuda:0"
    q, v = torch.tensor(b["q"], device=dev), torch.tensor(b["v"], device=dev)
    tau_d, mk = torch.tensor(tau, device=dev), torch.tensor(b["mask"], device=dev)
    plant = RigidContactPlant("mini_cheetah", device=0)
    out = plant.step(q, v, tau_d, mk, 1e-4)
    for _ in range(warm - 1):
        plant.step(q, v, tau_d, mk, 1e-4, out=out)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        plant.step(q, v, tau_d, mk, 1e-4, out=out)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / launches
    flags = out[2].cpu().numpy()
    info = plant.kernel_info()
    plant.close()
    return {"n": n, "us_per_step": us, "launches": launches, "bad": int(((flags & 8) != 0).sum()), "kernel": info}


def time_loops(n, steps, dt=1e-3):
    import numpy as np
    import torch
    from quadruped_drake_amd import MPTCController, RigidContactPlant, closed_loop, workloads
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
    rng = np.random.default_rng(1)
    q0, v0 = workloads.nominal_state("mini_cheetah", n)
    q0[7:] += rng.uniform(-0.03, 0.03, (12, n))
    t0 = rng.uniform(0.0, 0.6, n)
    dev = "cuda:0"
    res = {}
    for name in ("wbc_rollout", "wbc_plant_rollout"):
        ctrl = MPTCController(max_batch=n, device=0)
        plant = RigidContactPlant("mini_cheetah", device=0)
        q, v, t = torch.tensor(q0, device=dev), torch.tensor(v0, device=dev), torch.tensor(t0, device=dev)
        run = (lambda k: ctrl.rollout(traj, k, dt, q, v, t)) if name == "wbc_rollout" else \
              (lambda k: closed_loop(ctrl, plant, traj, k, dt, q, v, t))
        run(20)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(steps)
        e1.record()
        torch.cuda.synchronize()
        res[name] = {"us_per_tick": e0.elapsed_time(e1) * 1e3 / steps, "steps": steps,
                     "final_height_mean": float(q[6].mean()), "finite": bool(torch.isfinite(q).all())}
        plant.close(); ctrl.close()
    res["ratio"] = res["wbc_plant_rollout"]["us_per_tick"] / res["wbc_rollout"]["us_per_tick"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=400)
    ap.add_argument("--loop-steps", type=int, default=300)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    out = {}
    if os.path.exists(ASM):
        fl, n64, tot = flops_per_robot()
        out["count"] = {"issued_fp64_flops_per_robot": fl, "fp64_valu_per_lane": n64, "instructions_per_lane": tot}
    for n in (4096, 32768):
        r = time_plant_step(n, a.launches)
        if "count" in out:
            r["fp64_tflops"] = out["count"]["issued_fp64_flops_per_robot"] * n / (r["us_per_step"] * 1e-6) / 1e12
        out["plant_step_%d" % n] = r
        print(json.dumps(r), flush=True)
    out["closed_loop_4096_mptc"] = time_loops(4096, a.loop_steps)
    print(json.dumps(out["closed_loop_4096_mptc"]), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out.get("count", {})))


if __name__ == "__main__":
    main()
