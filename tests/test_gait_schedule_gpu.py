"""The gait planner's command schedules on the MI355X (include/wbc_gait_schedule.h; gait.GaitPlanner.set_schedule):
wbc_gait_schedule_targets_kernel and wbc_gait_schedule_terrain_targets_kernel against the host instantiation of the same law
(tests/host_gait_schedule.py) at the bars of tests/test_gait_schedule_cpu.py, their resources, the plain kernels' bits behind m = 0
and behind a cleared schedule, invalid schedules in every robot slot of a wavefront, a scheduled gait as the target source of
wbc_ground_rollout against the same launches issued by hand, and ID turning, stopping and reversing on the compliant ground."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import follow_oracle as fo
import gait_oracle as go
import gait_schedule_oracle as gso
import gait_terrain_oracle as gto
import host_gait as hg
import host_gait_schedule as hgs
import plant_edges as pe
import test_gait_cpu as tgc
import test_gait_terrain_cpu as tgt
from quadruped_drake_amd import _lib, gait, terrain as tr, workloads
from test_gait_gpu import DEV, LD, MODEL, NAMES, SIXTEEN, _loop, _ptr, _sync, _t
from test_gait_schedule_cpu import BLEND, NEAR, REVERSE, TURN, host_walk
from test_gait_terrain_gpu import RawTerrainGait

pytestmark = pytest.mark.gpu


class RawScheduleGait(RawTerrainGait):
    """RawTerrainGait with wbc_gait_set_schedule, whose arrays are freed before the targets are asked for"""

    def scheduled(self, n, ld, time, cmd, gid, sc, st, blend, m, when, cmds, ns=None, fill=7.5):
        """-> (targets [54, ld], mask [ld]) under the schedule set for ns (default n) instances; padding columns preset as RawGait's"""
        import torch
        keep = [_t(time), _t(cmd), None if gid is None else _t(gid), None if sc is None else _t(sc), None if st is None else _t(st)]
        _lib.check(self.L.wbc_gait_set_commands(self.h, *[_ptr(a) for a in keep[1:]]))
        s = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
        arrays = [_t(np.ascontiguousarray(m, dtype=np.uint8)), _t(when), _t(cmds)]
        _lib.check(self.L.wbc_gait_set_schedule(self.h, s, n if ns is None else ns, ld, float(blend), *[_ptr(a) for a in arrays]))
        for a in arrays:
            a.fill_(255 if a.dtype == torch.uint8 else math.nan)       # the call copied what it needs
        del arrays
        tg = torch.full((54, ld), fill, dtype=torch.float64, device=DEV)
        mk = torch.full((ld,), 0x55, dtype=torch.uint8, device=DEV)
        self.rc = self.L.wbc_gait_targets(self.h, s, n, ld, _ptr(keep[0]), _ptr(tg), _ptr(mk))
        if ns is None:
            _lib.check(self.rc)
        _sync()
        return tg.cpu().numpy(), mk.cpu().numpy()

    def clear_schedule(self):
        _lib.check(self.L.wbc_gait_clear_schedule(self.h))


def _schedules(rng, blend):
    """LD instances, instance i with m = i mod 8 switches at its own seeded path parameters (gaps of blend + 0.3 .. 2.5) and commands;
    rows from m on hold NaN: they are not read."""
    m = (np.arange(LD) % 8).astype(np.uint8)
    when, cmds = np.full((7, LD), np.nan), np.full((21, LD), np.nan)
    th = rng.uniform(0.0, 2.0, LD)
    for j in range(7):
        used = j < m
        when[j, used] = th[used]
        c = np.stack([rng.uniform(-1.0, 1.0, LD), rng.uniform(-1.0, 1.0, LD), rng.uniform(-2.0, 2.0, LD)])
        c[2, (np.arange(LD) + j) % 5 == 0] = 0.0
        c[2, (np.arange(LD) + j) % 5 == 1] = 1.5e-5
        cmds[3 * j:3 * j + 3, used] = c[:, used]
        th = th + blend + rng.uniform(0.3, 2.5, LD)
    return m, when, cmds


@functools.lru_cache(maxsize=None)
def _case(ground, blend):
    """LD instances on the sixteen strides of test_gait_gpu (and, terrain, the sixteen profiles of follow_oracle, each at its own
    scale), every one with its own schedule: seeded times, drawn again where they lie within 1e-9 s of a boundary of the stride, where a
    pose evaluation lies within 1e-9 of a Theta_j or a window's end, or where a foothold lies within 1e-9 m of a decision of the
    terrain law (none is dropped).  Read-only."""
    rng = np.random.default_rng(53 + int(10 * blend) + (100 if ground == "terrain" else 0))
    P = hg.params(wait_time=0.25)
    S = [gait.stride(s) for s in SIXTEEN]
    gid = (np.arange(LD) * 7 % 16).astype(np.uint8)
    sc = rng.uniform(0.5, 2.0, LD)
    time = np.r_[rng.uniform(-0.05, 0.25, 3), rng.uniform(0.25, 20.25, LD - 3)]
    cmd = np.stack([rng.uniform(-1.0, 1.0, LD), rng.uniform(-1.0, 1.0, LD), rng.uniform(-2.0, 2.0, LD)])
    cmd[2, ::6] = 0.0
    st = np.stack([rng.uniform(-1, 1, LD), rng.uniform(-1, 1, LD), rng.uniform(-3, 3, LD)])
    m, when, cmds = _schedules(rng, blend)
    kw = {}
    if ground == "terrain":
        kw = dict(profiles=fo.sixteen_profiles(), terrain_id=(np.arange(LD) * 5 % 16).astype(np.uint8),
                  terrain_scale=np.array(fo.SCALES)[(np.arange(LD) // 3) % 4].copy(), tp=gto.tparams(body="fit", max_grade=tgt.MAX_GRADE))
    for _ in range(20):
        info = {}
        o80 = gso.targets(P, S, time, cmd, m, when, cmds, blend, gid, sc, st, dtype=np.longdouble, info=info, **kw)
        again = (info["near"] < NEAR) | (info["terrain_near"] < NEAR)
        for i in range(3, LD):
            again[i] |= float(go.boundary_distance(S[gid[i]][0], time[i:i + 1], P["wait_time"], sc[i:i + 1])[0]) < 1e-9
        if not again[3:].any():
            break
        time[3:][again[3:]] = rng.uniform(0.25, 20.25, int(again[3:].sum()))
    assert not again[3:].any()
    o64 = gso.targets(P, S, time, cmd, m, when, cmds, blend, gid, sc, st, **kw)
    for a in (gid, sc, time, cmd, st, m, when, cmds):
        a.setflags(write=False)
    return dict(P=P, S=S, gid=gid, sc=sc, time=time, cmd=cmd, st=st, m=m, when=when, cmds=cmds, kw=kw, o64=o64, o80=o80)


def _raw(c, strides=SIXTEEN):
    g = RawScheduleGait(strides, c["P"])
    if c["kw"]:
        g.set_terrain(c["kw"]["tp"], c["kw"]["profiles"], c["kw"]["terrain_id"], c["kw"]["terrain_scale"])
    return g


@pytest.mark.parametrize("ground", ["plane", "terrain"])
@pytest.mark.parametrize("n", [1, 5, 17, 67])
def test_schedule_kernels_match_the_host_twin(n, ground):
    """n = 1, 5 (a quad tail), 17 (a second quad group of a wavefront's tail), 67 (more than one block of 16 robots), ld = 80 > n; beta =
    0 and 0.5; every instance with its own m = 0 .. 7, switches, commands, stride, stride scale and (terrain) profile and terrain
    scale.  The bars are the CPU test's, over all LD instances: 100 x the double oracle's distance from the extended-precision one,
    per kind of row.  The schedule's arrays are overwritten before the targets are asked for."""
    for blend in (0.0, 0.5):
        c = _case(ground, blend)
        g = _raw(c)
        got, gmask = g.scheduled(n, LD, c["time"], c["cmd"], c["gid"], c["sc"], c["st"], blend, c["m"], c["when"], c["cmds"])
        assert g.rc == 0
        want, wmask = hgs.run(SIXTEEN, c["time"], c["cmd"], c["m"], c["when"], c["cmds"], blend, c["gid"], c["sc"], c["st"], p=c["P"], **c["kw"])
        (o64, m64), (o80, _) = c["o64"], c["o80"]
        assert (got[:, n:] == 7.5).all() and (gmask[n:] == 0x55).all()                           # the padding columns: untouched
        assert (gmask[:n] == wmask[:n]).all() and (wmask == m64).all() and np.isfinite(got[:, :n]).all()
        for group, rows in (tgc.GROUPS if ground == "plane" else tgt.GROUPS):
            bar = 100.0 * float(np.abs(o64[rows] - o80[rows]).max())
            worst = float(np.abs(got[rows, :n] - want[rows, :n]).max())
            print("GAIT-SCHEDULE device-to-twin n=%d %-7s beta %.1f %-14s worst %.3g bar %.3g" % (n, ground, blend, group, worst, bar))
            assert bar > 0 and worst < bar, (n, ground, blend, group, worst, bar)
        g.close()


def test_schedule_kernels_resources_and_a_batch_larger_than_the_schedule():
    """Both new kernels: 0 scratch, 64 threads, the plain kernels' tables in LDS.  wbc_gait_targets with a larger n than the
    schedule's is refused before any launch, and runs again once the schedule is cleared."""
    p = gait.GaitPlanner(MODEL, device=0)
    plane, terrain, old = p.schedule_kernel_info(), p.schedule_kernel_info(terrain=True), p.kernel_info()
    print("GAIT-SCHEDULE kernels", plane, terrain, "plain", old)
    for info, lds in ((plane, 8 * (12 + 16 * 204)), (terrain, 8 * (12 + 16 * 204 + 12 + 16 * 40))):
        assert info["scratch_bytes_per_lane"] == 0 and info["block_threads"] == 64 and info["lds_bytes"] == lds and 0 < info["num_regs"] <= 256
    assert old["lds_bytes"] == 8 * (12 + 16 * 204) and old["scratch_bytes_per_lane"] == 0
    p.close()
    c = _case("plane", 0.5)
    g = _raw(c)
    got, gmask = g.scheduled(9, LD, c["time"], c["cmd"], c["gid"], c["sc"], c["st"], 0.5, c["m"], c["when"], c["cmds"], ns=8)
    assert g.rc < 0 and "wbc_gait_set_schedule" in g.L.wbc_last_error().decode() and (got == 7.5).all() and (gmask == 0x55).all()
    g.clear_schedule()
    plain, _ = g.targets(9, LD, c["time"], c["cmd"], c["gid"], c["sc"], c["st"])
    assert np.isfinite(plain[:, :9]).all()
    g.close()


@pytest.mark.parametrize("ground", ["plane", "terrain"])
def test_no_switch_and_a_cleared_schedule_give_the_plain_kernels_bits(ground):
    """The instances with m = 0 inside a scheduled batch, a whole batch with m = 0, an instance whose one switch lies far ahead, and a
    handle after wbc_gait_clear_schedule: the bits of the kernel a handle without a schedule launches; the instances with switches
    behind them get another answer."""
    c = _case(ground, 0.5)
    n = 67
    fresh = _raw(c)
    plain, pmask = fresh.targets(n, LD, c["time"], c["cmd"], c["gid"], c["sc"], c["st"])
    fresh.close()
    g = _raw(c)
    got, gmask = g.scheduled(n, LD, c["time"], c["cmd"], c["gid"], c["sc"], c["st"], 0.5, c["m"], c["when"], c["cmds"])
    none = c["m"][:n] == 0
    moved = (c["m"][:n] > 0) & (c["time"][:n] - 0.5 > c["when"][0, :n] + 3.0)
    assert none.sum() >= 8 and moved.sum() >= 8
    assert pe.same_bits(got[:, :n][:, none], plain[:, :n][:, none]) and (gmask[:n] == pmask[:n]).all()
    assert (np.abs(got[0:2, :n][:, moved] - plain[0:2, :n][:, moved]).max(0) > 1e-6).all()
    zero, zmask = g.scheduled(n, LD, c["time"], c["cmd"], c["gid"], c["sc"], c["st"], 0.5, np.zeros(LD, np.uint8), c["when"], c["cmds"])
    assert pe.same_bits(zero, plain) and (zmask == pmask).all()
    far = np.nan_to_num(c["when"], nan=0.0)
    far[0] = 40.0                                              # every pose evaluation of 20 s of samples lies before it
    ahead, _ = g.scheduled(n, LD, c["time"], c["cmd"], c["gid"], c["sc"], c["st"], 0.5, np.ones(LD, np.uint8), far, np.nan_to_num(c["cmds"], nan=0.1))
    assert pe.same_bits(ahead, plain)
    g.clear_schedule()
    off, omask = g.targets(n, LD, c["time"], c["cmd"], c["gid"], c["sc"], c["st"])
    assert pe.same_bits(off, plain) and (omask == pmask).all()
    g.close()


INVALID = [("m", 8), ("m", 255), ("when0", -1e-3), ("when0", math.nan), ("when2", math.inf), ("order", None), ("tight", None), ("cmd", math.nan)]


@pytest.mark.parametrize("ground", ["plane", "terrain"])
def test_invalid_schedules_in_every_slot_of_a_wavefront(ground):
    """8 ways for a schedule to be invalid x the 16 robot slots of a wavefront, one invalid robot per wavefront: NaN rows and mask 0xF
    for it, and every other robot the bits it has in the batch without it."""
    names = ["trot", "walk", "pace"]
    n = len(INVALID) * 16 * 16
    rng = np.random.default_rng(17)
    time = rng.uniform(0.0, 12.0, n)
    cmd = np.stack([rng.uniform(-1, 1, n), rng.uniform(-0.5, 0.5, n), rng.uniform(-2, 2, n)])
    gid = (np.arange(n) % 3).astype(np.uint8)
    sc = rng.uniform(0.5, 2.0, n)
    m = np.full(n, 3, np.uint8)
    when = np.zeros((7, n))
    when[0], when[1], when[2] = rng.uniform(0.0, 2.0, n), rng.uniform(2.5, 4.0, n), rng.uniform(4.5, 8.0, n)
    cmds = np.zeros((21, n))
    cmds[0:9] = rng.uniform(-1, 1, (9, n))
    dm, dw, dc = m.copy(), when.copy(), cmds.copy()
    bad = np.zeros(n, bool)
    for k, (case, value) in enumerate(INVALID):
        for slot in range(16):
            i = (k * 16 + slot) * 16 + slot
            bad[i] = True
            if case == "m":
                dm[i] = value
            elif case.startswith("when"):
                dw[int(case[-1]), i] = value
            elif case == "order":
                dw[1, i], dw[2, i] = dw[2, i], dw[1, i]
            elif case == "tight":
                dw[2, i] = dw[1, i] + 0.5 - 1e-9
            else:
                dc[4, i] = value
    P = hg.params()
    g = RawScheduleGait(names, P)
    kw = {}
    if ground == "terrain":
        profiles = fo.sixteen_profiles()[:5]
        tid = (np.arange(n) % 5).astype(np.uint8)
        kw = dict(profiles=profiles, terrain_id=tid, tp=gto.tparams(max_grade=tgt.MAX_GRADE))
        g.set_terrain(kw["tp"], profiles, tid)
    ct, cm = g.scheduled(n, n, time, cmd, gid, sc, None, 0.5, m, when, cmds)
    dt_, dmk = g.scheduled(n, n, time, cmd, gid, sc, None, 0.5, dm, dw, dc)
    assert np.isfinite(ct).all()
    assert np.isnan(dt_[:, bad]).all() and (dmk[bad] == 0xF).all()
    assert pe.same_bits(dt_[:, ~bad], ct[:, ~bad]) and (dmk[~bad] == cm[~bad]).all()
    twin, tmask = hgs.run(names, time, cmd, dm, dw, dc, 0.5, gid, sc, None, p=P, **kw)
    assert np.array_equal(np.isnan(twin), np.isnan(dt_)) and (tmask == dmk).all()
    g.close()


# ---- a scheduled gait as the target source of the rollout, and the closed loop
def _planner(cases, scale=0.5, blend=BLEND, profiles=None):
    """a GaitPlanner for len(cases) robots, robot i walking cases[i] = (c_0, times, commands); profiles: robot i's terrain (FIT)"""
    n = len(cases)
    p = gait.GaitPlanner(MODEL, strides=("trot",), device=0)
    p.set_commands(_t(np.array([c[0] for c in cases]).T.copy()), stride_scale=_t(np.full(n, scale)))
    mm = max(len(c[1]) for c in cases)
    times, cmds = np.full((mm, n), np.inf), np.zeros((mm, 3, n))
    for i, (_, ts, cs) in enumerate(cases):
        times[:len(ts), i] = ts
        cmds[:len(ts), :, i] = np.array(cs, dtype=np.float64).reshape(-1, 3)
    p.set_schedule(times, cmds, blend=blend)
    if profiles is not None:
        p.set_terrain(profiles, terrain_id=_t(np.arange(n, dtype=np.uint8)), body="fit")
    return p


def test_ground_rollout_with_a_scheduled_gait_equals_the_launches_made_by_hand():
    """200 ticks of wbc_ground_rollout, through the switches at 0.5 s, their blends and a second switch, with a scheduled gait set
    against wbc_gait_targets (the schedule kernel) -> wbc_step -> wbc_ground_step issued one by one: bit-identical; and another answer
    than the same planner's after clear_schedule()."""
    from quadruped_drake_amd import GroundContactPlant, IDController, closed_loop
    cases = [((0.2, 0.0, 0.0), [0.5], [(0.4, 0.0, 0.5)]), ((0.2, 0.0, 0.0), [0.5], [(-0.2, 0.0, 0.0)]),
             ((0.2, 0.0, 0.0), [0.5, 1.1], [(0.4, 0.0, 0.5), (0.0, 0.0, 0.0)]), ((0.1, 0.1, -0.5), [0.55], [(0.0, 0.0, 0.0)]), ((0.0, 0.0, 0.0), [], [])]
    n, steps, dt, t0 = len(cases), 200, 5e-3, 0.0
    q0, v0 = workloads.nominal_state(MODEL, n)
    plant = GroundContactPlant(MODEL, device=0)
    planner = _planner(cases)
    assert planner.has_schedule

    def rollout():
        ctrl = IDController(max_batch=n, device=0)
        q, v, tm = _t(q0), _t(v0), _t(np.full(n, t0))
        out = closed_loop(ctrl, plant, planner, steps, dt, q, v, tm)
        _sync()
        res = [x.cpu().numpy() for x in (q, v, out[0], out[6], out[3], out[4])]
        ctrl.close()
        return res

    got = rollout()
    ctrl = IDController(max_batch=n, device=0)
    q, v, tm = _t(q0), _t(v0), _t(np.full(n, t0))
    for _ in range(steps):
        tg, mk = planner.targets(tm)
        tau, met, st = ctrl.step(q, v, tg, mk)
        f, ct, fl = plant.step(q, v, tau, dt, time=tm)
    _sync()
    for a, b, name in zip(got, (q, v, tau, fl, tg, mk), NAMES):
        assert pe.same_bits(a, b.cpu().numpy()), name
    ctrl.close()
    planner.clear_schedule()
    assert not planner.has_schedule
    flat = rollout()
    assert not pe.same_bits(flat[4][:, :4], got[4][:, :4]) and pe.same_bits(flat[4][:, 4], got[4][:, 4])      # robot 4 has no switch
    plant.close(); planner.close()


@functools.lru_cache(maxsize=None)
def _device_walks():
    """The three closed loops of tests/test_gait_schedule_cpu.py in one batch on the device, and each on the host twins: Mini Cheetah,
    ID, dt 5 ms, trot at stride scale 0.5, 800 ticks on the compliant ground, beta = 0.5 -- turn, slow and stop; reverse; and the first
    over the kerb ramp_step(0.3, 0.10) -- the terrain gait in FIT on all three, the first two on flat(0).  -> dict(fell, bad: ticks per
    robot, ticks, status_nonzero, q: the final states, plan: the device's final targets, host: host_walk's answers on the rollout's
    clock)"""
    import torch
    from quadruped_drake_amd import GroundContactPlant, IDController, closed_loop
    makes = [lambda: tr.flat(0.0), lambda: tr.flat(0.0), lambda: tr.ramp_step(0.3, 0.10)]
    cases = [TURN, REVERSE, TURN]
    n, ticks, dt = 3, 800, 5e-3
    profiles = [f() for f in makes]
    q0, v0 = workloads.nominal_state(MODEL, n)
    plant = GroundContactPlant(MODEL, device=0)
    plant.set_terrain(profiles, terrain_id=_t(np.arange(n, dtype=np.uint8)))
    planner = _planner(cases, profiles=profiles)
    ctrl = IDController(max_batch=n, device=0)
    ctrl.stats(reset=True)
    q, v, tm = _t(q0), _t(v0), _t(np.zeros(n))
    counts = torch.zeros((4, n), dtype=torch.int32, device=DEV)
    closed_loop(ctrl, plant, planner, ticks, dt, q, v, tm, counts=counts)
    _sync()
    s = ctrl.stats()
    cn, qf = counts.cpu().numpy(), q.cpu().numpy()
    plan = planner.targets(tm)[0].cpu().numpy()
    _sync()
    plant.close(); planner.close(); ctrl.close()
    host = [host_walk((cases[i], makes[i]), accumulate=True) for i in range(n)]          # on the rollout's clock: time += dt
    for i, r in enumerate(host):
        print("GAIT-SCHEDULE device walk %d: device (%.5f, %.5f, %.5f) host (%.5f, %.5f, %.5f) plan (%.5f, %.5f)" %
              (i, qf[4, i], qf[5, i], qf[6, i], r["x"], r["y"], r["z"], r["plan"][0], r["plan"][1]))
    return dict(fell=cn[1], bad=cn[3], ticks=s["ticks"], status_nonzero=s["status_nonzero"], q=qf, plan=plan, host=host, n=n, want_ticks=n * ticks)


def test_id_turns_stops_and_reverses_on_the_device():
    """_device_walks(): no FELL, no BAD, status 0 on every tick, every final trunk within 0.03 m of its plan in x-y (the bar of
    tests/test_gait_cpu.py), and the device's plan is the oracle's.  Measured off the plan: 3.6 mm, 5.4 mm and 4.3 mm."""
    w = _device_walks()
    assert (w["fell"] == 0).all() and (w["bad"] == 0).all() and w["ticks"] == w["want_ticks"] and w["status_nonzero"] == 0
    for i, r in enumerate(w["host"]):
        off = math.hypot(w["q"][4, i] - r["plan"][0], w["q"][5, i] - r["plan"][1])
        print("GAIT-SCHEDULE device walk %d: off the plan %.5f" % (i, off))
        assert np.abs(w["plan"][0:3, i] - r["plan"]).max() < 1e-9 and not r["flags"] & 10 and r["status"] == 0
        assert off < 0.03


def test_the_device_walks_end_within_a_tenth_of_a_millimetre_of_the_host_twins():
    """_device_walks(): every final pose within 0.1 mm of the host twins' run of the same case, the figure profiles/r14/gait_terrain.md
    records for such loops.  The host twins run on the rollout's clock, which adds dt to the time tick by tick.  Measured: 7.0e-14 m
    (turn, slow, stop), 8.1e-14 m (reverse) and 1.4e-13 m (the turn over the kerb), the plant's flags equal on every tick.  With the
    host twins asked at k dt instead the runs are 1.5e-11 m apart until tick 230 -- 1.15 s, a boundary of the trot at scale 0.5, which
    k dt reaches and the summed clock does not -- have another contact mask for that tick, and end 0.34, 0.76 and 0.35 mm apart
    (profiles/r15/gait_schedule.md)."""
    w = _device_walks()
    apart = [float(np.linalg.norm([w["q"][4, i] - r["x"], w["q"][5, i] - r["y"], w["q"][6, i] - r["z"]])) for i, r in enumerate(w["host"])]
    print("GAIT-SCHEDULE device walks apart from the host twins' [m]:", apart)
    assert max(apart) < 1e-4, apart


def test_simulate_cmd_schedule_is_wired_and_reported(capsys):
    """python -m quadruped_drake_amd.simulate --planner gait --cmd-schedule: the JSON line names the schedule, and 4 robots turn, slow
    and stop over 4 s without FELL or BAD, within 0.03 m of their plan."""
    import json
    from quadruped_drake_amd import simulate
    rc = simulate.main(["--control", "ID", "--n", "4", "--sim-time", "4.0", "--dt", "5e-3", "--log-every", "200", "--planner", "gait", "--cmd", "0.2,0,0",
                        "--plant", "ground", "--cmd-schedule", "1.5:0.4,0,0.5;2.5:0.2,0,0;3.2:0,0,0"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rc == 0 and line["cmd_schedule"] == [[1.5, 0.4, 0.0, 0.5], [2.5, 0.2, 0.0, 0.0], [3.2, 0.0, 0.0, 0.0]] and line["cmd_blend"] == 0.5
    assert line["FELL"] == 0 and line["plant_flags"]["bad"] == 0 and line["plan_offset_worst"] < 0.03
