"""The gait planner on the MI355X (include/wbc_gait.h; gait.GaitPlanner): wbc_gait_targets_kernel against the host instantiation
of the same header (tests/host_gait.py) at the bars of tests/test_gait_cpu.py, malformed instances in every robot slot of a
wavefront, its resources, the gait as the target source of wbc_ground_rollout and wbc_plant_rollout against the same launches issued
by hand, and ID walking five commands at once on the compliant ground."""
import ctypes as C
import functools

import numpy as np
import pytest

import gait_oracle as go
import host_gait as hg
import plant_edges as pe
from quadruped_drake_amd import _lib, gait, workloads
from test_gait_cpu import DYADIC, GROUPS, MALFORMED, malformed_batch, spoil

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODEL = "mini_cheetah"
LD = 80
# sixteen strides: the reference's ten and six more (a dyadic trot, three feet always down, a one-phase-per-foot crawl, ...)
SIXTEEN = list(gait.STRIDES) + [DYADIC, ((0.2, 0.3), (0b1111, 0b1110)), ((0.15, 0.1, 0.15, 0.1, 0.15, 0.1, 0.15, 0.1), (14, 15, 13, 15, 11, 15, 7, 15)),
                                ((0.4, 0.4), (0b0101, 0b1010)), ((0.11, 0.07, 0.13), (0b1001, 0b0000, 0b0110)),
                                ((0.05, 0.5, 0.05, 0.5), (0b0011, 0b1111, 0b1100, 0b1111))]


def _t(a, dtype=None):
    import torch
    return torch.tensor(np.ascontiguousarray(a), device=DEV, dtype=dtype)


def _sync():
    import torch
    torch.cuda.synchronize()


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class RawGait:
    """A wbc_gait handle through the C ABI, with arrays of any leading dimension"""

    def __init__(self, strides, P):
        self.L = _lib.lib()
        self.h = C.c_void_p()
        cp = gait.c_params(P["stance"], P["height"], P["swing_height"], P["ramp_time"], P["wait_time"])
        _lib.check(self.L.wbc_gait_create(C.byref(cp), gait.c_strides(strides), len(strides), 0, C.byref(self.h)))

    def targets(self, n, ld, time, cmd, gid=None, sc=None, st=None, fill=7.5):
        """-> (targets [54, ld], mask [ld]) with the padding columns preset to `fill` / 0x55"""
        import torch
        keep = [_t(time), _t(cmd), None if gid is None else _t(gid), None if sc is None else _t(sc), None if st is None else _t(st)]
        _lib.check(self.L.wbc_gait_set_commands(self.h, *[_ptr(a) for a in keep[1:]]))
        tg = torch.full((54, ld), fill, dtype=torch.float64, device=DEV)
        mk = torch.full((ld,), 0x55, dtype=torch.uint8, device=DEV)
        s = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
        _lib.check(self.L.wbc_gait_targets(self.h, s, n, ld, _ptr(keep[0]), _ptr(tg), _ptr(mk)))
        _sync()
        return tg.cpu().numpy(), mk.cpu().numpy()

    def close(self):
        self.L.wbc_gait_destroy(self.h)


@functools.lru_cache(maxsize=None)
def _case():
    """LD instances: seeded times over -0.3 .. 20 s after the wait, each verified to lie 1e-9 s off every boundary of its stride
    (a time that does not is drawn again, none is dropped), commands, scales and starts as the CPU test draws them.  Read-only."""
    rng = np.random.default_rng(31)
    P = hg.params(wait_time=0.25)
    S = [gait.stride(s) for s in SIXTEEN]
    gid = (np.arange(LD) * 7 % 16).astype(np.uint8)
    sc = rng.uniform(0.5, 2.0, LD)
    time = np.r_[rng.uniform(-0.05, 0.25, 3), rng.uniform(0.25, 20.25, LD - 3)]
    for i in range(LD):
        while i >= 3 and float(go.boundary_distance(S[gid[i]][0], time[i:i + 1], P["wait_time"], sc[i:i + 1])[0]) < 1e-9:
            time[i] = rng.uniform(0.25, 20.25)
    cmd = np.stack([rng.uniform(-1.0, 1.0, LD), rng.uniform(-1.0, 1.0, LD), rng.uniform(-2.0, 2.0, LD)])
    cmd[2, ::6] = 0.0
    cmd[2, 1::6] = 1.5e-5                                   # |omega theta / 2| on either side of 1e-4 within 20 s
    st = np.stack([rng.uniform(-1, 1, LD), rng.uniform(-1, 1, LD), rng.uniform(-3, 3, LD)])
    for a in (gid, sc, time, cmd, st):
        a.setflags(write=False)
    return dict(P=P, S=S, gid=gid, sc=sc, time=time, cmd=cmd, st=st)


@pytest.mark.parametrize("n", [1, 5, 17, 67])
def test_gait_kernel_matches_the_host_twin(n):
    """n = 1, 5 (a quad tail), 17 (a second quad group of a wavefront's tail), 67 (more than one block of 16 robots), ld = 80 > n."""
    c = _case()
    g = RawGait(SIXTEEN, c["P"])
    if n >= 16:
        assert sorted(set(c["gid"][:n])) == list(range(16))
    for full in (True, False):
        gid, sc, st = (c["gid"], c["sc"], c["st"]) if full else (None, None, None)
        got, gmask = g.targets(n, LD, c["time"], c["cmd"], gid, sc, st)
        want, wmask = hg.run(SIXTEEN, c["time"], c["cmd"], gid, sc, st, p=c["P"])
        o64, m64 = go.targets(c["P"], c["S"], c["time"], c["cmd"], gid, sc, st)
        o80, _ = go.targets(c["P"], c["S"], c["time"], c["cmd"], gid, sc, st, dtype=np.longdouble)
        assert (got[:, n:] == 7.5).all() and (gmask[n:] == 0x55).all()                       # the padding columns: untouched
        assert (gmask[:n] == wmask[:n]).all() and (wmask == m64).all() and np.isfinite(got[:, :n]).all()
        for group, rows in GROUPS:
            bar = 100.0 * float(np.abs(o64[rows] - o80[rows]).max())                        # over all LD instances: one bar for every n
            worst = float(np.abs(got[rows, :n] - want[rows, :n]).max())
            print("GAIT device-to-twin n=%d %s %-13s worst %.3g bar %.3g" % (n, "all arrays" if full else "defaults  ", group, worst, bar))
            assert worst < bar, (n, full, group, worst, bar)
    g.close()


def test_malformed_instances_in_every_slot_of_a_wavefront():
    """13 ways to be malformed x the 16 robot slots of a wavefront, one malformed robot per wavefront: it gets NaN rows and mask 0xF,
    and every other robot the bits it has in the batch without it."""
    names = ["trot", "walk", "pace"]
    n = len(MALFORMED) * 16 * 16
    clean = malformed_batch(n, len(names), seed=6)
    dirty = [a.copy() for a in clean]
    bad = np.zeros(n, bool)
    for k, (case, value) in enumerate(MALFORMED):
        for slot in range(16):
            i = (k * 16 + slot) * 16 + slot
            spoil(case, value, i, len(names), *dirty)
            bad[i] = True
    P = hg.params()
    g = RawGait(names, P)
    ct, cm = g.targets(n, n, *clean)
    dt_, dm = g.targets(n, n, *dirty)
    assert np.isfinite(ct).all()
    assert np.isnan(dt_[:, bad]).all() and (dm[bad] == 0xF).all()
    assert pe.same_bits(dt_[:, ~bad], ct[:, ~bad]) and (dm[~bad] == cm[~bad]).all()
    twin, tmask = hg.run(names, *dirty, p=P)
    assert np.array_equal(np.isnan(twin), np.isnan(dt_)) and (tmask == dm).all()
    g.close()


def test_gait_kernel_resources():
    p = gait.GaitPlanner(MODEL, device=0)
    info = p.kernel_info()
    print("GAIT kernel", info)
    assert info["scratch_bytes_per_lane"] == 0 and info["block_threads"] == 64
    assert info["lds_bytes"] == 8 * (12 + 16 * 204)                 # the packed table: csrc/wbc_gait.hpp
    assert 0 < info["num_regs"] <= 128
    import torch
    with pytest.raises(ValueError):
        p.targets(torch.zeros(4, dtype=torch.float64, device=DEV))  # before set_commands
    p.close()


# ---- the gait as the target source of the rollouts
COMMANDS5 = np.array([(0.2, 0.0, 0.0), (-0.2, 0.0, 0.0), (0.4, 0.0, 0.5), (0.0, 0.0, 0.0), (0.1, 0.1, -0.5)]).T.copy()


def _planner(n=5):
    p = gait.GaitPlanner(MODEL, strides=("trot",), device=0)
    p.set_commands(_t(COMMANDS5[:, :n]), stride_scale=_t(np.full(n, 0.5)))
    return p


def _standing_traj():
    from quadruped_drake_amd.trajectory import TrunkTrajectory
    return TrunkTrajectory(np.zeros(0), np.zeros((0, 54)), np.zeros(0, np.uint8), model=MODEL, wait_time=1e9, device=0,
                           standing_targets=workloads.standing_targets(MODEL, 1)[:, 0], standing_mask=0b1111)


def _loop(plant, traj, steps, dt, q0, v0):
    """closed_loop with a fresh ID controller -> q, v, and the last tick's tau, flags, targets and mask"""
    from quadruped_drake_amd import IDController, closed_loop
    ctrl = IDController(max_batch=q0.shape[1], device=0)
    q, v, tm = _t(q0), _t(v0), _t(np.zeros(q0.shape[1]))
    out = closed_loop(ctrl, plant, traj, steps, dt, q, v, tm)
    _sync()
    res = [x.cpu().numpy() for x in (q, v, out[0], out[6], out[3], out[4])]
    ctrl.close()
    return res


NAMES = ("q", "v", "tau", "flags", "targets", "mask")


@pytest.mark.parametrize("ground", ["slope_fit", "plane"])
def test_ground_rollout_with_a_gait_equals_the_launches_made_by_hand(ground):
    """20 ticks of wbc_ground_rollout with a gait set -- on a slope of grade 0.2 with FIT, and on the plane with no terrain -- against
    wbc_gait_targets -> wbc_ground_follow_targets (on the slope) -> wbc_step -> wbc_ground_step issued one by one: bit-identical.  Then
    the trajectory again."""
    import terrain_oracle as to
    from quadruped_drake_amd import GroundContactPlant, IDController
    n, steps, dt = 5, 20, 5e-3
    slope = ground == "slope_fit"
    if slope:
        _, q0, v0, prof = to.slope_stance(MODEL, 0.2, n=n)
    else:
        q0, v0 = workloads.nominal_state(MODEL, n)
    plant = GroundContactPlant(MODEL, device=0)
    traj = _standing_traj()
    before = _loop(plant, traj, steps, dt, q0, v0)              # a plant that never saw a gait
    if slope:
        plant.set_terrain([prof])
        plant.set_follow("fit")
    planner = _planner(n)
    got = _loop(plant, planner, steps, dt, q0, v0)
    ctrl = IDController(max_batch=n, device=0)
    q, v, tm = _t(q0), _t(v0), _t(np.zeros(n))
    for _ in range(steps):
        tg, mk = planner.targets(tm)
        if slope:
            plant.follow_targets(tg, "fit")
        tau, met, st = ctrl.step(q, v, tg, mk)
        f, ct, fl = plant.step(q, v, tau, dt, time=tm)
    _sync()
    for a, b, name in zip(got, (q, v, tau, fl, tg, mk), NAMES):
        assert pe.same_bits(a, b.cpu().numpy()), name
    assert np.allclose(tm.cpu().numpy(), steps * dt) and len(set(got[0][4])) == n          # five commands, five places
    ctrl.close()
    # the gait taken off again: the rollout has its trajectory back
    plant.set_terrain(None)
    plant.set_follow("off")
    _lib.check(plant._L.wbc_ground_set_gait(plant._h, planner._h))
    _lib.check(plant._L.wbc_ground_set_gait(plant._h, None))
    for a, b, name in zip(before, _loop(plant, traj, steps, dt, q0, v0), NAMES):
        assert pe.same_bits(a, b), name
    assert not pe.same_bits(before[0], got[0])
    with pytest.raises(ValueError):
        _loop(plant, planner, steps, dt, q0[:, :3], v0[:, :3])                               # commands for 5, a batch of 3
    plant.close(); planner.close(); traj.close()


def test_set_gait_refuses_a_gait_of_another_device():
    """A gait handle is host work until its first set_commands, so one for device 1 exists on any machine: both plants' setters
    refuse it as misuse, keep what they had, and take one of their own device."""
    from quadruped_drake_amd import GroundContactPlant, RigidContactPlant
    L = _lib.lib()
    P = hg.params()
    cp = gait.c_params(P["stance"], P["height"], P["swing_height"], P["ramp_time"], P["wait_time"])
    far, near = C.c_void_p(), C.c_void_p()
    _lib.check(L.wbc_gait_create(C.byref(cp), gait.c_strides(["trot"]), 1, 1, C.byref(far)))
    _lib.check(L.wbc_gait_create(C.byref(cp), gait.c_strides(["trot"]), 1, 0, C.byref(near)))
    for plant, fn in ((GroundContactPlant(MODEL, device=0), L.wbc_ground_set_gait), (RigidContactPlant(MODEL, device=0), L.wbc_plant_set_gait)):
        assert fn(plant._h, far) < 0 and "another device" in L.wbc_last_error().decode()
        assert fn(plant._h, near) == 0 and fn(plant._h, far) < 0 and fn(plant._h, None) == 0
        plant.close()
    L.wbc_gait_destroy(far); L.wbc_gait_destroy(near)


def test_plant_rollout_with_a_gait_equals_the_launches_made_by_hand():
    from quadruped_drake_amd import IDController, RigidContactPlant
    n, steps, dt = 5, 20, 5e-3
    q0, v0 = workloads.nominal_state(MODEL, n)
    plant = RigidContactPlant(MODEL, device=0)
    traj = _standing_traj()
    before = _loop(plant, traj, steps, dt, q0, v0)
    planner = _planner(n)
    got = _loop(plant, planner, steps, dt, q0, v0)
    ctrl = IDController(max_batch=n, device=0)
    q, v, tm = _t(q0), _t(v0), _t(np.zeros(n))
    for _ in range(steps):
        tg, mk = planner.targets(tm)
        tau, met, st = ctrl.step(q, v, tg, mk)
        vd, f, fl = plant.step(q, v, tau, mk, dt, time=tm)
    _sync()
    for a, b, name in zip(got, (q, v, tau, fl, tg, mk), NAMES):
        assert pe.same_bits(a, b.cpu().numpy()), name
    ctrl.close()
    for a, b, name in zip(before, _loop(plant, traj, steps, dt, q0, v0), NAMES):
        assert pe.same_bits(a, b), name
    assert not pe.same_bits(before[0], got[0])
    plant.close(); planner.close(); traj.close()


def test_id_walks_five_commands_on_the_device():
    """The flat scenario of tests/test_gait_cpu.py on the device: Mini Cheetah, ID, dt 5 ms, trot at stride scale 0.5, 600 ticks in
    one closed_loop, five robots with five commands (the three of the CPU test, stepping in place, and a diagonal arc).  No FELL, no
    BAD, status 0 on every tick, every trunk within 0.03 m of its planned position and within 5 mm of 0.3 m above the ground."""
    import torch
    from quadruped_drake_amd import GroundContactPlant, IDController, closed_loop
    n, ticks, dt = 5, 600, 5e-3
    q0, v0 = workloads.nominal_state(MODEL, n)
    plant = GroundContactPlant(MODEL, device=0)
    planner = _planner(n)
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
    want = go.targets(hg.params(MODEL), [gait.stride("trot")], np.full(n, ticks * dt), COMMANDS5, None, np.full(n, 0.5))[0]
    off = np.hypot(qf[4] - want[0], qf[5] - want[1])
    print("GAIT device walk: x", qf[4], "y", qf[5], "off", off, "height", qf[6], "slip ticks", cn[0])
    assert np.abs(plan[0:2] - want[0:2]).max() < 1e-9 and np.allclose(tm.cpu().numpy(), ticks * dt)
    assert (cn[1] == 0).all() and (cn[3] == 0).all() and s["ticks"] == n * ticks and s["status_nonzero"] == 0
    assert (off < 0.03).all() and (np.abs(qf[6] - 0.3) < 5e-3).all()
    plant.close(); planner.close(); ctrl.close()


def test_simulate_gait_is_wired_and_reported(capsys):
    """python -m quadruped_drake_amd.simulate --planner gait on both plants: the JSON line names the gait and the command, and on the
    ground plant the distance from the plan; 40 ticks of ID end without FELL or BAD."""
    import json
    from quadruped_drake_amd import simulate
    common = ["--control", "ID", "--n", "4", "--sim-time", "0.2", "--dt", "5e-3", "--log-every", "20", "--planner", "gait", "--cmd", "0.2,0,0.3",
              "--cmd-spread", "0.1,0.05,0.2"]
    rc = simulate.main(common + ["--plant", "ground", "--terrain", "slope:0.1", "--follow", "fit"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rc == 0 and line["planner"] == "gait" and line["gait"] == "trot" and line["stride_scale"] == 0.5 and line["cmd"] == [0.2, 0.0, 0.3]
    assert line["FELL"] == 0 and line["plant_flags"]["bad"] == 0 and 0 <= line["plan_offset_mean"] <= line["plan_offset_worst"] < 0.03
    rc = simulate.main(common + ["--plant", "rigid", "--gait", "walk"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rc == 0 and line["gait"] == "walk" and line["plant_flags"]["bad"] == 0
