"""Targets that follow the terrain on the MI355X (include/wbc_ground.h, "Following the ground"; GroundContactPlant.follow_targets /
set_follow): wbc_ground_follow_kernel against the host instantiation of the same template (tests/host_follow.py) at the bar of
tests/test_follow_cpu.py, what it must leave alone, its resources, the wiring of the follow step into wbc_ground_rollout, and ID
standing on four slopes at once with followed targets."""
import ctypes as C
import functools

import numpy as np
import pytest

import follow_oracle as fo
import host_follow as hf
import plant_edges as pe
import terrain_oracle as to
from quadruped_drake_amd import workloads
from test_follow_cpu import BAR, worst

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODEL = "mini_cheetah"
BLOCK = 64                      # threads, and robots, per block of the follow kernel


def _t(a, dtype=None):
    import torch
    return torch.tensor(np.ascontiguousarray(a), device=DEV, dtype=dtype)


def _sync():
    import torch
    torch.cuda.synchronize()


def _marked(n):
    """-> (instances with a dead foot, instances with a bad terrain choice): the first and the last slot of every block of 64, in
    turn -- block 0: dead foot first, bad choice last; block 1 the other way round; and so on -- and below one block the last
    instance is a bad choice."""
    dead, bad = [], []
    for blk in range((n + BLOCK - 1) // BLOCK):
        first, last = blk * BLOCK, blk * BLOCK + BLOCK - 1
        (dead if blk % 2 == 0 else bad).append(first)
        if last < n:
            (bad if blk % 2 == 0 else dead).append(last)
    if 1 < n < BLOCK:
        bad.append(n - 1)
    return dead, bad


@functools.lru_cache(maxsize=None)
def _case(n):
    """The sixteen-profile batch of tests/test_follow_cpu.py cut to n instances, with what must be left alone in the slots of
    _marked: feet without a finite target (foot 1, 2, ... in turn), and terrain_id beyond the table or a NaN terrain_scale in turn.
    Read-only."""
    first = 6 if n < 8 else 0            # the smallest batches start on the eight-knot profile, at scales -0.7, 2.5, 1
    profiles, tid, tsc, t = fo.draw(max(n, 8) + first, 21)
    tid, tsc, t = tid[first:first + n].copy(), tsc[first:first + n].copy(), np.ascontiguousarray(t[:, first:first + n])
    dead_foot, bad = _marked(n)
    feet = [(k + 1) % 4 for k in range(len(dead_foot))]
    for c, i in zip(feet, dead_foot):
        t[18 + 9 * c:27 + 9 * c, i] = np.nan
    for k, i in enumerate(bad):
        if k % 2 == 0:
            tid[i] = 16 if k % 4 == 0 else 255
        else:
            tsc[i] = np.nan
    for a in (tid, tsc, t):
        a.setflags(write=False)
    return dict(profiles=profiles, tid=tid, tsc=tsc, t=t, dead_foot=list(zip(feet, dead_foot)), bad=bad)


def _plant(c, model=MODEL):
    from quadruped_drake_amd import GroundContactPlant
    plant = GroundContactPlant(model, device=0)
    plant.set_terrain(c["profiles"], _t(c["tid"]), _t(c["tsc"]))
    return plant


def _follow_wide(plant, t, n, ld, mode):
    """wbc_ground_follow_targets through the C ABI on targets of ld >= n columns, the padding NaN -> the whole [54, ld] array"""
    from quadruped_drake_amd import _lib
    tg = _t(pe.wide(t, ld, np.nan))
    _lib.check(plant._L.wbc_ground_follow_targets(plant._h, plant._stream(), n, ld, mode, C.c_void_p(tg.data_ptr())))
    _sync()
    return tg.cpu().numpy()


@pytest.mark.parametrize("n", [1, 3, 64, 65, 257])
def test_follow_kernel_matches_the_host_twin(n):
    c = _case(n)
    ld = n + 3
    plant = _plant(c)
    for name, mode in (("lift", fo.LIFT), ("fit", fo.FIT)):
        got = _follow_wide(plant, c["t"], n, ld, mode)
        want = hf.run(c["profiles"], c["t"], name, c["tid"], c["tsc"])
        assert pe.padding_kept(got, n, np.nan), name
        got = got[:, :n]
        fin = np.isfinite(want)
        assert np.array_equal(np.isfinite(got), fin), name
        w = worst(got[fin], want[fin])
        print("FOLLOW device-to-twin n=%d %s worst %.3g" % (n, name, w))
        assert w < BAR, name
        # every row the mode does not write, every row of an instance it must leave alone, every row of a dead foot: the input's bits
        written = np.zeros((54, n), bool)
        written[fo.ZROWS + (fo.ATTITUDE if mode == fo.FIT else [])] = True
        written[:, c["bad"]] = False
        for foot, i in c["dead_foot"]:
            written[18 + 9 * foot:27 + 9 * foot, i] = False
        assert pe.same_bits(got[~written], c["t"][~written]), name
        assert pe.same_bits(want[~written], c["t"][~written]), name
        if n >= 64:
            # and it wrote what it should (a quarter of the batch stands on scale 0, and level pieces move no velocity row)
            assert (pe.bits(got) != pe.bits(c["t"]))[written].mean() > 0.3
    plant.close()


def test_follow_kernel_resources():
    from quadruped_drake_amd import GroundContactPlant
    plant = GroundContactPlant(MODEL, device=0)
    info = plant.follow_kernel_info()
    print("FOLLOW kernel", info)
    assert info["scratch_bytes_per_lane"] == 0 and info["lds_bytes"] == 0 and info["block_threads"] == BLOCK
    assert 0 < info["num_regs"] <= 256
    plant.close()


def test_off_and_no_terrain_leave_the_targets_alone():
    from quadruped_drake_amd import GroundContactPlant
    n = 65
    c = _case(n)
    plant = _plant(c)
    assert pe.same_bits(_follow_wide(plant, c["t"], n, n + 3, fo.OFF), pe.wide(c["t"], n + 3, np.nan))
    tg = _t(c["t"])
    assert plant.follow_targets(tg, "off") is tg
    _sync()
    assert pe.same_bits(tg.cpu().numpy(), c["t"])
    plant.follow_targets(tg, "fit")
    _sync()
    assert not pe.same_bits(tg.cpu().numpy(), c["t"])
    plant.set_terrain(None)
    for mode in ("lift", "fit"):
        tg = _t(c["t"])
        plant.follow_targets(tg, mode)
        _sync()
        assert pe.same_bits(tg.cpu().numpy(), c["t"]), mode
    fresh = GroundContactPlant(MODEL, device=0)
    assert pe.same_bits(_follow_wide(fresh, c["t"], n, n, fo.FIT), c["t"])
    with pytest.raises(ValueError):
        plant.follow_targets(tg, "tilt")
    with pytest.raises(ValueError):
        plant.follow_targets(tg[:53], "fit")
    plant.close(); fresh.close()


# ---- the follow step inside wbc_ground_rollout
def _standing_traj(model=MODEL):
    from quadruped_drake_amd.trajectory import TrunkTrajectory
    return TrunkTrajectory(np.zeros(0), np.zeros((0, 54)), np.zeros(0, np.uint8), model=model, wait_time=1e9, device=0,
                           standing_targets=workloads.standing_targets(model, 1)[:, 0], standing_mask=0b1111)


def _slope_plant(n, scales=None):
    """n robots of fo.slope_start on a plant whose table holds another ground in slot 0 (level, 0.3 m up) and the slope in slot 1."""
    from quadruped_drake_amd import GroundContactPlant, terrain as tr
    scales = tuple(np.linspace(1.0, -1.0, n)) if scales is None else scales
    t, q, v, prof, sc = fo.slope_start(MODEL, scales=scales)
    profiles = [tr.flat(0.3), prof]
    tid = np.ones(n, np.uint8)
    plant = GroundContactPlant(MODEL, device=0)
    plant.set_terrain(profiles, _t(tid), _t(sc))
    return plant, t, q, v, profiles, tid, sc


def _loop(plant, traj, steps, dt, q0, v0):
    """closed_loop with a fresh ID controller -> q, v, and the last tick's tau, flags and targets"""
    from quadruped_drake_amd import IDController, closed_loop
    ctrl = IDController(max_batch=q0.shape[1], device=0)
    q, v, tm = _t(q0), _t(v0), _t(np.zeros(q0.shape[1]))
    out = closed_loop(ctrl, plant, traj, steps, dt, q, v, tm)
    _sync()
    res = [x.cpu().numpy() for x in (q, v, out[0], out[6], out[3])]
    ctrl.close()
    return res


def test_closed_loop_with_follow_off_is_the_closed_loop_without_it():
    n, steps, dt = 8, 5, 5e-3
    traj = _standing_traj()
    plant, _, q0, v0, *_ = _slope_plant(n)
    want = _loop(plant, traj, steps, dt, q0, v0)              # no call to set_follow
    plant.set_follow("fit")
    other = _loop(plant, traj, steps, dt, q0, v0)
    plant.set_follow("off")
    got = _loop(plant, traj, steps, dt, q0, v0)
    for a, b, name in zip(want, got, ("q", "v", "tau", "flags", "targets")):
        assert pe.same_bits(a, b), name
    assert not pe.same_bits(other[0], want[0]) and not pe.same_bits(other[4], want[4])
    # and with follow on but no terrain: the plane's loop
    plant.set_terrain(None)
    flat = _loop(plant, traj, steps, dt, q0, v0)
    plant.set_follow("fit")
    for a, b, name in zip(flat, _loop(plant, traj, steps, dt, q0, v0), ("q", "v", "tau", "flags", "targets")):
        assert pe.same_bits(a, b), name
    plant.close()


def test_closed_loop_with_follow_equals_the_loop_made_by_hand():
    from quadruped_drake_amd import IDController
    n, steps, dt = 5, 5, 5e-3
    traj = _standing_traj()
    plant, _, q0, v0, *_ = _slope_plant(n)
    for mode in ("fit", "lift"):
        plant.set_follow(mode)
        q1, v1, tau1, fl1, tg1 = _loop(plant, traj, steps, dt, q0, v0)
        ctrl = IDController(max_batch=n, device=0)
        q, v, tm = _t(q0), _t(v0), _t(np.zeros(n))
        for _ in range(steps):
            tg, mk = traj.lookup(tm)
            plant.follow_targets(tg, mode)
            tau, met, st = ctrl.step(q, v, tg, mk)
            f, ct, fl = plant.step(q, v, tau, dt, time=tm)
        _sync()
        for a, b, name in zip((q1, v1, tau1, fl1, tg1), (q, v, tau, fl, tg), ("q", "v", "tau", "flags", "targets")):
            assert pe.same_bits(a, b.cpu().numpy()), (mode, name)
        assert np.allclose(tm.cpu().numpy(), steps * dt)
        ctrl.close()
    plant.close()


def test_simulate_follow_is_wired_and_reported(capsys):
    """python -m quadruped_drake_amd.simulate --plant ground --terrain slope:0.2 --follow fit: the JSON line says so, nobody falls or
    turns BAD in 40 ticks of ID, and the trunks end pitched with the slope; without --follow the line reports "off" and the trunks
    are held level."""
    import json
    from quadruped_drake_amd import simulate
    common = ["--control", "ID", "--n", "4", "--sim-time", "0.2", "--dt", "5e-3", "--log-every", "20", "--plant", "ground",
              "--terrain", "slope:0.2"]
    pitch = {}
    for follow in ("fit", "off"):
        a = simulate.parse(common + (["--follow", follow] if follow != "off" else []))
        r = simulate.run(a)
        w, x, y, z = r["q"][0:4]
        pitch[follow] = np.arcsin(2.0 * (w * y - z * x))
        assert r["plant_flags"]["bad"] == 0 and r["plant_flags"]["fell"] == 0 and r["status_nonzero"] == 0, follow
    assert np.abs(pitch["fit"] + 0.2).max() < 0.01 and np.abs(pitch["off"]).max() < np.abs(pitch["fit"]).min()   # slope:0.2 is an angle
    rc = simulate.main(common + ["--follow", "fit"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rc == 0 and line["follow"] == "fit" and line["terrain"] == "slope:0.2" and line["plant_flags"]["bad"] == 0
    simulate.main(common)
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["follow"] == "off"


def test_id_stands_on_four_slopes_with_followed_targets():
    """The scenario of test_follow_cpu on the device: four robots on slopes of grade 0.2 x (1, 0.5, 0, -1) through terrain_scale,
    each square on its own slope, ID, dt 5 ms, 100 ticks, FIT, one tick per closed_loop call.  Per instance: no plant flag, no
    non-zero status, the trunk within 1e-3 of 0.3 m above the ground under it and of the pitch -atan(grade).  Every tick of every
    instance: the device's followed targets equal the host twin's (the bar of this file), and the device's state equals the host
    twin's ground step from the device's previous state under the device's torques (the bar of tests/test_plant_edges_gpu.py:
    1e-9, flags and contact equal but within 1e-6 of a threshold, on at most 1 % of the instance ticks)."""
    import host_terrain as ht
    from quadruped_drake_amd import IDController, closed_loop
    scales = (1.0, 0.5, 0.0, -1.0)
    n, ticks, dt = len(scales), 100, 5e-3
    traj = _standing_traj()
    ctrl = IDController(max_batch=n, device=0)
    plant, t, q0, v0, profiles, tid, sc = _slope_plant(n, scales)
    plant.set_follow("fit")
    want_tg = hf.run(profiles, np.repeat(workloads.standing_targets(MODEL, 1), n, axis=1), "fit", tid, sc)
    q, v, tm = _t(q0), _t(v0), _t(np.zeros(n))
    flags, status, w_tg, w_state, differed = np.zeros(n, np.int32), np.zeros(n, np.int32), 0.0, 0.0, 0
    for k in range(ticks):
        qp, vp = q.cpu().numpy(), v.cpu().numpy()
        out = closed_loop(ctrl, plant, traj, 1, dt, q, v, tm)
        _sync()
        tau, st, tg, f, fl, ct = (out[j].cpu().numpy() for j in (0, 2, 3, 5, 6, 7))
        flags |= fl; status |= st
        w_tg = max(w_tg, worst(tg, want_tg))
        ref = ht.run(t["flat"], qp, vp, tau, act_perm=t.get("act_perm"), dt=dt, profiles=profiles, terrain_id=tid, terrain_scale=sc)
        errs = (pe.rel(q.cpu().numpy(), ref["q"]), pe.rel(v.cpu().numpy(), ref["v"]), pe.rel(f, ref["force"]))
        w_state = max(w_state, *errs)
        assert max(errs) < 1e-9, (k, errs)
        for i in np.flatnonzero((ct != ref["contact"]) | (fl != ref["flags"])):       # only at a threshold, as in test_plant_edges_gpu
            differed += 1
            assert min(to.margin(t, qp[:, i], vp[:, i], tau[:, i], profiles[1], sc[i]),
                       to.margin(t, ref["q"][:, i], ref["v"][:, i], tau[:, i], profiles[1], sc[i])) < 1e-6, (k, i, fl[i], ref["flags"][i])
    height, pitch = fo.trunk_height_and_pitch(q.cpu().numpy(), profiles[1], sc)
    print("FOLLOW device stand: height - 0.3", height - 0.3, "pitch + atan(grade)", pitch + np.arctan(0.2 * sc),
          "worst targets %.3g state %.3g" % (w_tg, w_state))
    assert w_tg < BAR and differed <= 0.01 * n * ticks
    assert (flags == 0).all() and (status == 0).all()
    assert np.abs(height - 0.3).max() < 1e-3 and np.abs(pitch + np.arctan(0.2 * sc)).max() < 1e-3
    assert np.allclose(tm.cpu().numpy(), ticks * dt)
    plant.close(); ctrl.close()
