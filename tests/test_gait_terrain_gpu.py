"""The gait planner's terrain on the MI355X (include/wbc_gait_terrain.h; gait.GaitPlanner.set_terrain):
wbc_gait_terrain_targets_kernel against the host instantiation of the same header (tests/host_gait_terrain.py) at the bars of
tests/test_gait_terrain_cpu.py, malformed instances in every robot slot of a wavefront, the plain kernel still behind a handle without
a terrain, the new kernel's resources, a terrain gait as the target source of wbc_ground_rollout against the same launches issued by
hand, and ID walking five terrains at once on the compliant ground."""
import ctypes as C
import functools

import numpy as np
import pytest

import follow_oracle as fo
import gait_oracle as go
import gait_terrain_oracle as gto
import host_gait as hg
import host_gait_terrain as hgt
import plant_edges as pe
from quadruped_drake_amd import _lib, gait, terrain as tr, workloads
from test_gait_gpu import DEV, LD, MODEL, NAMES, SIXTEEN, RawGait, _loop, _ptr, _sync, _t
from test_gait_terrain_cpu import GROUPS, MALFORMED, MAX_GRADE, NEAR, WALKS, Z_BAR, host_walk, malformed_batch, spoil

pytestmark = pytest.mark.gpu


class RawTerrainGait(RawGait):
    """RawGait with wbc_gait_set_terrain; the terrain's arrays stay alive here"""

    def set_terrain(self, tp, profiles, tid=None, tsc=None):
        self.keep = [None if tid is None else _t(tid), None if tsc is None else _t(tsc)]
        ctp = gait.c_terrain_params(**tp)
        arr = tr.c_array(profiles)
        _lib.check(self.L.wbc_gait_set_terrain(self.h, C.byref(ctp), C.cast(arr, C.c_void_p), len(profiles), *[_ptr(a) for a in self.keep]))

    def clear_terrain(self):
        _lib.check(self.L.wbc_gait_set_terrain(self.h, None, None, 0, None, None))


@functools.lru_cache(maxsize=None)
def _case(body):
    """LD instances on the sixteen strides of test_gait_gpu and the sixteen profiles of follow_oracle, each with its own scale: seeded
    times, drawn again where they lie within 1e-9 s of a boundary of the stride or where a foothold lies within 1e-9 m of a decision
    of the terrain law (none is dropped).  Read-only."""
    rng = np.random.default_rng(47)
    P = hg.params(wait_time=0.25)
    S = [gait.stride(s) for s in SIXTEEN]
    profiles = fo.sixteen_profiles()
    tp = gto.tparams(body=body, max_grade=MAX_GRADE)
    gid = (np.arange(LD) * 7 % 16).astype(np.uint8)
    tid = (np.arange(LD) * 5 % 16).astype(np.uint8)
    tsc = np.array(fo.SCALES)[(np.arange(LD) // 3) % 4].copy()
    sc = rng.uniform(0.5, 2.0, LD)
    time = np.r_[rng.uniform(-0.05, 0.25, 3), rng.uniform(0.25, 20.25, LD - 3)]
    cmd = np.stack([rng.uniform(-1.0, 1.0, LD), rng.uniform(-1.0, 1.0, LD), rng.uniform(-2.0, 2.0, LD)])
    cmd[2, ::6] = 0.0
    st = np.stack([rng.uniform(-1, 1, LD), rng.uniform(-1, 1, LD), rng.uniform(-3, 3, LD)])
    for _ in range(20):
        info = {}
        gto.targets(P, S, tp, profiles, time, cmd, gid, sc, st, tid, tsc, dtype=np.longdouble, info=info)
        again = np.asarray(info["near"] < NEAR)
        for i in range(3, LD):
            again[i] |= float(go.boundary_distance(S[gid[i]][0], time[i:i + 1], P["wait_time"], sc[i:i + 1])[0]) < 1e-9
        if not again[3:].any():
            break
        time[3:][again[3:]] = rng.uniform(0.25, 20.25, int(again[3:].sum()))
    assert not again.any()
    o64 = gto.targets(P, S, tp, profiles, time, cmd, gid, sc, st, tid, tsc)
    o80 = gto.targets(P, S, tp, profiles, time, cmd, gid, sc, st, tid, tsc, dtype=np.longdouble)
    for a in (gid, tid, tsc, sc, time, cmd, st):
        a.setflags(write=False)
    return dict(P=P, S=S, profiles=profiles, tp=tp, gid=gid, tid=tid, tsc=tsc, sc=sc, time=time, cmd=cmd, st=st, o64=o64, o80=o80)


@pytest.mark.parametrize("body", ["fit", "lift"])
@pytest.mark.parametrize("n", [1, 5, 17, 67])
def test_terrain_kernel_matches_the_host_twin(n, body):
    """n = 1, 5 (a quad tail), 17 (a second quad group of a wavefront's tail), 67 (more than one block of 16 robots), ld = 80 > n;
    every instance with its own stride, stride scale, profile and terrain scale; the bars are the CPU test's, measured over all LD
    instances: 100 x the double oracle's distance from the extended-precision one, per kind of row."""
    c = _case(body)
    g = RawTerrainGait(SIXTEEN, c["P"])
    g.set_terrain(c["tp"], c["profiles"], c["tid"], c["tsc"])
    got, gmask = g.targets(n, LD, c["time"], c["cmd"], c["gid"], c["sc"], c["st"])
    want, wmask = hgt.run(SIXTEEN, c["profiles"], c["time"], c["cmd"], c["gid"], c["sc"], c["st"], c["tid"], c["tsc"], tp=c["tp"], p=c["P"])
    (o64, m64), (o80, _) = c["o64"], c["o80"]
    assert (got[:, n:] == 7.5).all() and (gmask[n:] == 0x55).all()                           # the padding columns: untouched
    assert (gmask[:n] == wmask[:n]).all() and (wmask == m64).all() and np.isfinite(got[:, :n]).all()
    for group, rows in GROUPS:
        bar = 100.0 * float(np.abs(o64[rows] - o80[rows]).max())
        worst = float(np.abs(got[rows, :n] - want[rows, :n]).max())
        print("GAIT-TERRAIN device-to-twin n=%d %s %-14s worst %.3g bar %.3g" % (n, body, group, worst, bar))
        assert worst < bar or (body == "lift" and bar == 0 and worst == 0), (n, body, group, worst, bar)
    if n == 67:                                                                                 # the defaults: profile 0 at scale 1
        g.set_terrain(c["tp"], c["profiles"])
        got, gmask = g.targets(n, LD, c["time"], c["cmd"])
        want, wmask = hgt.run(SIXTEEN, c["profiles"], c["time"], c["cmd"], tp=c["tp"], p=c["P"])
        assert (gmask[:n] == wmask[:n]).all()
        for group, rows in GROUPS:
            bar = 100.0 * float(np.abs(o64[rows] - o80[rows]).max())
            assert float(np.abs(got[rows, :n] - want[rows, :n]).max()) < bar or bar == 0, group
    g.close()


def test_malformed_instances_in_every_slot_of_a_wavefront():
    """17 ways to be malformed -- the gait's 13, a terrain_id beyond the table and three non-finite terrain scales -- x the 16 robot
    slots of a wavefront (every lane quad), one malformed robot per wavefront: NaN rows and mask 0xF for it, and every other robot
    the bits it has in the batch without it."""
    names = ["trot", "walk", "pace"]
    profiles = fo.sixteen_profiles()[:5]
    n = len(MALFORMED) * 16 * 16
    clean = malformed_batch(n, len(names), len(profiles), seed=6)
    dirty = [a.copy() for a in clean]
    bad = np.zeros(n, bool)
    for k, (case, value) in enumerate(MALFORMED):
        for slot in range(16):
            i = (k * 16 + slot) * 16 + slot
            spoil(case, value, i, len(names), len(profiles), *dirty)
            bad[i] = True
    P = hg.params()
    tp = gto.tparams(max_grade=MAX_GRADE)
    g = RawTerrainGait(names, P)
    g.set_terrain(tp, profiles, clean[5], clean[6])
    ct, cm = g.targets(n, n, *clean[:5])
    g.set_terrain(tp, profiles, dirty[5], dirty[6])
    dt_, dm = g.targets(n, n, *dirty[:5])
    assert np.isfinite(ct).all()
    assert np.isnan(dt_[:, bad]).all() and (dm[bad] == 0xF).all()
    assert pe.same_bits(dt_[:, ~bad], ct[:, ~bad]) and (dm[~bad] == cm[~bad]).all()
    twin, tmask = hgt.run(names, profiles, *dirty, tp=tp, p=P)
    assert np.array_equal(np.isnan(twin), np.isnan(dt_)) and (tmask == dm).all()
    g.close()


def test_a_handle_without_a_terrain_still_launches_the_plain_kernel():
    """A handle that never had a terrain, one after set_terrain then clear_terrain, and GaitPlanner after clear_terrain(): the plain
    kernel's answer bit for bit; with the terrain set the answer is another.  The new kernel: 0 scratch, 64 threads, the two tables
    in LDS; the plain kernel's resources are what they were."""
    import torch
    rng = np.random.default_rng(3)
    n = 37
    P = hg.params()
    time, cmd = rng.uniform(0.0, 6.0, n), np.stack([rng.uniform(-1, 1, n), rng.uniform(-0.5, 0.5, n), rng.uniform(-2, 2, n)])
    sc = rng.uniform(0.5, 2.0, n)
    fresh = RawTerrainGait(["trot", "walk"], P)
    plain, pmask = fresh.targets(n, n, time, cmd, None, sc)
    g = RawTerrainGait(["trot", "walk"], P)
    g.set_terrain(gto.tparams(), [tr.ramp_step(0.3, 0.1)])
    on, _ = g.targets(n, n, time, cmd, None, sc)
    g.clear_terrain()
    off, omask = g.targets(n, n, time, cmd, None, sc)
    assert pe.same_bits(off, plain) and (omask == pmask).all() and not pe.same_bits(on, plain)
    twin, _ = hg.run(["trot", "walk"], time, cmd, None, sc, p=P)
    assert np.abs(plain - twin).max() < 1e-9
    fresh.close(); g.close()
    p = gait.GaitPlanner(MODEL, strides=("trot", "walk"), device=0)
    p.set_commands(_t(cmd), stride_scale=_t(sc))
    a = p.targets(_t(time))[0].cpu().numpy()
    p.set_terrain([tr.ramp_step(0.3, 0.1)], body="lift")
    assert p.has_terrain
    b = p.targets(_t(time))[0].cpu().numpy()
    p.clear_terrain()
    c = p.targets(_t(time))[0].cpu().numpy()
    on_twin = hgt.run(["trot", "walk"], [tr.ramp_step(0.3, 0.1)], time, cmd, None, sc, tp=gto.tparams(body="lift"), p=P)[0]
    assert pe.same_bits(a, plain) and pe.same_bits(c, plain) and not pe.same_bits(b, plain) and not p.has_terrain
    assert np.abs(b - on_twin).max() < 1e-9 and np.abs(b - plain).max() > 0.05
    p.set_terrain([tr.flat()], terrain_id=torch.zeros(n + 1, dtype=torch.uint8, device=DEV))      # ids for another batch size
    with pytest.raises(ValueError):
        p.targets(_t(time))
    info, old = p.terrain_kernel_info(), p.kernel_info()
    print("GAIT-TERRAIN kernel", info, "plain", old)
    assert info["scratch_bytes_per_lane"] == 0 and info["block_threads"] == 64
    assert info["lds_bytes"] == 8 * (12 + 16 * 204 + 12 + 16 * 40) and 0 < info["num_regs"] <= 256
    assert old["lds_bytes"] == 8 * (12 + 16 * 204) and old["scratch_bytes_per_lane"] == 0
    p.close()


FIVE = [lambda: tr.flat(0.0), WALKS["kerb_0.10"][0], WALKS["stairs_0.08"][0], WALKS["yawed_kerb_arc"][0], lambda: tr.ridge(0.3, 0.5, 0.5, 0.1)]
CMD5 = np.array([(0.2, 0.0, 0.0), (0.2, 0.0, 0.0), (0.2, 0.0, 0.0), (0.3, 0.0, 0.4), (0.2, 0.0, 0.0)]).T.copy()


def _terrain_planner(n=5, body="fit", profiles=None):
    p = gait.GaitPlanner(MODEL, strides=("trot",), device=0)
    p.set_commands(_t(CMD5[:, :n]), stride_scale=_t(np.full(n, 0.5)))
    p.set_terrain([f() for f in FIVE] if profiles is None else profiles, terrain_id=_t(np.arange(n, dtype=np.uint8)), body=body)
    return p


def test_ground_rollout_with_a_terrain_gait_equals_the_launches_made_by_hand():
    """40 ticks of wbc_ground_rollout with a terrain gait set against wbc_gait_targets (the terrain kernel) -> wbc_step ->
    wbc_ground_step issued one by one: bit-identical.  Five kerbs of 0.02 .. 0.10 m that begin 5 mm ahead of the front feet, so that
    the first footholds are already moved off them: another answer than the plain gait's.  And closed_loop refuses the pair of a
    terrain gait and a plant that follows."""
    from quadruped_drake_amd import GroundContactPlant, IDController
    n, steps, dt = 5, 40, 5e-3
    q0, v0 = workloads.nominal_state(MODEL, n)
    kerbs = [tr.ramp_step(0.18, 0.02 * (k + 1), yaw=0.1 * k) for k in range(n)]
    plant = GroundContactPlant(MODEL, device=0)
    plant.set_terrain(kerbs, terrain_id=_t(np.arange(n, dtype=np.uint8)))
    planner = _terrain_planner(n, profiles=kerbs)
    got = _loop(plant, planner, steps, dt, q0, v0)
    ctrl = IDController(max_batch=n, device=0)
    q, v, tm = _t(q0), _t(v0), _t(np.zeros(n))
    for _ in range(steps):
        tg, mk = planner.targets(tm)
        tau, met, st = ctrl.step(q, v, tg, mk)
        f, ct, fl = plant.step(q, v, tau, dt, time=tm)
    _sync()
    for a, b, name in zip(got, (q, v, tau, fl, tg, mk), NAMES):
        assert pe.same_bits(a, b.cpu().numpy()), name
    ctrl.close()
    plant.set_follow("fit")
    with pytest.raises(ValueError, match="follow"):
        _loop(plant, planner, steps, dt, q0, v0)
    plant.set_follow("off")
    planner.clear_terrain()
    flat = _loop(plant, planner, steps, dt, q0, v0)
    assert not pe.same_bits(flat[4], got[4])
    plant.close(); planner.close()


def test_id_walks_five_terrains_on_the_device():
    """The scenarios of tests/test_gait_terrain_cpu.py on the device, five robots in one batch on five terrains -- flat, the kerb of
    0.10 m, the stairs of 0.08 m, the yawed kerb on its arc, a ridge of 0.1 m: Mini Cheetah, ID, 800 ticks of 5 ms, trot at stride
    scale 0.5, FIT.  No FELL, no BAD, status 0 on every tick, every trunk within 0.03 m of its planned (x, y) and within 1.6 mm of
    its planned z (the CPU test's bars), and the final poses within 0.03 m of the host twins' runs."""
    import torch
    from quadruped_drake_amd import GroundContactPlant, IDController, closed_loop
    n, ticks, dt = 5, 800, 5e-3
    q0, v0 = workloads.nominal_state(MODEL, n)
    profiles = [f() for f in FIVE]
    plant = GroundContactPlant(MODEL, device=0)
    plant.set_terrain(profiles, terrain_id=_t(np.arange(n, dtype=np.uint8)))
    planner = _terrain_planner(n)
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
    want = gto.targets(hg.params(MODEL), [gait.stride("trot")], gto.tparams(), profiles, np.full(n, ticks * dt), CMD5, None, np.full(n, 0.5),
                       None, np.arange(n))[0]
    off, dz = np.hypot(qf[4] - want[0], qf[5] - want[1]), qf[6] - want[2]
    print("GAIT-TERRAIN device walk: x", qf[4], "y", qf[5], "z", qf[6], "off", off, "dz", dz, "slip ticks", cn[0])
    assert np.abs(plan[0:3] - want[0:3]).max() < 1e-9 and np.allclose(tm.cpu().numpy(), ticks * dt)
    assert (cn[1] == 0).all() and (cn[3] == 0).all() and s["ticks"] == n * ticks and s["status_nonzero"] == 0
    assert (off < 0.03).all() and (np.abs(dz) < Z_BAR).all()
    for i in range(n):
        r = host_walk(profiles[i], CMD5[:, i])
        print("GAIT-TERRAIN device against host walk %d: device (%.4f, %.4f, %.4f) host (%.4f, %.4f, %.4f)" % (i, qf[4, i], qf[5, i], qf[6, i], r["x"], r["y"], r["z"]))
        assert not r["flags"] & 10 and np.linalg.norm([qf[4, i] - r["x"], qf[5, i] - r["y"], qf[6, i] - r["z"]]) < 0.03
    plant.close(); planner.close(); ctrl.close()


def test_simulate_gait_terrain_is_wired_and_reported(capsys):
    """python -m quadruped_drake_amd.simulate --planner gait --terrain ramp_step:0.1 --gait-terrain fit: the JSON line names the mode,
    and 4 robots walk 4 s over the kerb of 0.10 m without FELL or BAD, within 0.03 m of their plan."""
    import json
    from quadruped_drake_amd import simulate
    rc = simulate.main(["--control", "ID", "--n", "4", "--sim-time", "4.0", "--dt", "5e-3", "--log-every", "200", "--planner", "gait", "--cmd", "0.2,0,0",
                        "--plant", "ground", "--terrain", "ramp_step:0.1", "--gait-terrain", "fit"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rc == 0 and line["gait_terrain"] == "fit" and line["follow"] == "off" and line["terrain"] == "ramp_step:0.1"
    assert line["FELL"] == 0 and line["plant_flags"]["bad"] == 0 and line["plan_offset_worst"] < 0.03
    assert 0.39 < line["body_height_final"][0] <= line["body_height_final"][1] < 0.41
