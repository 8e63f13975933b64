"""Rigid-contact plant step on the MI355X (include/wbc_plant.h, quadruped_drake_amd/plant.py): the device kernel against the dense
numpy plant (tests/plant_oracle.py), the plant equal to the controller (one tick and closed loop), a mismatched closed loop checked
tick by tick, predictable physics, robustness and resources."""
import ctypes as C

import numpy as np
import pytest

import plant_oracle as po
from quadruped_drake_amd import load_model, workloads

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a, dtype=None):
    import torch
    return torch.tensor(np.ascontiguousarray(a), device=DEV, dtype=dtype)


def _rel(a, b):
    return np.abs(a - b).max() / (1.0 + np.abs(b).max())


def _trot(model="mini_cheetah"):
    """The stored trot trajectory of bench.py's closed_loop (4 s at 1 kHz, diagonal pairs switching every 150 ms)."""
    st_t = workloads.standing_targets(model, 1)[:, 0]
    K = 4000
    ts = np.arange(K) * 1e-3
    tg = np.tile(st_t, (K, 1))
    tg[:, 0] += 0.01 * np.sin(2 * np.pi * ts / 0.3); tg[:, 3] = 0.01 * 2 * np.pi / 0.3 * np.cos(2 * np.pi * ts / 0.3)
    masks = np.where((np.arange(K) // 150) % 2 == 0, 0b1001, 0b0110).astype(np.uint8)
    for f in range(4):
        sw = ((masks >> f) & 1) == 0
        tg[sw, 18 + 9 * f + 2] += 0.02
    return ts, tg, masks, st_t


def _trot_start(n, seed=1, model="mini_cheetah"):
    rng = np.random.default_rng(seed)
    q0, v0 = workloads.nominal_state(model, n)
    q0[7:] += rng.uniform(-0.03, 0.03, (12, n))
    return q0, v0, rng.uniform(0.0, 0.6, n)


@pytest.mark.parametrize("cfg", [3, 2, 4])
def test_device_plant_matches_dense_oracle(cfg):
    import torch
    from quadruped_drake_amd import RigidContactPlant
    n = 4096
    b = workloads.make_batch(cfg, n=n)
    t = load_model(b["model"])
    rng = np.random.default_rng(100 + cfg)
    tau = rng.uniform(-30.0, 30.0, (12, n)); mask = (np.arange(n) % 16).astype(np.uint8); sp = rng.uniform(0.8, 1.2, n)
    plant = RigidContactPlant(b["model"], device=0)
    vd, f, fl = plant.forward(_t(b["q"]), _t(b["v"]), _t(tau), _t(mask), mass_scale=_t(sp))
    torch.cuda.synchronize()
    vd, f, fl = vd.cpu().numpy(), f.cpu().numpy(), fl.cpu().numpy()
    idx = np.random.default_rng(7).choice(n, 512, replace=False)
    vdo, fo, flo = po.forward(t, b["q"], b["v"], tau, mask, mass_scale=sp, idx=idx)
    assert _rel(vd[:, idx], vdo) < 1e-9 and _rel(f[:, idx], fo) < 1e-9
    keep = np.array([po.margin(t, b["q"][:, i], b["v"][:, i], tau[:, i], int(mask[i]), 1.0, sp[i]) > 1e-6 for i in idx])
    assert keep.sum() > 0.9 * idx.size
    assert np.array_equal(fl[idx][keep], flo[keep])
    assert ((flo & (po.PULL | po.CONE)) != 0).any()
    # and with nothing of oracle/ in the loop: the closed-form terms of tests/energy_model.py, trunk scale included
    vde, fe, fle = po.forward(t, b["q"], b["v"], tau, mask, mass_scale=sp, idx=idx, backend="energy")
    assert _rel(vd[:, idx], vde) < 1e-9 and _rel(f[:, idx], fe) < 1e-9
    keep_e = np.array([po.margin(t, b["q"][:, i], b["v"][:, i], tau[:, i], int(mask[i]), 1.0, sp[i], backend="energy") > 1e-6
                       for i in idx])
    assert keep_e.sum() > 0.9 * idx.size
    assert np.array_equal(fl[idx][keep_e], fle[keep_e])
    plant.close()


@pytest.mark.parametrize("box", [False, True])
@pytest.mark.parametrize("kind", ["id", "mptc", "pc", "clf"])
def test_plant_equals_controller_one_tick(kind, box):
    """With the plant equal to the controller, the plant's accelerations given the QP's torques are the QP's."""
    import torch
    from quadruped_drake_amd import IDController, MPTCController, PCController, CLFController, RigidContactPlant
    cls = {"id": IDController, "mptc": MPTCController, "pc": PCController, "clf": CLFController}[kind]
    b = workloads.make_batch(5, n=1024)       # per-instance mu and mass scale
    tm = {"mptc": 6.0, "pc": 6.0, "id": 12.0, "clf": 12.0}[kind] if box else float("inf")
    ctrl = cls(model=b["model"], max_batch=1024, device=0, params=None if not box else {"tau_max": tm})
    q, v, tg, mk = _t(b["q"]), _t(b["v"]), _t(b["targets"]), _t(b["mask"])
    mu, ms = _t(b["mu"]), _t(b["mass_scale"])
    vq = torch.zeros((18, 1024), dtype=torch.float64, device=DEV)
    ctrl.set_vdot_output(vq)
    tau, met, st = ctrl.step(q, v, tg, mk, mu=mu, mass_scale=ms)
    plant = RigidContactPlant(b["model"], device=0, kd_contact=ctrl.params.Kd_contact, tau_max=tm)
    vd, f, fl = plant.forward(q, v, tau, mk, mu=mu, mass_scale=ms)
    torch.cuda.synchronize()
    st, vq, vd, fl = st.cpu().numpy(), vq.cpu().numpy(), vd.cpu().numpy(), fl.cpu().numpy()
    ok = st == 0
    assert ok.sum() > 900
    assert np.abs(vd[:, ok] - vq[:, ok]).max() <= 1e-8 * (1.0 + np.abs(vq[:, ok]).max())
    assert (fl[ok] & (po.PULL | po.BAD) == 0).all(), np.bincount(fl[ok])
    # CONE: only where the QP's own force sits on its cone to the active-set method's feasibility tolerance (PC's passivity row
    # leaves a handful of ticks 1e-9 .. 1e-7 outside): the plant is not the one that violates it
    f = f.cpu().numpy(); mu_h = b["mu"]
    for i in np.flatnonzero(ok & ((fl & po.CONE) != 0)):
        fi = f[:, i].reshape(4, 3)
        excess = (np.maximum(np.abs(fi[:, 0]), np.abs(fi[:, 1])) - mu_h[i] * fi[:, 2]).max()
        assert excess <= 1e-7 * np.abs(fi).sum(), (i, excess)
    assert (ok & ((fl & po.CONE) != 0)).sum() <= 2
    if box:
        assert (np.abs(tau.cpu().numpy()) >= tm * (1 - 1e-9)).any()   # the box binds somewhere
    plant.close(); ctrl.close()


@pytest.mark.parametrize("kind,dt", [("id", 5e-3), ("mptc", 1e-3)])
def test_closed_loop_equals_plan_following_rollout(kind, dt):
    import torch
    from quadruped_drake_amd import IDController, MPTCController, RigidContactPlant, closed_loop
    from quadruped_drake_amd.trajectory import TrunkTrajectory
    cls = IDController if kind == "id" else MPTCController
    n, steps = 1024, 200
    ts, tg, masks, st_t = _trot()
    traj = TrunkTrajectory(ts, tg, masks, wait_time=0.0, device=0, standing_targets=st_t, standing_mask=0b1111)
    q0, v0, t0 = _trot_start(n)
    ca = cls(max_batch=n, device=0)
    qa, va, ta = _t(q0), _t(v0), _t(t0)
    ca.rollout(traj, steps, dt, qa, va, ta)
    cb = cls(max_batch=n, device=0)
    plant = RigidContactPlant("mini_cheetah", device=0)
    qb, vb, tb = _t(q0), _t(v0), _t(t0)
    counts = torch.zeros((4, n), dtype=torch.int32, device=DEV)
    tau, met, st, tgl, mk, f, fl = closed_loop(cb, plant, traj, steps, dt, qb, vb, tb, counts=counts)
    torch.cuda.synchronize()
    assert (counts[3] == 0).all()
    assert torch.equal(ta, tb)
    for a, c in ((qa, qb), (va, vb)):
        a, c = a.cpu().numpy(), c.cpu().numpy()
        assert np.abs(a - c).max() <= 1e-7 * (1.0 + np.abs(a).max()), np.abs(a - c).max()
    assert ca.stats()["ticks"] == cb.stats()["ticks"] == n * steps
    plant.close(); ca.close(); cb.close()


def test_mismatched_closed_loop_every_tick_against_oracle():
    """Plant trunk 0.8 - 1.2 x the controller's: every tick's device plant step equals the dense numpy plant on the same q, v, tau;
    on every 10th tick also the dense plant over the independent terms (backend "energy"), for 64 of the 256 instances."""
    import torch
    from quadruped_drake_amd import IDController, RigidContactPlant
    from quadruped_drake_amd.trajectory import TrunkTrajectory
    n, steps, dt = 256, 200, 5e-3
    t = load_model("mini_cheetah")
    ts, tg, masks, st_t = _trot()
    traj = TrunkTrajectory(ts, tg, masks, wait_time=0.0, device=0, standing_targets=st_t, standing_mask=0b1111)
    q0, v0, t0 = _trot_start(n, seed=4)
    sp = np.random.default_rng(5).uniform(0.8, 1.2, n)
    ctrl = IDController(max_batch=n, device=0)
    plant = RigidContactPlant("mini_cheetah", device=0)
    q, v, tm, spd = _t(q0), _t(v0), _t(t0), _t(sp)
    worst = 0.0
    for k in range(steps):
        tgk, mk = traj.lookup(tm)
        tau, met, st = ctrl.step(q, v, tgk, mk)
        torch.cuda.synchronize()
        qh, vh, tauh, mkh = q.cpu().numpy(), v.cpu().numpy(), tau.cpu().numpy(), mk.cpu().numpy()
        vd, f, fl = plant.step(q, v, tau, mk, dt, time=tm, mass_scale=spd)
        torch.cuda.synchronize()
        qo, vo, vdo, fo, flo = po.step(t, qh, vh, tauh, mkh, dt, mass_scale=sp)
        fl = fl.cpu().numpy()
        assert _rel(vd.cpu().numpy(), vdo) < 1e-9 and _rel(f.cpu().numpy(), fo) < 1e-9, k
        assert _rel(q.cpu().numpy(), qo) < 1e-9 and _rel(v.cpu().numpy(), vo) < 1e-9, k
        diff = fl != flo
        if diff.any():
            for i in np.flatnonzero(diff):
                assert po.margin(t, qh[:, i], vh[:, i], tauh[:, i], int(mkh[i]), 1.0, sp[i]) < 1e-6, (k, i, fl[i], flo[i])
        if k % 10 == 0:
            qe, ve, vde, fe, fle = po.step(t, qh[:, :64], vh[:, :64], tauh[:, :64], mkh[:64], dt, mass_scale=sp[:64], backend="energy")
            assert _rel(vd.cpu().numpy()[:, :64], vde) < 1e-9 and _rel(f.cpu().numpy()[:, :64], fe) < 1e-9, k
            assert _rel(q.cpu().numpy()[:, :64], qe) < 1e-9 and _rel(v.cpu().numpy()[:, :64], ve) < 1e-9, k
        worst = max(worst, _rel(q.cpu().numpy(), qo))
    assert np.isfinite(q.cpu().numpy()).all()
    plant.close(); ctrl.close()


def _standing(model="mini_cheetah"):
    from quadruped_drake_amd.trajectory import TrunkTrajectory
    st_t = workloads.standing_targets(model, 1)[:, 0]
    return TrunkTrajectory(np.zeros(0), np.zeros((0, 54)), np.zeros(0, np.uint8), wait_time=1e9, device=0, standing_targets=st_t,
                           standing_mask=0b1111), st_t


def test_heavier_trunk_settles_below_target():
    import torch
    from quadruped_drake_amd import IDController, RigidContactPlant, closed_loop
    n, dt, steps = 64, 5e-3, 200
    traj, st_t = _standing()
    z_err = {}
    for s in (1.2, 1.0):
        q0, v0 = workloads.nominal_state("mini_cheetah", n)
        ctrl = IDController(max_batch=n, device=0)
        plant = RigidContactPlant("mini_cheetah", device=0)
        q, v, tm = _t(q0), _t(v0), _t(np.zeros(n))
        closed_loop(ctrl, plant, traj, steps, dt, q, v, tm, plant_mass_scale=_t(np.full(n, s)))
        torch.cuda.synchronize()
        z_err[s] = q[6].cpu().numpy() - st_t[2]
        plant.close(); ctrl.close()
    g, kp = 9.81, 500.0
    pred = (1.2 - 1.0) * g / kp                      # ~3.9 mm if the whole robot were the trunk
    assert (z_err[1.2] < -0.3 * pred).all() and (z_err[1.2] > -1.2 * pred).all(), z_err[1.2]
    assert np.abs(z_err[1.0]).max() * 10 <= np.abs(z_err[1.2]).min()


def test_friction_cone_of_the_plant_ground():
    """bench.py's sideways sway (2 Hz, 5 cm, four feet in stance, 7.9 m/s^2 peak against the controller's 0.7 g): the QP's forces
    reach 0.7 f_z.  On the reference's ground (mu 1.0) no flag; on mu 0.5 every robot leaves the cone on some tick.
    The ID law at dt 1 ms: under MPTC the plan-following loop itself leaves this scenario within the period (the body climbs
    ~9 cm in 0.3 s and the loop diverges after ~0.35 s, with the plant equal to the controller, i.e. exactly wbc_rollout's loop)."""
    import torch
    from quadruped_drake_amd import IDController, RigidContactPlant, closed_loop
    from quadruped_drake_amd.trajectory import TrunkTrajectory
    n, dt, steps = 256, 1e-3, 500
    dur = 0.8
    tss = np.arange(int(round(dur / dt)) + 1) * dt
    tgs = workloads.standing_targets("mini_cheetah", tss.size)
    w = 2 * np.pi * 2.0
    tgs[1] += 0.05 * np.sin(w * tss); tgs[4] = 0.05 * w * np.cos(w * tss); tgs[7] = -0.05 * w * w * np.sin(w * tss)
    sway = TrunkTrajectory(tss, np.ascontiguousarray(tgs.T), np.full(tss.size, 0b1111, np.uint8), wait_time=0.0, device=0)
    rng = np.random.default_rng(0)
    q0, v0 = workloads.nominal_state("mini_cheetah", n)
    q0[7:] += rng.uniform(-0.05, 0.05, (12, n)); v0[0:6] = rng.normal(0, 0.05, (6, n))
    t0 = np.random.default_rng(5).uniform(0.0, 0.2, n)
    res = {}
    for mu_p in (1.0, 0.5):
        ctrl = IDController(max_batch=n, device=0)
        plant = RigidContactPlant("mini_cheetah", device=0, mu=mu_p)
        q, v, tm = _t(q0), _t(v0), _t(t0)
        counts = torch.zeros((4, n), dtype=torch.int32, device=DEV)
        closed_loop(ctrl, plant, sway, steps, dt, q, v, tm, counts=counts)
        torch.cuda.synchronize()
        res[mu_p] = counts.cpu().numpy()
        plant.close(); ctrl.close()
    assert (res[1.0][:2] == 0).all() and (res[1.0][3] == 0).all(), res[1.0].sum(1)
    assert (res[0.5][1] > 0).all(), (res[0.5][1] == 0).sum()


def test_nan_instance_is_bad_and_isolated():
    import torch
    from quadruped_drake_amd import RigidContactPlant
    n = 200
    b = workloads.make_batch(3, n=n)
    rng = np.random.default_rng(2)
    tau = rng.uniform(-30.0, 30.0, (12, n))
    plant = RigidContactPlant("mini_cheetah", device=0)

    def run(q, tau_):
        qd, vd_ = _t(q), _t(b["v"])
        vdot, f, fl = plant.step(qd, vd_, _t(tau_), _t(b["mask"]), 1e-3)
        torch.cuda.synchronize()
        return [x.cpu().numpy() for x in (vdot, f, fl, qd, vd_)]

    clean = run(b["q"], tau)
    qn, tn = b["q"].copy(), tau.copy()
    tn[4, 17] = np.nan; qn[12, 53] = np.nan          # instance 17 (tau), instance 53 (q); 16 / 52 share their wavefront row
    dirty = run(qn, tn)
    bad = np.zeros(n, bool); bad[[17, 53]] = True
    assert np.array_equal((dirty[2] & po.BAD) != 0, bad)
    for a, c in zip(clean, dirty):
        assert np.array_equal(a[..., ~bad], c[..., ~bad])          # bit-identical
    assert (dirty[0][:, bad] == 0).all() and (dirty[1][:, bad] == 0).all()
    assert np.array_equal(dirty[3][:, bad], qn[:, bad], equal_nan=True) and np.array_equal(dirty[4][:, bad], b["v"][:, bad])
    plant.close()


def test_plant_kernel_has_no_scratch_and_rollout_refuses_host_handles():
    from quadruped_drake_amd import IDController, RigidContactPlant, plant as plant_mod
    from quadruped_drake_amd.trajectory import TrunkTrajectory
    plant = RigidContactPlant("anymal_b", device=0)
    info = plant.kernel_info()
    assert info["scratch_bytes_per_lane"] == 0 and info["lds_bytes"] == 0 and info["block_threads"] == 64
    h = IDController(max_batch=4, device=0, host_ptrs=True)
    traj, _ = _standing()
    L = plant_mod._L()
    P = C.c_void_p(1)
    rc = L.wbc_plant_rollout(h._h, plant._h, traj._h, None, 1, 1e-3, 4, 4, *([P] * 15))
    assert rc < 0 and "WBC_DEVICE_PTRS" in L.wbc_last_error().decode()
    h.close(); plant.close()
