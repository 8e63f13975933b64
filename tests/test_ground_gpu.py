"""Compliant-ground plant on the MI355X (include/wbc_ground.h, quadruped_drake_amd/plant.py): the device kernel against the dense
numpy plant (tests/ground_oracle.py) and against the host instantiation of the same math (tests/host_ground.py), robustness and
resources, and closed loops: the ID controller standing on the ground, and a push on low friction."""
import numpy as np
import pytest

import ground_oracle as go
import host_ground as hg
from quadruped_drake_amd import workloads

draw, draw_near_stance = go.draw, go.draw_near_stance

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a, dtype=None):
    import torch
    return torch.tensor(np.ascontiguousarray(a), device=DEV, dtype=dtype)


def _rel(a, b):
    return np.abs(a - b).max() / (1.0 + np.abs(b).max())


@pytest.mark.parametrize("cfg", [3, 4])
def test_device_ground_forward_matches_dense_oracle(cfg):
    import torch
    from quadruped_drake_amd import GroundContactPlant
    n = 4096
    t, q, v, tau, sp, we = draw(cfg, n, 100 + cfg)
    model = {3: "mini_cheetah", 4: "anymal_b"}[cfg]
    plant = GroundContactPlant(model, device=0)
    vd, f, ct, fl = plant.forward(_t(q), _t(v), _t(tau), mass_scale=_t(sp), ext_wrench=_t(we))
    torch.cuda.synchronize()
    vd, f, ct, fl = vd.cpu().numpy(), f.cpu().numpy(), ct.cpu().numpy(), fl.cpu().numpy()
    idx = np.random.default_rng(7).choice(n, 256, replace=False)
    bits = (ct[None, idx] >> np.arange(4)[:, None]) & 1
    assert bits.mean() >= 0.2 and (1 - bits).mean() >= 0.2
    assert (f[np.repeat(((ct[None, :] >> np.arange(4)[:, None]) & 1) == 0, 3, axis=0)] == 0).all()   # clear feet: exactly 0
    for backend in ("oracle", "energy"):
        vdo, fo, cto, flo = go.forward(t, q, v, tau, mass_scale=sp, ext_wrench=we, idx=idx, backend=backend)
        assert _rel(vd[:, idx], vdo) < 1e-9 and _rel(f[:, idx], fo) < 1e-9, backend
        assert np.array_equal(ct[idx], cto), backend
        keep = np.array([go.margin(t, q[:, i], v[:, i], tau[:, i], s_p=sp[i], backend=backend) > 1e-6 for i in idx])
        assert keep.sum() >= 0.9 * idx.size, backend
        assert np.array_equal(fl[idx][keep], flo[keep]), backend
        assert ((flo & go.SLIP) != 0).any() and ((flo & go.SLIP) == 0).any()
    # the whole batch against the host instantiation of the same headers
    out = hg.run(t["flat"], q, v, tau, mass_scale=sp, ext_wrench=we, act_perm=t.get("act_perm"))
    assert _rel(vd, out["vdot"]) < 1e-9 and _rel(f, out["force"]) < 1e-9
    assert np.array_equal(ct, out["contact"])
    plant.close()


@pytest.mark.parametrize("model,n", [("mini_cheetah", 1000), ("anymal_b", 203)])
def test_device_ground_step_matches_host(model, n):
    """One step of S = 8 substeps in one launch against the host instantiation; n is no multiple of the 16 robots of a wavefront."""
    import torch
    from quadruped_drake_amd import GroundContactPlant
    dt = 1e-3
    t, q, v, tau, sp, we = draw_near_stance(model, n, 31)
    mu = np.random.default_rng(3).uniform(0.2, 1.0, n)
    plant = GroundContactPlant(model, device=0, max_substep=dt / 8)
    assert plant.substeps(dt) == 8
    qd, vd_, tm = _t(q), _t(v), _t(np.linspace(0.0, 1.0, n))
    counts = torch.zeros((4, n), dtype=torch.int32, device=DEV)
    f, ct, fl = plant.step(qd, vd_, _t(tau), dt, time=tm, mu=_t(mu), mass_scale=_t(sp), ext_wrench=_t(we), counts=counts)
    torch.cuda.synchronize()
    out = hg.run(t["flat"], q, v, tau, mu=mu, mass_scale=sp, ext_wrench=we, act_perm=t.get("act_perm"), dt=dt,
                 params={"max_substep": dt / 8}, time=np.linspace(0.0, 1.0, n), counts=np.zeros((4, n), np.int32))
    assert out["substeps"] == 8
    assert _rel(qd.cpu().numpy(), out["q"]) < 1e-9 and _rel(vd_.cpu().numpy(), out["v"]) < 1e-9
    assert _rel(f.cpu().numpy(), out["force"]) < 1e-9
    assert np.array_equal(ct.cpu().numpy(), out["contact"])
    assert np.array_equal(fl.cpu().numpy(), out["flags"])
    assert np.array_equal(tm.cpu().numpy(), out["time"])
    assert np.array_equal(counts.cpu().numpy(), out["counts"])
    assert not np.array_equal(qd.cpu().numpy(), q)
    plant.close()


def test_nan_instance_is_bad_and_isolated():
    import torch
    from quadruped_drake_amd import GroundContactPlant
    n = 200
    t, q, v, tau, sp, we = draw_near_stance("mini_cheetah", n, 2)
    plant = GroundContactPlant("mini_cheetah", device=0)

    def run(q_, tau_, v_):
        qd, vd_ = _t(q_), _t(v_)
        f, ct, fl = plant.step(qd, vd_, _t(tau_), 1e-3, ext_wrench=_t(we))
        torch.cuda.synchronize()
        return [x.cpu().numpy() for x in (f, ct, fl, qd, vd_)]

    clean = run(q, tau, v)
    qn, tn, vn = q.copy(), tau.copy(), v.copy()
    tn[4, 17] = np.nan; qn[12, 53] = np.nan           # 16 / 52 share their quad's wavefront row
    vn[0, 130] = 1e200                                # finite input, non-finite result inside the substeps
    dirty = run(qn, tn, vn)
    bad = np.zeros(n, bool); bad[[17, 53, 130]] = True
    assert np.array_equal((dirty[2] & go.BAD) != 0, bad)
    for a, c in zip(clean, dirty):
        assert np.array_equal(a[..., ~bad], c[..., ~bad])          # quad-mates and everyone else: bit-identical
    assert (dirty[0][:, bad] == 0).all() and (dirty[1][bad] == 0).all()
    assert np.array_equal(dirty[3][:, bad], qn[:, bad], equal_nan=True) and np.array_equal(dirty[4][:, bad], vn[:, bad])
    plant.close()


def test_ground_kernel_has_no_scratch_and_rollout_refuses_host_handles():
    import ctypes as C
    from quadruped_drake_amd import GroundContactPlant, IDController, plant as plant_mod
    from quadruped_drake_amd.trajectory import TrunkTrajectory
    plant = GroundContactPlant("anymal_b", device=0)
    info = plant.kernel_info()
    assert info["scratch_bytes_per_lane"] == 0 and info["lds_bytes"] == 0 and info["block_threads"] == 64
    h = IDController(max_batch=4, device=0, host_ptrs=True)
    st_t = workloads.standing_targets("mini_cheetah", 1)[:, 0]
    traj = TrunkTrajectory(np.zeros(0), np.zeros((0, 54)), np.zeros(0, np.uint8), wait_time=1e9, device=0, standing_targets=st_t,
                           standing_mask=0b1111)
    L = plant_mod._L()
    P = C.c_void_p(1)
    rc = L.wbc_ground_rollout(h._h, plant._h, traj._h, None, 1, 1e-3, 4, 4, *([P] * 17))
    assert rc < 0 and "WBC_DEVICE_PTRS" in L.wbc_last_error().decode()
    h.close(); plant.close()


def _standing(model="mini_cheetah"):
    from quadruped_drake_amd.trajectory import TrunkTrajectory
    st_t = workloads.standing_targets(model, 1)[:, 0]
    return TrunkTrajectory(np.zeros(0), np.zeros((0, 54)), np.zeros(0, np.uint8), wait_time=1e9, device=0, standing_targets=st_t,
                           standing_mask=0b1111), st_t


def test_id_stand_on_the_ground():
    """The ID controller (which assumes four held feet) standing on the compliant ground: from the reference's initial state with
    the base set so that the feet touch, 1 s at dt = 1 ms (16 substeps per tick).  The same loop on the CPU (tests/host_tick.py +
    tests/host_ground.py, one instance) ends with a trunk-height error of -6.49e-6 m and mean sum f_z / W - 1 = -1.42e-6 over the
    last 0.1 s (profiles/r08/ground.md); the bars are 10 x those."""
    import torch
    from quadruped_drake_amd import GroundContactPlant, IDController, closed_loop
    n, dt = 64, 1e-3
    t, q0, v0 = go.drop_state("mini_cheetah", height=0.0, n=n)
    W = go.defaults(t)["stiffness"] * go.DELTA
    traj, st_t = _standing()
    ctrl = IDController(max_batch=n, device=0)
    plant = GroundContactPlant("mini_cheetah", device=0)
    q, v, tm = _t(q0), _t(v0), _t(np.zeros(n))
    counts = torch.zeros((4, n), dtype=torch.int32, device=DEV)
    closed_loop(ctrl, plant, traj, 900, dt, q, v, tm, counts=counts)
    fz = torch.zeros(n, dtype=torch.float64, device=DEV)
    for _ in range(100):
        out = closed_loop(ctrl, plant, traj, 1, dt, q, v, tm, counts=counts)
        fz += out[5][2::3].sum(0)
    torch.cuda.synchronize()
    counts = counts.cpu().numpy()
    assert (counts[1] == 0).all() and (counts[3] == 0).all()          # no FELL, no BAD
    assert (out[7].cpu().numpy() == 15).all()                          # four feet on the ground
    z_err = q[6].cpu().numpy() - st_t[2]
    load_err = fz.cpu().numpy() / 100 / W - 1.0
    print("height error", z_err[0], "load error", load_err[0])
    assert np.abs(z_err).max() <= 6.488e-5
    assert np.abs(load_err).max() <= 1.4224e-5
    assert np.allclose(tm.cpu().numpy(), 1.0)
    plant.close(); ctrl.close()


def test_push_on_low_friction_slips():
    """A lateral push of 0.5 W on the trunk for T = 0.2 s while the ID controller (friction 0.7 in its QP) stands.  On a ground
    of mu_p = 0.2 every robot raises SLIP and its feet travel beyond v_s T; the same batch on mu_p = 1.0 never raises SLIP and
    every foot that stays in contact throughout moves by at most v_s T (the creep bound of the force law)."""
    import torch
    from quadruped_drake_amd import GroundContactPlant, IDController, closed_loop
    n, dt, T = 32, 1e-3, 0.2
    steps = int(round(T / dt))
    t, q0, v0 = go.drop_state("mini_cheetah", height=0.0, n=n)
    P = go.defaults(t)
    W, vs = P["stiffness"] * go.DELTA, P["v_stiction"]
    traj, st_t = _standing()
    we = np.zeros((6, n)); we[4] = 0.5 * W * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    for mu_p in (0.2, 1.0):
        ctrl = IDController(max_batch=n, device=0)
        plant = GroundContactPlant("mini_cheetah", device=0)
        q, v, tm, mu_d, we_d = _t(q0), _t(v0), _t(np.zeros(n)), _t(np.full(n, mu_p)), _t(we)
        closed_loop(ctrl, plant, traj, 300, dt, q, v, tm, plant_mu=mu_d)                   # settle
        torch.cuda.synchronize()
        qs, vs_, ts = q.clone(), v.clone(), tm.clone()
        p0 = np.array([go.feet_positions(t, c) for c in q.cpu().numpy().T])
        # tick by tick, to follow which feet stay in contact
        counts = torch.zeros((4, n), dtype=torch.int32, device=DEV)
        touching = torch.full((n,), 15, dtype=torch.uint8, device=DEV)
        for _ in range(steps):
            tg, mk = traj.lookup(tm)
            tau, met, st = ctrl.step(q, v, tg, mk)
            f, ct, fl = plant.step(q, v, tau, dt, time=tm, mu=mu_d, ext_wrench=we_d, counts=counts)
            touching &= ct
        # and the same 200 ticks as one closed_loop call with ext_wrench=
        counts2 = torch.zeros((4, n), dtype=torch.int32, device=DEV)
        closed_loop(ctrl, plant, traj, steps, dt, qs, vs_, ts, plant_mu=mu_d, counts=counts2, ext_wrench=we_d)
        torch.cuda.synchronize()
        assert torch.equal(qs, q) and torch.equal(vs_, v) and torch.equal(counts2, counts)
        counts, touching = counts.cpu().numpy(), touching.cpu().numpy()
        p1 = np.array([go.feet_positions(t, c) for c in q.cpu().numpy().T])
        moved = np.linalg.norm((p1 - p0)[:, :, :2], axis=2)            # [instance, foot]
        stayed = ((touching[:, None] >> np.arange(4)[None, :]) & 1) == 1
        print("mu_p", mu_p, "SLIP ticks", counts[0].min(), counts[0].max(), "moved", moved.min(), moved.max(), "stayed", stayed.mean())
        assert (counts[3] == 0).all()
        if mu_p == 0.2:
            assert (counts[0] > 0).all()
            assert (moved.max(1) > vs * T).all()
        else:
            assert (counts[0] == 0).all()
            assert stayed.any(1).all()
            assert (moved[stayed] <= vs * T).all()
        plant.close(); ctrl.close()
