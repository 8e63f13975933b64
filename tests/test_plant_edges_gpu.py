"""The two plants on the MI355X at the edges of their ABI (include/wbc_plant.h, include/wbc_ground.h): renumbered joints and
actuators, ld > n and batch tails, handle parameters that differ from every default, every substep count and optional pointer,
the ground closed loop tick by tick against the dense numpy plant, the routing of the four mu / mass_scale arrays, and malformed
instances in every robot slot of a wavefront.  References: tests/ground_oracle.py and tests/plant_oracle.py over both of their
backends, and the host instantiations tests/host_ground.py and tests/host_plant.py.  Bars: _rel < 1e-9 with
_rel(a, b) = max|a - b| / (1 + max|b|); flags and contact equal except where go.margin / po.margin is below 1e-6, on at most a
tenth of the compared instances (1 % in the closed loop).  Each test prints its worst figures ("EDGE ..." lines); the host twins
are in tests/test_ground_cpu.py and tests/test_plant_cpu.py, the recorded figures in profiles/r09/plant_edges.md."""
import ctypes as C

import numpy as np
import pytest

import ground_oracle as go
import host_ground as hg
import host_plant as hp
import plant_edges as pe
import plant_oracle as po
from quadruped_drake_amd import load_model, workloads
from test_plant_gpu import _trot

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BACKENDS = ["oracle", "energy"]
MODEL_OF = {2: "mini_cheetah", 3: "mini_cheetah", 4: "anymal_b"}
_rel = pe.rel


def _t(a, dtype=None):
    import torch
    return None if a is None else torch.tensor(np.ascontiguousarray(a), device=DEV, dtype=dtype)


def _h(x):
    return x.cpu().numpy()


def _sync():
    import torch
    torch.cuda.synchronize()


def _note(test, **kw):
    print("EDGE", test, " ".join("%s=%s" % (k, ("%.3g" % x) if isinstance(x, float) else x) for k, x in kw.items()))


def _ptr(x):
    return None if x is None else C.c_void_p(x.data_ptr())


# ---- the C ABI with (rows, ld) tensors: plant.py always passes ld = n
def _ground_forward(plant, n, ld, q, v, tau, mu=None, ms=None, we=None, vdot=None, force=None, contact=None, flags=None):
    from quadruped_drake_amd import _lib
    _lib.check(plant._L.wbc_ground_forward(plant._h, plant._stream(), n, ld, *[_ptr(x) for x in (q, v, tau, mu, ms, we, vdot, force, contact, flags)]))


def _ground_step(plant, n, ld, dt, q, v, tau, time=None, mu=None, ms=None, we=None, force=None, contact=None, flags=None, counts=None):
    from quadruped_drake_amd import _lib
    _lib.check(plant._L.wbc_ground_step(plant._h, plant._stream(), n, ld, float(dt),
                                        *[_ptr(x) for x in (q, v, time, tau, mu, ms, we, force, contact, flags, counts)]))


def _rigid_forward(plant, n, ld, q, v, tau, mask, mu=None, ms=None, vdot=None, force=None, flags=None):
    from quadruped_drake_amd import _lib
    _lib.check(plant._L.wbc_plant_forward(plant._h, plant._stream(), n, ld, *[_ptr(x) for x in (q, v, tau, mask, mu, ms, vdot, force, flags)]))


def _rigid_step(plant, n, ld, dt, q, v, tau, mask, time=None, mu=None, ms=None, vdot=None, force=None, flags=None, counts=None):
    from quadruped_drake_amd import _lib
    _lib.check(plant._L.wbc_plant_step(plant._h, plant._stream(), n, ld, float(dt),
                                       *[_ptr(x) for x in (q, v, time, tau, mask, mu, ms, vdot, force, flags, counts)]))


def _standing(model="mini_cheetah"):
    from quadruped_drake_amd.trajectory import TrunkTrajectory
    st_t = workloads.standing_targets(model, 1)[:, 0]
    return TrunkTrajectory(np.zeros(0), np.zeros((0, 54)), np.zeros(0, np.uint8), model=model, wait_time=1e9, device=0,
                           standing_targets=st_t, standing_mask=0b1111)


def _trot_traj():
    from quadruped_drake_amd.trajectory import TrunkTrajectory
    ts, tg, masks, st_t = _trot()
    return TrunkTrajectory(ts, tg, masks, wait_time=0.0, device=0, standing_targets=st_t, standing_mask=0b1111)


def _flags_outside_margin(name, got, want, keep, cap=0.9):
    """Flags (or contact) equal on the kept instances, and the kept share is at least `cap`."""
    assert keep.sum() >= cap * keep.size, (name, keep.sum(), keep.size)
    assert np.array_equal(got[keep], want[keep]), (name, np.flatnonzero(got != want))
    return 1.0 - keep.mean()


# =============================================================== 1. renumbered joints and actuators
@pytest.mark.parametrize("cfg", [3, 4])
def test_ground_forward_with_renumbered_joints_and_actuators(cfg):
    from quadruped_drake_amd import GroundContactPlant
    n = 256
    t, q, v, tau, sp, we = go.draw(cfg, n, 41)
    qp, ap = pe.perm_pair(5, avoid=t.get("act_perm", range(12)))
    q2, v2 = pe.permute_rows(q, v, qp)
    plant = GroundContactPlant(MODEL_OF[cfg], device=0, q_perm=qp, act_perm=ap)
    vd2, f, ct, fl = [_h(x) for x in plant.forward(_t(q2), _t(v2), _t(tau), mass_scale=_t(sp), ext_wrench=_t(we))]
    vd = pe.canonical_v(vd2, qp)
    t2 = pe.table_with(t, ap)
    worst, left = 0.0, 0.0
    for backend in BACKENDS:
        vdo, fo, cto, flo = go.forward(t2, q, v, tau, mass_scale=sp, ext_wrench=we, backend=backend)
        worst = max(worst, _rel(vd, vdo), _rel(f, fo))
        assert _rel(vd, vdo) < 1e-9 and _rel(f, fo) < 1e-9, backend
        assert np.array_equal(ct, cto), backend
        left = max(left, _flags_outside_margin(backend, fl, flo, pe.ground_margin_keep(t2, q, v, tau, sp, None, backend)))
    out = hg.run(t["flat"], q2, v2, tau, mass_scale=sp, ext_wrench=we, q_perm=qp, act_perm=ap)
    assert _rel(vd2, out["vdot"]) < 1e-9 and _rel(f, out["force"]) < 1e-9
    assert np.array_equal(ct, out["contact"]) and np.array_equal(fl, out["flags"])
    # only the row addresses differ from the identity-numbered launch: the same bits after un-permuting
    ident = GroundContactPlant(MODEL_OF[cfg], device=0, act_perm=list(range(12)))
    vdi, fi, cti, fli = [_h(x) for x in ident.forward(_t(q), _t(v), _t(pe.tau_for_identity(tau, ap)), mass_scale=_t(sp), ext_wrench=_t(we))]
    assert pe.same_bits(vd, vdi) and pe.same_bits(f, fi) and np.array_equal(ct, cti) and np.array_equal(fl, fli)
    _note("ground_forward_renumbered[%d]" % cfg, oracle=worst, host=max(_rel(vd2, out["vdot"]), _rel(f, out["force"])), left_out=left)
    plant.close(); ident.close()


@pytest.mark.parametrize("model", ["mini_cheetah", "anymal_b"])
def test_ground_step_with_renumbered_joints_and_actuators(model):
    """One step of S = 8: the whole batch against the host instantiation, 48 sampled instances against the dense plant."""
    import torch
    from quadruped_drake_amd import GroundContactPlant
    n, dt, S = 203, 1e-3, 8
    t, q, v, tau, sp, we = go.draw_near_stance(model, n, 45)
    qp, ap = pe.perm_pair(6, avoid=t.get("act_perm", range(12)))
    q2, v2 = pe.permute_rows(q, v, qp)
    t2 = pe.table_with(t, ap)

    def run(plant, q_, v_, tau_):
        qd, vd_, tm = _t(q_), _t(v_), _t(np.linspace(0.0, 1.0, n))
        counts = torch.zeros((4, n), dtype=torch.int32, device=DEV)
        f, ct, fl = plant.step(qd, vd_, _t(tau_), dt, time=tm, mass_scale=_t(sp), ext_wrench=_t(we), counts=counts)
        return [_h(x) for x in (qd, vd_, f, ct, fl, tm, counts)]

    plant = GroundContactPlant(model, device=0, max_substep=dt / S, q_perm=qp, act_perm=ap)
    assert plant.substeps(dt) == S
    q2n, v2n, f, ct, fl, tm, counts = run(plant, q2, v2, tau)
    qn, vn = pe.canonical_q(q2n, qp), pe.canonical_v(v2n, qp)
    out = hg.run(t["flat"], q2, v2, tau, mass_scale=sp, ext_wrench=we, q_perm=qp, act_perm=ap, dt=dt, params={"max_substep": dt / S},
                 time=np.linspace(0.0, 1.0, n), counts=np.zeros((4, n), np.int32))
    assert out["substeps"] == S
    host = max(_rel(q2n, out["q"]), _rel(v2n, out["v"]), _rel(f, out["force"]))
    assert host < 1e-9
    assert np.array_equal(ct, out["contact"]) and np.array_equal(fl, out["flags"])
    assert np.array_equal(tm, out["time"]) and np.array_equal(counts, out["counts"])
    idx = np.random.default_rng(7).choice(n, 48, replace=False)
    worst, left = 0.0, 0.0
    for backend in BACKENDS:
        qo, vo, fo, cto, flo = go.step(t2, q[:, idx], v[:, idx], tau[:, idx], dt, S, mass_scale=sp[idx], ext_wrench=we[:, idx], backend=backend)
        worst = max(worst, _rel(qn[:, idx], qo), _rel(vn[:, idx], vo), _rel(f[:, idx], fo))
        assert _rel(qn[:, idx], qo) < 1e-9 and _rel(vn[:, idx], vo) < 1e-9 and _rel(f[:, idx], fo) < 1e-9, backend
        # a threshold may be met at the start or at the end of the step: both states have to be clear of it
        keep = pe.ground_margin_keep(t2, q, v, tau, sp, None, backend, idx) & pe.ground_margin_keep(t2, qo, vo, tau[:, idx], sp[idx], None, backend)
        left = max(left, _flags_outside_margin(backend, fl[idx], flo, keep), _flags_outside_margin(backend, ct[idx], cto, keep))
    ident = GroundContactPlant(model, device=0, max_substep=dt / S, act_perm=list(range(12)))
    qi, vi, fi, cti, fli, tmi, ci = run(ident, q, v, pe.tau_for_identity(tau, ap))
    assert pe.same_bits(qn, qi) and pe.same_bits(vn, vi) and pe.same_bits(f, fi)
    assert np.array_equal(ct, cti) and np.array_equal(fl, fli) and np.array_equal(counts, ci)
    _note("ground_step_renumbered[%s]" % model, oracle=worst, host=host, left_out=left)
    plant.close(); ident.close()


ODD3 = dict(kd_contact=37.0, tau_max=28.0, mu=0.45)      # each differs from its default (100, inf, 1.0)


@pytest.mark.parametrize("cfg", [2, 3, 4])
def test_rigid_plant_with_renumbered_joints_actuators_and_odd_parameters(cfg):
    """Forward and one step under a random q_perm / act_perm, on a handle whose Kd_contact, tau_max and mu all differ from their
    defaults (no per-instance mu is passed: the handle's is the one used), against the dense plant over both backends."""
    from quadruped_drake_amd import RigidContactPlant
    n, dt = 256, 2e-3
    b = workloads.make_batch(cfg, n=n)
    t = load_model(b["model"])
    rng = np.random.default_rng(200 + cfg)
    tau = rng.uniform(-30.0, 30.0, (12, n)); mask = (np.arange(n) % 16).astype(np.uint8); sp = rng.uniform(0.8, 1.2, n)
    q, v = b["q"], b["v"]
    qp, ap = pe.perm_pair(7, avoid=t.get("act_perm", range(12)))
    q2, v2 = pe.permute_rows(q, v, qp)
    t2 = pe.table_with(t, ap)
    kw = dict(mass_scale=sp, kd=ODD3["kd_contact"], tau_max=ODD3["tau_max"], mu0=ODD3["mu"])

    def run(plant, q_, v_, tau_):
        fw = [_h(x) for x in plant.forward(_t(q_), _t(v_), _t(tau_), _t(mask), mass_scale=_t(sp))]
        qd, vd_ = _t(q_), _t(v_)
        st = [_h(x) for x in plant.step(qd, vd_, _t(tau_), _t(mask), dt, mass_scale=_t(sp))]
        return fw, st, _h(qd), _h(vd_)

    plant = RigidContactPlant(b["model"], device=0, q_perm=qp, act_perm=ap, **ODD3)
    (vd2, f, fl), (vds, fs, fls), q2n, v2n = run(plant, q2, v2, tau)
    assert pe.same_bits(vd2, vds) and pe.same_bits(f, fs) and np.array_equal(fl, fls)      # the step's forward part
    vd, qn, vn = pe.canonical_v(vd2, qp), pe.canonical_q(q2n, qp), pe.canonical_v(v2n, qp)
    worst, left = 0.0, 0.0
    for backend in BACKENDS:
        qo, vo, vdo, fo, flo = po.step(t2, q, v, tau, mask, dt, backend=backend, **kw)
        worst = max(worst, _rel(vd, vdo), _rel(f, fo), _rel(qn, qo), _rel(vn, vo))
        assert _rel(vd, vdo) < 1e-9 and _rel(f, fo) < 1e-9 and _rel(qn, qo) < 1e-9 and _rel(vn, vo) < 1e-9, backend
        keep = np.array([po.margin(t2, q[:, i], v[:, i], tau[:, i], int(mask[i]), ODD3["mu"], sp[i], ODD3["kd_contact"], ODD3["tau_max"],
                                   backend) > 1e-6 for i in range(n)])
        left = max(left, _flags_outside_margin(backend, fl, flo, keep))
        for bit in (po.PULL | po.CONE, po.CLIP):
            assert ((flo & bit) != 0).any() and ((flo & bit) == 0).any(), (backend, bit)
    # each parameter matters: the dense plant at its default gives another answer
    sub = np.arange(64)
    for k, x in (("kd", 100.0), ("tau_max", np.inf)):
        assert _rel(po.forward(t2, q, v, tau, mask, idx=sub, **dict(kw, **{k: x}))[0], vdo[:, sub]) > 1e-3, k
    assert not np.array_equal(po.forward(t2, q, v, tau, mask, idx=sub, **dict(kw, mu0=1.0))[2], flo[sub])
    out = hp.run(t["flat"], q2, v2, tau, mask, mass_scale=sp, params3=[ODD3["kd_contact"], ODD3["tau_max"], ODD3["mu"]], q_perm=qp, act_perm=ap)
    host = max(_rel(vd2, out["vdot"]), _rel(f, out["force"]))
    assert host < 1e-9
    ident = RigidContactPlant(b["model"], device=0, act_perm=list(range(12)), **ODD3)
    (vdi, fi, fli), _, qi, vi = run(ident, q, v, pe.tau_for_identity(tau, ap))
    assert pe.same_bits(vd, vdi) and pe.same_bits(f, fi) and np.array_equal(fl, fli) and pe.same_bits(qn, qi) and pe.same_bits(vn, vi)
    _note("rigid_renumbered[%d]" % cfg, oracle=worst, host=host, left_out=left)
    plant.close(); ident.close()


def test_ground_closed_loop_with_renumbered_joints_and_actuators():
    """50 ticks of the ID trot on the ground with controller and plant built on the same non-identity q_perm / act_perm: the
    identity-numbered loop, un-permuted, bit for bit."""
    import torch
    from quadruped_drake_amd import GroundContactPlant, IDController, closed_loop
    n, steps, dt = 35, 50, 1e-3
    t = load_model("mini_cheetah")
    q0, v0, t0 = pe.trot_ground_start(n, 3)
    qp, ap = pe.perm_pair(8, avoid=t.get("act_perm", range(12)))
    traj = _trot_traj()
    rng = np.random.default_rng(4)
    mu_p, s_p = rng.uniform(0.3, 1.0, n), rng.uniform(0.8, 1.2, n)
    res = []
    for perms, (qs, vs) in ((dict(q_perm=qp, act_perm=ap), pe.permute_rows(q0, v0, qp)), (dict(), (q0, v0))):
        ctrl = IDController(max_batch=n, device=0, **perms)
        plant = GroundContactPlant("mini_cheetah", device=0, **perms)
        q, v, tm = _t(qs), _t(vs), _t(t0)
        counts = torch.zeros((4, n), dtype=torch.int32, device=DEV)
        out = closed_loop(ctrl, plant, traj, steps, dt, q, v, tm, plant_mu=_t(mu_p), plant_mass_scale=_t(s_p), counts=counts)
        _sync()
        res.append([_h(x) for x in (q, v, tm, counts, out[5], out[7], out[6])])
        plant.close(); ctrl.close()
    (qa, va, *ra), (qb, vb, *rb) = res
    assert not pe.same_bits(qa, qb)
    assert pe.same_bits(pe.canonical_q(qa, qp), qb) and pe.same_bits(pe.canonical_v(va, qp), vb)
    for a, c in zip(ra, rb):
        assert pe.same_bits(a, c)
    assert (rb[1][3] == 0).all() and not np.array_equal(qb, q0)          # no BAD, and the robots moved
    assert len(set(rb[3].tolist())) >= 2                                 # feet in different contact patterns


# =============================================================== 2. ld > n and batch tails
def _wide_runner(kernel):
    """-> run(n, ld): launches `kernel` on the first n instances of a fixed 203-instance batch held in arrays of ld columns, and
    returns name -> (array as left on the device, what its padding held before the call)."""
    import torch
    from quadruped_drake_amd import GroundContactPlant, IDController, RigidContactPlant, _lib
    ground, rollout = kernel.startswith("ground"), kernel.endswith("rollout")
    step = kernel.endswith("step") or rollout
    model = "mini_cheetah" if rollout else "anymal_b"
    N = 203
    # parameters under which every flag but BAD is raised on part of the batch: counts rows are only written where one is
    if ground:
        t, b = pe.ground_batch(model, N, 11)
        plant = GroundContactPlant(model, device=0, tau_max=9.5, v_stiction=0.01, fall_height=float(np.median(b["q"][6])))
    else:
        t, b = pe.rigid_batch(3 if rollout else 4, N, 11)
        plant = RigidContactPlant(model, device=0, tau_max=9.5)
    b["time"] = np.linspace(0.0, 1.0, N)
    b["counts"] = (np.arange(4 * N).reshape(4, N) % 3).astype(np.int32)
    ctrl = IDController(model=model, max_batch=256, device=0) if rollout else None
    traj = _standing(model) if rollout else None
    dt = 1e-3

    def run(n, ld):
        nan = lambda k: _t(pe.wide(b[k][..., :n], ld, np.nan))
        sent = lambda k: _t(pe.wide(b[k][..., :n], ld))
        new = lambda rows, dtype: _t(pe.wide(np.zeros(((rows, 0) if rows else (0,)), dtype), ld))
        a, fill = {}, {}
        for k in ("q", "v"):
            a[k] = sent(k) if step else nan(k); fill[k] = None if step else np.nan
        for k in ("tau", "mu", "mass_scale") + (("ext_wrench",) if ground else ()):
            a[k] = nan(k); fill[k] = np.nan
        if not ground:
            a["mask"] = sent("mask"); fill["mask"] = None
        for k, rows, dtype in (("vdot", 18, np.float64), ("force", 12, np.float64), ("flags", 0, np.int32), ("contact", 0, np.uint8)):
            if (k != "contact" or ground) and not (k == "vdot" and ground and step):
                a[k] = new(rows, dtype); fill[k] = None
        if step:
            a["time"] = sent("time"); a["counts"] = sent("counts"); fill["time"] = fill["counts"] = None
        if rollout:
            # the controller's arrays: written by the loop itself, so all of them start as sentinels (tau too)
            a["tau"] = new(12, np.float64); fill["tau"] = None
            for k, rows, dtype in (("targets", 54, np.float64), ("metrics", 4, np.float64), ("status", 0, np.int32)):
                a[k] = new(rows, dtype); fill[k] = None
            if ground:
                a["mask"] = new(0, np.uint8); fill["mask"] = None
            a["ctrl_mu"] = _t(pe.wide(np.full(n, 0.6), ld, np.nan)); a["ctrl_ms"] = _t(pe.wide(np.full(n, 1.05), ld, np.nan))
            fill["ctrl_mu"] = fill["ctrl_ms"] = np.nan
            s = torch.cuda.current_stream(0).cuda_stream
            if ground:
                rc = plant._L.wbc_ground_rollout(ctrl._h, plant._h, traj._h, C.c_void_p(s), 3, dt, n, ld, *[_ptr(a[k]) for k in (
                    "q", "v", "time", "targets", "mask", "ctrl_mu", "ctrl_ms", "mu", "mass_scale", "ext_wrench", "tau", "metrics", "status",
                    "force", "contact", "flags", "counts")])
            else:
                rc = plant._L.wbc_plant_rollout(ctrl._h, plant._h, traj._h, C.c_void_p(s), 3, dt, n, ld, *[_ptr(a[k]) for k in (
                    "q", "v", "time", "targets", "mask", "ctrl_mu", "ctrl_ms", "mu", "mass_scale", "tau", "metrics", "status", "force",
                    "flags", "counts")])
            _lib.check(rc)
            ctrl._bound_stream = s
        elif ground and step:
            _ground_step(plant, n, ld, dt, a["q"], a["v"], a["tau"], a["time"], a["mu"], a["mass_scale"], a["ext_wrench"], a["force"],
                         a["contact"], a["flags"], a["counts"])
        elif ground:
            _ground_forward(plant, n, ld, a["q"], a["v"], a["tau"], a["mu"], a["mass_scale"], a["ext_wrench"], a["vdot"], a["force"],
                            a["contact"], a["flags"])
        elif step:
            _rigid_step(plant, n, ld, dt, a["q"], a["v"], a["tau"], a["mask"], a["time"], a["mu"], a["mass_scale"], a["vdot"], a["force"],
                        a["flags"], a["counts"])
        else:
            _rigid_forward(plant, n, ld, a["q"], a["v"], a["tau"], a["mask"], a["mu"], a["mass_scale"], a["vdot"], a["force"], a["flags"])
        _sync()
        return {k: (_h(x), fill[k]) for k, x in a.items()}

    def close():
        plant.close()
        if ctrl is not None:
            ctrl.close()
    return run, close, b


@pytest.mark.parametrize("kernel", ["ground_forward", "ground_step", "rigid_forward", "rigid_step", "ground_rollout", "rigid_rollout"])
def test_wide_arrays_and_batch_tails(kernel):
    """n in {1, 17, 203} (15 dead quads, a tail of one robot, a tail of 11) in arrays of ld = n, n + 5 and 256 columns, every optional
    array given.  Padding columns: NaN in the inputs, a sentinel in everything a kernel writes.  The columns below n are the
    ld = n run's bit for bit, every padding column keeps its bits, nobody is BAD, and n = 1 and n = 17 are the first columns of
    the n = 203 run: what the dead quads compute on robot n - 1 goes nowhere."""
    run, close, b = _wide_runner(kernel)
    big = run(203, 203)
    assert (big["flags"][0] & pe.BAD == 0).all()
    if "forward" not in kernel:
        raised = (big["counts"][0] - b["counts"]) > 0                    # [4, 203]
        rows = {"ground_step": [raised[0], raised[1], raised[2]], "rigid_step": [raised[0], raised[2]],
                "ground_rollout": [raised[1]], "rigid_rollout": [raised[0]]}[kernel]
        for r in rows:
            assert r.any() and not r.all(), (kernel, raised.sum(1))
    for k in ("force",) + (("q", "v", "time", "counts") if "forward" not in kernel else ("vdot",)):
        assert np.isfinite(big[k][0]).all(), k
    for n in (1, 17, 203):
        base = big if n == 203 else run(n, n)
        for k, (x, _) in base.items():
            assert pe.same_bits(x, big[k][0][..., :n]), (kernel, n, k)
        for ld in (n + 5, 256):
            got = run(n, ld)
            for k, (x, fill) in got.items():
                assert x.shape[-1] == ld
                assert pe.same_bits(x[..., :n], base[k][0]), (kernel, n, ld, k)
                assert pe.padding_kept(x, n, fill), (kernel, n, ld, k)
    close()


# =============================================================== 3. handle parameters, CLIP and FELL on the device
@pytest.mark.parametrize("cfg", [3, 4])
def test_ground_handle_parameters_reach_the_kernels(cfg):
    """A handle whose every parameter differs from its default (foot_radius, tau_max, fall_height, mu, stiffness, dissipation,
    v_stiction; no per-instance mu): forward on draw(cfg, 256, 41) and one S = 8 step near stance against the dense plant with the
    same parameters.  SLIP, FELL and CLIP are each raised and not raised in the batch, and clipping changes the answer exactly
    where CLIP is set."""
    from quadruped_drake_amd import GroundContactPlant
    n = 256
    model = MODEL_OF[cfg]
    t, q, v, tau, sp, we = go.draw(cfg, n, 41)
    over = pe.odd_ground_params(t, q)
    P = go.params(t, over)
    plant = GroundContactPlant(model, device=0, **over)
    vd, f, ct, fl = [_h(x) for x in plant.forward(_t(q), _t(v), _t(tau), mass_scale=_t(sp), ext_wrench=_t(we))]
    unclipped = GroundContactPlant(model, device=0, **dict(over, tau_max=None))
    vdu = _h(unclipped.forward(_t(q), _t(v), _t(tau), mass_scale=_t(sp), ext_wrench=_t(we))[0])
    clip = (fl & go.CLIP) != 0
    assert np.array_equal(clip, (np.abs(tau) > over["tau_max"] * (1 + 1e-9)).any(0))
    assert (np.abs(vdu - vd)[:, clip].max(0) > 1e-3).all() and pe.same_bits(vdu[:, ~clip], vd[:, ~clip])
    worst, left = 0.0, 0.0
    for backend in BACKENDS:
        vdo, fo, cto, flo = go.forward(t, q, v, tau, mass_scale=sp, ext_wrench=we, P=P, backend=backend)
        worst = max(worst, _rel(vd, vdo), _rel(f, fo))
        assert _rel(vd, vdo) < 1e-9 and _rel(f, fo) < 1e-9, backend
        assert np.array_equal(ct, cto), backend
        left = max(left, _flags_outside_margin(backend, fl, flo, pe.ground_margin_keep(t, q, v, tau, sp, P, backend)))
        for bit in (go.SLIP, go.FELL, go.CLIP):
            assert ((flo & bit) != 0).any() and ((flo & bit) == 0).any(), (backend, bit)
    matters = pe.ground_params_that_matter(t, q[:, :64], v[:, :64], tau[:, :64], sp[:64], we[:, :64], over)
    # one step of S = 8 near stance, FELL judged at the end state
    ns, dt, S = 64, 1e-3, 8
    t, q, v, tau, sp, we = go.draw_near_stance(model, ns, 47)
    over = dict(pe.odd_ground_params(t, q), tau_max=9.5, max_substep=dt / S)
    P = go.params(t, over)
    stepper = GroundContactPlant(model, device=0, **over)
    assert stepper.substeps(dt) == S
    qd, vd_ = _t(q), _t(v)
    fs, cts, fls = [_h(x) for x in stepper.step(qd, vd_, _t(tau), dt, mass_scale=_t(sp), ext_wrench=_t(we))]
    qn, vn = _h(qd), _h(vd_)
    idx = np.arange(0, ns, 2)
    wstep = 0.0
    for backend in BACKENDS:
        qo, vo, fo, cto, flo = go.step(t, q[:, idx], v[:, idx], tau[:, idx], dt, S, mass_scale=sp[idx], ext_wrench=we[:, idx], P=P, backend=backend)
        wstep = max(wstep, _rel(qn[:, idx], qo), _rel(vn[:, idx], vo), _rel(fs[:, idx], fo))
        assert _rel(qn[:, idx], qo) < 1e-9 and _rel(vn[:, idx], vo) < 1e-9 and _rel(fs[:, idx], fo) < 1e-9, backend
        keep = pe.ground_margin_keep(t, q, v, tau, sp, P, backend, idx) & pe.ground_margin_keep(t, qo, vo, tau[:, idx], sp[idx], P, backend)
        left = max(left, _flags_outside_margin(backend, fls[idx], flo, keep), _flags_outside_margin(backend, cts[idx], cto, keep))
        for bit in (go.FELL, go.CLIP):
            assert ((flo & bit) != 0).any() and ((flo & bit) == 0).any(), (backend, bit)
    # every parameter matters to the dense plant on one batch or the other, so a default left in the kernel's arguments cannot pass
    matters |= pe.ground_params_that_matter(t, q, v, tau, sp, we, over)
    assert matters == set(over) - {"max_substep"}, matters
    out = hg.run(t["flat"], q, v, tau, mass_scale=sp, ext_wrench=we, act_perm=t.get("act_perm"), params=over, dt=dt)
    host = max(_rel(qn, out["q"]), _rel(vn, out["v"]), _rel(fs, out["force"]))
    assert host < 1e-9 and np.array_equal(cts, out["contact"]) and np.array_equal(fls, out["flags"])
    _note("ground_handle_parameters[%d]" % cfg, oracle_forward=worst, oracle_step=wstep, host_step=host, left_out=left)
    plant.close(); unclipped.close(); stepper.close()


# =============================================================== 4. substep counts and every optional pointer
@pytest.mark.parametrize("S,dt", pe.substep_cases())
@pytest.mark.parametrize("model", ["mini_cheetah", "anymal_b"])
def test_ground_step_at_every_substep_count(model, S, dt):
    import torch
    from quadruped_drake_amd import GroundContactPlant
    n = 64
    t, q, v, tau, sp, we = go.draw_near_stance(model, n, 43)
    mu = np.random.default_rng(3).uniform(0.2, 1.0, n)
    plant = GroundContactPlant(model, device=0)
    assert plant.substeps(dt) == S
    qd, vd_, tm = _t(q), _t(v), _t(np.linspace(0.0, 1.0, n))
    counts = torch.zeros((4, n), dtype=torch.int32, device=DEV)
    f, ct, fl = [_h(x) for x in plant.step(qd, vd_, _t(tau), dt, time=tm, mu=_t(mu), mass_scale=_t(sp), ext_wrench=_t(we), counts=counts)]
    qn, vn = _h(qd), _h(vd_)
    out = hg.run(t["flat"], q, v, tau, mu=mu, mass_scale=sp, ext_wrench=we, act_perm=t.get("act_perm"), dt=dt,
                 time=np.linspace(0.0, 1.0, n), counts=np.zeros((4, n), np.int32))
    assert out["substeps"] == S
    host = max(_rel(qn, out["q"]), _rel(vn, out["v"]), _rel(f, out["force"]))
    assert host < 1e-9
    assert np.array_equal(ct, out["contact"]) and np.array_equal(fl, out["flags"])
    assert np.array_equal(_h(tm), out["time"]) and np.array_equal(_h(counts), out["counts"])
    idx = np.arange(0, n, 4)
    qo, vo, fo, cto, flo = go.step(t, q[:, idx], v[:, idx], tau[:, idx], dt, S, mu=mu[idx], mass_scale=sp[idx], ext_wrench=we[:, idx])
    worst = max(_rel(qn[:, idx], qo), _rel(vn[:, idx], vo), _rel(f[:, idx], fo))
    assert worst < 1e-9
    _note("ground_substeps[%s-%d]" % (model, S), oracle=worst, host=host)
    plant.close()


@pytest.mark.parametrize("model", ["mini_cheetah", "anymal_b"])
def test_ground_every_optional_pointer_null(model):
    """The step with time, mu, mass_scale, ext_wrench, force, contact, flags and counts all NULL leaves q and v as the step that
    is given all of them with the defaults' values (mu = params.mu, mass_scale = 1, zero wrench); the forward kernel with vdot
    and force NULL in turn writes the other outputs as before."""
    import torch
    from quadruped_drake_amd import GroundContactPlant
    n, dt = 67, 1e-3
    t, q, v, tau, sp, we = go.draw_near_stance(model, n, 44)
    plant = GroundContactPlant(model, device=0, mu=0.6)
    tau_d = _t(tau)
    qa, va = _t(q), _t(v)
    f, ct, fl = plant.step(qa, va, tau_d, dt, time=_t(np.zeros(n)), mu=_t(np.full(n, plant.params.mu)), mass_scale=_t(np.ones(n)),
                           ext_wrench=_t(np.zeros((6, n))), counts=torch.zeros((4, n), dtype=torch.int32, device=DEV))
    qb, vb = _t(q), _t(v)
    _ground_step(plant, n, n, dt, qb, vb, tau_d)
    _sync()
    assert torch.equal(qa, qb) and torch.equal(va, vb) and not pe.same_bits(_h(qb), q)
    full = [_h(x) for x in plant.forward(_t(q), _t(v), tau_d)]
    for drop in ("vdot", "force", "all"):
        outs = dict(vdot=_t(pe.wide(np.zeros((18, 0)), n)), force=_t(pe.wide(np.zeros((12, 0)), n)),
                    contact=_t(pe.wide(np.zeros(0, np.uint8), n)), flags=_t(pe.wide(np.zeros(0, np.int32), n)))
        given = {k: (None if drop in (k, "all") else x) for k, x in outs.items()}
        _ground_forward(plant, n, n, _t(q), _t(v), tau_d, **given)
        _sync()
        for k, ref in zip(("vdot", "force", "contact", "flags"), full):
            if given[k] is None:
                assert pe.padding_kept(_h(outs[k]), 0), (drop, k)
            else:
                assert pe.same_bits(_h(outs[k]), ref), (drop, k)
    plant.close()


@pytest.mark.parametrize("cfg", [3, 4])
def test_rigid_every_optional_pointer_null(cfg):
    import torch
    from quadruped_drake_amd import RigidContactPlant
    n, dt = 67, 1e-3
    t, b = pe.rigid_batch(cfg, n, 12)
    plant = RigidContactPlant(MODEL_OF[cfg], device=0, mu=0.6)
    tau_d, mk = _t(b["tau"]), _t(b["mask"])
    qa, va = _t(b["q"]), _t(b["v"])
    plant.step(qa, va, tau_d, mk, dt, time=_t(np.zeros(n)), mu=_t(np.full(n, 0.6)), mass_scale=_t(np.ones(n)),
               counts=torch.zeros((4, n), dtype=torch.int32, device=DEV))
    qb, vb = _t(b["q"]), _t(b["v"])
    _rigid_step(plant, n, n, dt, qb, vb, tau_d, mk)
    _sync()
    assert torch.equal(qa, qb) and torch.equal(va, vb) and not pe.same_bits(_h(qb), b["q"])
    full = [_h(x) for x in plant.forward(_t(b["q"]), _t(b["v"]), tau_d, mk)]
    for drop in ("vdot", "force", "flags"):
        outs = dict(vdot=_t(pe.wide(np.zeros((18, 0)), n)), force=_t(pe.wide(np.zeros((12, 0)), n)), flags=_t(pe.wide(np.zeros(0, np.int32), n)))
        given = {k: (None if k == drop else x) for k, x in outs.items()}
        _rigid_forward(plant, n, n, _t(b["q"]), _t(b["v"]), tau_d, mk, **given)
        _sync()
        for k, ref in zip(("vdot", "force", "flags"), full):
            assert pe.padding_kept(_h(outs[k]), 0) if given[k] is None else pe.same_bits(_h(outs[k]), ref), (drop, k)
    plant.close()


# =============================================================== 5. the closed loop on the ground, every tick against the oracle
def _ground_loop_setup(n, seed):
    rng = np.random.default_rng(seed + 1)
    q0, v0, t0 = pe.trot_ground_start(n, seed)
    return q0, v0, t0, dict(mu_p=rng.uniform(0.3, 1.0, n), s_p=rng.uniform(0.8, 1.2, n), mu_c=rng.uniform(0.4, 1.0, n),
                            s_c=rng.uniform(0.8, 1.2, n))


def test_ground_closed_loop_every_tick_against_oracle():
    """MPTC trotting on the compliant ground, 64 robots that differ in start, trot phase, plant friction and trunk mass, and in
    the friction and mass the controller assumes; 100 ticks of 1 ms at 16 substeps.  Every tick's device ground step against the
    host instantiation on the same q, v, tau for the whole batch; every fourth tick against the dense plant on 8 instances
    (every twentieth: backend "energy").  Then the same 100 ticks as ONE closed_loop call given all four of mu, mass_scale,
    plant_mu and plant_mass_scale as different arrays: bit for bit the tick-by-tick loop that routed them by hand."""
    import torch
    from quadruped_drake_amd import GroundContactPlant, MPTCController, closed_loop
    n, steps, dt, S = 64, 100, 1e-3, 16
    t = load_model("mini_cheetah")
    traj = _trot_traj()
    q0, v0, t0, p = _ground_loop_setup(n, 7)
    we = np.zeros((6, n)); we[4] = np.random.default_rng(9).normal(0.0, 2.0, n)          # a small lateral push, held
    ctrl = MPTCController(max_batch=n, device=0)
    plant = GroundContactPlant("mini_cheetah", device=0)
    assert plant.substeps(dt) == S
    q, v, tm = _t(q0), _t(v0), _t(t0)
    mu_c, s_c, mu_p, s_p, we_d = _t(p["mu_c"]), _t(p["s_c"]), _t(p["mu_p"]), _t(p["s_p"]), _t(we)
    counts = torch.zeros((4, n), dtype=torch.int32, device=DEV)
    host, oracle = 0.0, 0.0
    patterns, slip_ticks, compared, differed = set(), 0, 0, 0
    sample = np.arange(0, n, 8)
    for k in range(steps):
        tgk, mk = traj.lookup(tm)
        tau, met, st = ctrl.step(q, v, tgk, mk, mu=mu_c, mass_scale=s_c)
        _sync()
        qh, vh, tauh = _h(q), _h(v), _h(tau)
        f, ct, fl = plant.step(q, v, tau, dt, time=tm, mu=mu_p, mass_scale=s_p, ext_wrench=we_d, counts=counts)
        _sync()
        qn, vn, f, ct, fl = _h(q), _h(v), _h(f), _h(ct), _h(fl)
        out = hg.run(t["flat"], qh, vh, tauh, mu=p["mu_p"], mass_scale=p["s_p"], ext_wrench=we, act_perm=t.get("act_perm"), dt=dt)
        assert out["substeps"] == S
        host = max(host, _rel(qn, out["q"]), _rel(vn, out["v"]), _rel(f, out["force"]))
        assert _rel(qn, out["q"]) < 1e-9 and _rel(vn, out["v"]) < 1e-9 and _rel(f, out["force"]) < 1e-9, k
        for i in np.flatnonzero((ct != out["contact"]) | (fl != out["flags"])):
            differed += 1
            assert min(go.margin(t, qh[:, i], vh[:, i], tauh[:, i], p["mu_p"][i], p["s_p"][i]),
                       go.margin(t, out["q"][:, i], out["v"][:, i], tauh[:, i], p["mu_p"][i], p["s_p"][i])) < 1e-6, (k, i, fl[i], out["flags"][i])
        compared += n
        if k % 4 == 0:
            backend = "energy" if k % 20 == 0 else "oracle"
            s_ = sample
            qo, vo, fo, cto, flo = go.step(t, qh[:, s_], vh[:, s_], tauh[:, s_], dt, S, mu=p["mu_p"][s_], mass_scale=p["s_p"][s_],
                                           ext_wrench=we[:, s_], backend=backend)
            oracle = max(oracle, _rel(qn[:, s_], qo), _rel(vn[:, s_], vo), _rel(f[:, s_], fo))
            assert _rel(qn[:, s_], qo) < 1e-9 and _rel(vn[:, s_], vo) < 1e-9 and _rel(f[:, s_], fo) < 1e-9, (k, backend)
            for j in np.flatnonzero((ct[s_] != cto) | (fl[s_] != flo)):
                i = s_[j]
                differed += 1
                assert min(go.margin(t, qh[:, i], vh[:, i], tauh[:, i], p["mu_p"][i], p["s_p"][i], backend=backend),
                           go.margin(t, qo[:, j], vo[:, j], tauh[:, i], p["mu_p"][i], p["s_p"][i], backend=backend)) < 1e-6, (k, i)
            compared += s_.size
        patterns |= set(ct.tolist())
        slip_ticks += int(((fl & go.SLIP) != 0).sum())
        assert (fl & (go.BAD | go.FELL) == 0).all(), (k, np.flatnonzero(fl & (go.BAD | go.FELL)))
    assert differed <= 0.01 * compared, (differed, compared)
    # the run is no trivial loop
    assert len(patterns) >= 6, sorted(patterns)
    assert any(pt != 15 for pt in patterns)
    assert 0 < slip_ticks < n * steps
    c = _h(counts)
    assert c[0].sum() == slip_ticks and (c[1] == 0).all() and (c[3] == 0).all()
    _note("ground_closed_loop_every_tick", host=host, oracle=oracle, differed=differed, compared=compared, patterns=sorted(patterns),
          slip_instance_ticks=slip_ticks)
    # ---- the same 100 ticks as one call; each of the four arrays has to reach its own party
    ctrl2 = MPTCController(max_batch=n, device=0)
    q2, v2, tm2 = _t(q0), _t(v0), _t(t0)
    counts2 = torch.zeros((4, n), dtype=torch.int32, device=DEV)
    closed_loop(ctrl2, plant, traj, steps, dt, q2, v2, tm2, mu=mu_c, mass_scale=s_c, plant_mu=mu_p, plant_mass_scale=s_p, counts=counts2,
                ext_wrench=we_d)
    _sync()
    assert torch.equal(q2, q) and torch.equal(v2, v) and torch.equal(tm2, tm) and torch.equal(counts2, counts)
    plant.close(); ctrl.close(); ctrl2.close()


def test_rigid_closed_loop_routes_the_four_arrays():
    """ID trot on the rigid plant, 50 ticks: closed_loop with mu, mass_scale, plant_mu and plant_mass_scale all different equals
    the tick-by-tick loop that hands mu / mass_scale to the controller and plant_mu / plant_mass_scale to the plant; and each of
    the four changes the outcome, so a swap cannot hide."""
    import torch
    from quadruped_drake_amd import IDController, RigidContactPlant, closed_loop
    n, steps, dt = 64, 50, 2e-3
    traj = _trot_traj()
    rng = np.random.default_rng(11)
    q0, v0 = workloads.nominal_state("mini_cheetah", n)
    q0[7:] += rng.uniform(-0.03, 0.03, (12, n))
    t0 = rng.uniform(0.0, 0.6, n)
    # friction below what the sway of the trot needs (~0.45 f_z): the controller's cone binds and the plant's is left
    arr = dict(mu=rng.uniform(0.05, 0.3, n), mass_scale=rng.uniform(0.8, 1.2, n), plant_mu=rng.uniform(0.05, 0.3, n),
               plant_mass_scale=rng.uniform(0.8, 1.2, n))
    plant = RigidContactPlant("mini_cheetah", device=0)

    def whole(**kw):
        ctrl = IDController(max_batch=n, device=0)
        q, v, tm = _t(q0), _t(v0), _t(t0)
        counts = torch.zeros((4, n), dtype=torch.int32, device=DEV)
        closed_loop(ctrl, plant, traj, steps, dt, q, v, tm, counts=counts, **{k: _t(x) for k, x in kw.items()})
        _sync()
        ctrl.close()
        return q, v, tm, counts

    ctrl = IDController(max_batch=n, device=0)
    q, v, tm = _t(q0), _t(v0), _t(t0)
    counts = torch.zeros((4, n), dtype=torch.int32, device=DEV)
    d = {k: _t(x) for k, x in arr.items()}
    for _ in range(steps):
        tgk, mk = traj.lookup(tm)
        tau, met, st = ctrl.step(q, v, tgk, mk, mu=d["mu"], mass_scale=d["mass_scale"])
        plant.step(q, v, tau, mk, dt, time=tm, mu=d["plant_mu"], mass_scale=d["plant_mass_scale"], counts=counts)
    _sync()
    ref = (q, v, tm, counts)
    got = whole(**arr)
    for a, c in zip(ref, got):
        assert torch.equal(a, c)
    assert (counts[3] == 0).all() and (counts[1] > 0).any()          # no BAD; the low plant friction shows as CONE
    for k in arr:                                                     # each array matters on its own
        other = whole(**dict(arr, **{k: arr[k][::-1].copy()}))
        assert not (torch.equal(other[0], q) and torch.equal(other[3], counts)), k
    plant.close(); ctrl.close()


def test_anymal_ground_rollout_equals_tick_by_tick():
    """ANYmal, the ID controller standing, n = 35 with starts that all differ: wbc_ground_rollout against the launch-per-stage loop."""
    import torch
    from quadruped_drake_amd import GroundContactPlant, IDController, closed_loop
    n, steps, dt = 35, 40, 1e-3
    t, q0, v0, tau0, sp, we = go.draw_near_stance("anymal_b", n, 51)
    rng = np.random.default_rng(52)
    arr = dict(mu=rng.uniform(0.4, 1.0, n), mass_scale=rng.uniform(0.9, 1.1, n), plant_mu=rng.uniform(0.3, 1.0, n), plant_mass_scale=sp)
    d = {k: _t(x) for k, x in arr.items()}
    traj = _standing("anymal_b")
    plant = GroundContactPlant("anymal_b", device=0)
    ctrl = IDController(model="anymal_b", max_batch=n, device=0)
    q, v, tm = _t(q0), _t(v0), _t(np.zeros(n))
    counts = torch.zeros((4, n), dtype=torch.int32, device=DEV)
    for _ in range(steps):
        tgk, mk = traj.lookup(tm)
        tau, met, st = ctrl.step(q, v, tgk, mk, mu=d["mu"], mass_scale=d["mass_scale"])
        f, ct, fl = plant.step(q, v, tau, dt, time=tm, mu=d["plant_mu"], mass_scale=d["plant_mass_scale"], counts=counts)
    ctrl2 = IDController(model="anymal_b", max_batch=n, device=0)
    q2, v2, tm2 = _t(q0), _t(v0), _t(np.zeros(n))
    counts2 = torch.zeros((4, n), dtype=torch.int32, device=DEV)
    out = closed_loop(ctrl2, plant, traj, steps, dt, q2, v2, tm2, counts=counts2, **d)
    _sync()
    assert torch.equal(q2, q) and torch.equal(v2, v) and torch.equal(tm2, tm) and torch.equal(counts2, counts)
    assert torch.equal(out[0], tau) and torch.equal(out[5], f) and torch.equal(out[7], ct) and torch.equal(out[6], fl)
    assert (counts[3] == 0).all() and (counts[1] == 0).all() and np.isfinite(_h(q)).all()
    assert len({tuple(c) for c in _h(q).T.round(9)}) == n
    plant.close(); ctrl.close(); ctrl2.close()


# =============================================================== 6. malformed instances in every slot
def _poison_runs(ground, model_or_cfg):
    """-> (t, base batch, run(batch, step) -> dict of host arrays) on a plant with tau_max = 25 (the batch's torques stay below 10)."""
    import torch
    from quadruped_drake_amd import GroundContactPlant, RigidContactPlant
    n, dt = 80, 1e-3
    if ground:
        t, base = pe.ground_batch(model_or_cfg, n, 17)
        plant = GroundContactPlant(model_or_cfg, device=0, tau_max=25.0)
    else:
        t, base = pe.rigid_batch(model_or_cfg, n, 17)
        plant = RigidContactPlant(MODEL_OF[model_or_cfg], device=0, tau_max=25.0)
    base["time"] = np.linspace(0.0, 1.0, n)
    base["counts"] = (np.arange(4 * n).reshape(4, n) % 5).astype(np.int32)

    def run(b, step):
        q, v, tau, mu, ms = _t(b["q"]), _t(b["v"]), _t(b["tau"]), _t(b["mu"]), _t(b["mass_scale"])
        o = {}
        if ground and not step:
            o["vdot"], o["force"], o["contact"], o["flags"] = plant.forward(q, v, tau, mu=mu, mass_scale=ms, ext_wrench=_t(b["ext_wrench"]))
        elif ground:
            o["time"], o["counts"] = _t(b["time"]), _t(b["counts"])
            o["force"], o["contact"], o["flags"] = plant.step(q, v, tau, dt, time=o["time"], mu=mu, mass_scale=ms,
                                                              ext_wrench=_t(b["ext_wrench"]), counts=o["counts"])
        elif not step:
            o["vdot"], o["force"], o["flags"] = plant.forward(q, v, tau, _t(b["mask"]), mu=mu, mass_scale=ms)
        else:
            o["time"], o["counts"] = _t(b["time"]), _t(b["counts"])
            o["vdot"], o["force"], o["flags"] = plant.step(q, v, tau, _t(b["mask"]), dt, time=o["time"], mu=mu, mass_scale=ms, counts=o["counts"])
        if step:
            o["q"], o["v"] = q, v
        _sync()
        return {k: _h(x) for k, x in o.items()}
    return t, base, run, plant, dt


@pytest.mark.parametrize("plant_kind,which", [("ground", "mini_cheetah"), ("ground", "anymal_b"), ("rigid", 3), ("rigid", 4)])
def test_malformed_instance_in_every_wavefront_slot(plant_kind, which):
    """Every kind of pe.plant_poisons, one forward and one step launch per kind at n = 80: the kind sits in each of the 16 robot
    slots of a wavefront once (slot s in wavefront (s + kind) mod 5), next to clean quads, and the per-leg kinds put it on every
    lane of the quad.  The damaged instances: flags BAD exactly -- CLIP | BAD exactly where a torque is over the limit --, zero
    force, vdot and contact, q and v untouched, counts row 3 (and row 2 with CLIP) incremented, time advanced.  Everybody else:
    the clean run's bits.  A quaternion of norm 3.7 is legal: the dense plant's answer, no BAD."""
    ground = plant_kind == "ground"
    t, base, run, plant, dt = _poison_runs(ground, which)
    clean = {s: run(base, s) for s in (False, True)}
    assert (clean[False]["flags"] & (pe.BAD | pe.CLIP) == 0).all() and (clean[True]["flags"] & (pe.BAD | pe.CLIP) == 0).all()
    kinds = pe.plant_poisons(t.get("act_perm", range(12)), ground, 40.0)
    seen_slots, worst = set(), 0.0
    for j, (name, (damage, want)) in enumerate(kinds.items()):
        b = pe.copy_batch(base)
        hit = pe.slots_of(j)
        assert sorted(hit % 16) == list(range(16))
        for i in hit:
            damage(b, i)
        ok = np.ones(80, bool); ok[hit] = False
        for step in (False, True):
            out = run(b, step)
            for k, x in clean[step].items():
                assert pe.same_bits(out[k][..., ok], x[..., ok]), (name, step, k)
            if want == "legal":
                assert (out["flags"][hit] & pe.BAD == 0).all(), name
                if ground:
                    a = [x[..., hit] for x in (b["q"], b["v"], b["tau"], b["mu"], b["mass_scale"], b["ext_wrench"])]
                    if step:
                        qo, vo, fo, cto, flo = go.step(t, a[0], a[1], a[2], dt, 16, a[3], a[4], a[5], go.params(t, {"tau_max": 25.0}))
                        worst = max(worst, _rel(out["q"][:, hit], qo), _rel(out["v"][:, hit], vo), _rel(out["force"][:, hit], fo))
                    else:
                        vdo, fo, cto, flo = go.forward(t, a[0], a[1], a[2], a[3], a[4], a[5], go.params(t, {"tau_max": 25.0}))
                        worst = max(worst, _rel(out["vdot"][:, hit], vdo), _rel(out["force"][:, hit], fo))
                    assert np.array_equal(out["contact"][hit], cto)
                else:
                    qo, vo, vdo, fo, flo = po.step(t, b["q"][:, hit], b["v"][:, hit], b["tau"][:, hit], b["mask"][hit], dt, mu=b["mu"][hit],
                                                   mass_scale=b["mass_scale"][hit], tau_max=25.0)
                    worst = max(worst, _rel(out["vdot"][:, hit], vdo), _rel(out["force"][:, hit], fo))
                    if step:
                        worst = max(worst, _rel(out["q"][:, hit], qo), _rel(out["v"][:, hit], vo))
                assert worst < 1e-9, (name, worst)
                assert np.array_equal(out["flags"][hit], flo), name
                continue
            flags = pe.BAD | (pe.CLIP if want == "clip_bad" else 0)
            assert (out["flags"][hit] == flags).all(), (name, step, out["flags"][hit])
            assert (out["force"][:, hit] == 0).all(), (name, step)
            if "vdot" in out:
                assert (out["vdot"][:, hit] == 0).all(), (name, step)
            if ground:
                assert (out["contact"][hit] == 0).all(), (name, step)
            if step:
                assert pe.same_bits(out["q"][:, hit], b["q"][:, hit]) and pe.same_bits(out["v"][:, hit], b["v"][:, hit]), name
                want_counts = base["counts"][:, hit].copy()
                want_counts[3] += 1
                want_counts[2] += 1 if want == "clip_bad" else 0
                assert np.array_equal(out["counts"][:, hit], want_counts), name
                assert np.array_equal(out["time"][hit], base["time"][hit] + dt), name
        seen_slots |= set((hit % 16).tolist())
    assert seen_slots == set(range(16))
    _note("malformed_every_slot[%s-%s]" % (plant_kind, which), kinds=len(kinds), legal_oracle=worst)
    plant.close()


@pytest.mark.parametrize("plant_kind", ["ground", "rigid"])
def test_malformed_instances_in_a_closed_loop(plant_kind):
    """20 ticks of closed_loop from a batch with a NaN joint (instance 5), a negative plant_mu (22) and a rate of 1e200 (39, in
    the last wavefront's tail): the plant reports the three on every tick (counts row 3 = 20) and leaves their q and v alone,
    everybody else ends as in the clean loop, bit for bit.  The controller reports (status 2) the two whose damage it is given;
    the plant's friction never reaches it."""
    import torch
    from quadruped_drake_amd import GroundContactPlant, IDController, RigidContactPlant, closed_loop
    n, steps, dt = 43, 20, 1e-3
    ground = plant_kind == "ground"
    q0, v0, t0 = pe.trot_ground_start(n, 13)
    traj = _trot_traj()
    mu_p = np.random.default_rng(14).uniform(0.3, 1.0, n)
    plant = GroundContactPlant("mini_cheetah", device=0) if ground else RigidContactPlant("mini_cheetah", device=0)
    res = {}
    for dirty in (False, True):
        qs, vs, mus = q0.copy(), v0.copy(), mu_p.copy()
        if dirty:
            qs[7 + 4, 5] = np.nan; mus[22] = -0.5; vs[0, 39] = 1e200
        ctrl = IDController(max_batch=n, device=0)
        q, v, tm = _t(qs), _t(vs), _t(t0)
        counts = torch.zeros((4, n), dtype=torch.int32, device=DEV)
        out = closed_loop(ctrl, plant, traj, steps, dt, q, v, tm, plant_mu=_t(mus), counts=counts)
        _sync()
        res[dirty] = dict(q=_h(q), v=_h(v), time=_h(tm), counts=_h(counts), tau=_h(out[0]), status=_h(out[2]), force=_h(out[5]),
                          flags=_h(out[6]), start=(qs, vs))
        ctrl.close()
    bad = np.zeros(n, bool); bad[[5, 22, 39]] = True
    c, d = res[False], res[True]
    assert (c["counts"][3] == 0).all()
    assert np.array_equal(d["counts"][3], np.where(bad, steps, 0))
    assert pe.same_bits(d["q"][:, bad], d["start"][0][:, bad]) and pe.same_bits(d["v"][:, bad], d["start"][1][:, bad])
    for k in ("q", "v", "counts", "tau", "status", "force", "flags"):
        assert pe.same_bits(d[k][..., ~bad], c[k][..., ~bad]), k
    assert np.array_equal(d["time"], c["time"])                          # time advances for everybody
    assert (d["flags"][bad] == pe.BAD).all() and (d["force"][:, bad] == 0).all()
    assert d["status"][5] == 2 and d["status"][39] == 2
    assert (d["tau"][:, [5, 39]] == 0).all() and np.isfinite(d["tau"]).all()
    assert not pe.same_bits(c["q"], c["start"][0])
    plant.close()
