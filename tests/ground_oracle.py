"""Dense numpy restatement of the compliant-ground plant (include/wbc_ground.h) -- test infrastructure.

Shares no algorithm with the arrowhead elimination of csrc/wbc_ground.hpp: M, Cv, tau_g come from the C oracle's inverse-dynamics
passes (oracle_py.calc_dynamics of the trunk-scaled model), the feet's positions and Jacobians from oracle_py.foot_quantities, the
force law is restated here from the header's sentence, and the full 18x18 system is solved with np.linalg.solve.  The integration
is traj_oracle.integrate.  Joint rows in canonical order (q_perm = identity); torques in actuator order through act_perm.

backend="energy" takes the same terms from tests/energy_model.py instead (closed form from plain FK and Kane projection, trunk
scale included): no number of oracle/ enters, only the model table and traj_oracle's integrator."""
import math

import numpy as np

import energy_model as em
from oracle import oracle_py as orc
from oracle import traj_oracle

SLIP, FELL, CLIP, BAD = 1, 2, 4, 8
DELTA = 1e-3


def _table(model):
    return em.load(model) if isinstance(model, str) else model


def defaults(model):
    """The default parameters: k = weight (s_p = 1) / 1 mm, d = 1 / sqrt(g 1 mm), mu 1.0, v_s 0.05 m/s, substeps of at most 0.0625 ms."""
    t = _table(model)
    g = t["gravity"]
    w = (t["base"]["mass"] + sum(L["mass"] for leg in t["legs"] for L in leg["links"])) * g
    return dict(stiffness=w / DELTA, dissipation=1.0 / math.sqrt(g * DELTA), mu=1.0, v_stiction=0.05, foot_radius=0.0,
                tau_max=math.inf, max_substep=6.25e-5, fall_height=0.0)


def params(model, over=None):
    p = defaults(model)
    p.update(over or {})
    return p


def substeps(dt, max_substep):
    return max(1, int(math.ceil(dt / max_substep * (1.0 - 1e-12))))


def terms(model, q, v, s_p, backend):
    """(M, Cv, tau_g, [(p_c, J_c)] x 4, act_perm) of the trunk-scaled model from the chosen backend."""
    if backend == "oracle":
        m = orc.model_scaled(model, s_p)
        M, Cv, tg = orc.calc_dynamics(m, q, v)
        return M, Cv, tg, [orc.foot_quantities(m, q, v, c)[:2] for c in range(4)], list(m.act_perm)
    assert backend == "energy"
    t = _table(model)
    M, Cv, tg = em.dynamics_exact(t, q, v, s_p)
    ft = em.foot_terms_exact(t, q, v)
    return M, Cv, tg, [(ft[c][0], ft[c][1]) for c in range(4)], list(t.get("act_perm", range(12)))


def foot_force(P, mu, p, pd):
    """-> (f[3], touching, loaded and sliding faster than v_s)"""
    phi = P["foot_radius"] - p[2]
    if not phi > 0:
        return np.zeros(3), False, False
    fn = P["stiffness"] * phi * max(0.0, 1.0 - P["dissipation"] * pd[2])
    vt = math.hypot(pd[0], pd[1])
    ft = -mu * fn * pd[:2] / max(vt, P["v_stiction"])
    return np.array([ft[0], ft[1], fn]), True, bool(fn > 0 and vt > P["v_stiction"])


def forward_one(model, q, v, tau, mu=None, s_p=1.0, wext=None, P=None, backend="oracle", detail=False):
    """One instance -> (vdot[18], force[12], contact bits, flags)."""
    P = params(model) if P is None else P
    mu = P["mu"] if mu is None else mu
    q = np.asarray(q, float); v = np.asarray(v, float); tau = np.asarray(tau, float)
    wext = np.zeros(6) if wext is None else np.asarray(wext, float)
    flags = 0
    if np.any(np.abs(tau) > P["tau_max"] * (1 + 1e-9)):
        flags |= CLIP
    if (not np.all(np.isfinite(q)) or not np.all(np.isfinite(v)) or not np.all(np.isfinite(tau)) or not np.all(np.isfinite(wext))
            or not (np.isfinite(mu) and mu > 0) or not (np.isfinite(s_p) and s_p > 0)):
        return np.zeros(18), np.zeros(12), 0, flags | BAD
    ta = np.clip(tau, -P["tau_max"], P["tau_max"])
    M, Cv, tg, feet, act_perm = terms(model, q, v, s_p, backend)
    gen = np.zeros(18)
    for k in range(12):
        gen[6 + act_perm[k]] += ta[k]
    gen[:6] += wext
    f = np.zeros(12); contact = 0; slip = False
    for c, (p, J) in enumerate(feet):
        fc, touch, sl = foot_force(P, mu, p, J @ v)
        f[3 * c:3 * c + 3] = fc
        gen += J.T @ fc
        contact |= int(touch) << c
        slip |= sl
    vd = np.linalg.solve(M, gen - Cv - tg)
    if not np.all(np.isfinite(vd)):
        return np.zeros(18), np.zeros(12), 0, flags | BAD
    flags |= (SLIP if slip else 0) | (FELL if not q[6] > P["fall_height"] else 0)
    return vd, f, contact, flags


def forward(model, q, v, tau, mu=None, mass_scale=None, ext_wrench=None, P=None, idx=None, backend="oracle"):
    """SoA batch (q[19, N] ...) -> vdot[18, N'], force[12, N'], contact[N'], flags[N'] for the instances `idx` (default all)."""
    n = q.shape[1]
    idx = np.arange(n) if idx is None else np.asarray(idx)
    vd = np.zeros((18, idx.size)); f = np.zeros((12, idx.size)); ct = np.zeros(idx.size, np.uint8); fl = np.zeros(idx.size, np.int32)
    for j, i in enumerate(idx):
        vd[:, j], f[:, j], ct[j], fl[j] = forward_one(model, q[:, i], v[:, i], tau[:, i], None if mu is None else mu[i],
                                                       1.0 if mass_scale is None else mass_scale[i],
                                                       None if ext_wrench is None else ext_wrench[:, i], P, backend)
    return vd, f, ct, fl


def step(model, q, v, tau, dt, n_sub, mu=None, mass_scale=None, ext_wrench=None, P=None, backend="oracle"):
    """`n_sub` explicit substeps of dt / n_sub.  -> (q+, v+, mean force, contact of the last substep, flags); a BAD instance keeps
    its state and gets zero force.  FELL is judged on the end state, SLIP over all substeps."""
    P = params(model) if P is None else P
    q0 = np.array(q, float); v0 = np.array(v, float)
    qn, vn = q0.copy(), v0.copy()
    n = q0.shape[1]
    fsum = np.zeros((12, n)); ct = np.zeros(n, np.uint8); fl = np.zeros(n, np.int32)
    h = dt / n_sub
    for _ in range(n_sub):
        vd, f, ct, fs = forward(model, qn, vn, tau, mu, mass_scale, ext_wrench, P, backend=backend)
        fl |= fs & ~np.int32(FELL)
        fsum += f
        qn, vn = traj_oracle.integrate(qn, vn, vd, h)
    bad = ((fl & BAD) != 0) | ~np.isfinite(qn).all(0) | ~np.isfinite(vn).all(0)
    fl[~bad & ~(qn[6] > P["fall_height"])] |= FELL
    fl[bad] = (fl[bad] & CLIP) | BAD
    qn[:, bad] = q0[:, bad]; vn[:, bad] = v0[:, bad]
    fsum[:, bad] = 0; ct[bad] = 0
    return qn, vn, fsum / n_sub, ct, fl


def margin(model, q, v, tau, mu=None, s_p=1.0, P=None, backend="oracle"):
    """Smallest relative distance of one instance to a flag or contact threshold (for excluding borderline draws): foot height
    against the contact plane (per metre of the trunk height's scale, 1 m), sliding speed against v_s, the damping factor against
    0, trunk height against fall_height and torques against tau_max."""
    P = params(model) if P is None else P
    q = np.asarray(q, float); v = np.asarray(v, float)
    _, _, _, feet, _ = terms(model, q, v, s_p, backend)
    d = [abs(q[6] - P["fall_height"])]
    for p, J in feet:
        pd = J @ v
        d.append(abs(P["foot_radius"] - p[2]))
        if P["foot_radius"] - p[2] > 0:
            d.append(abs(math.hypot(pd[0], pd[1]) - P["v_stiction"]) / P["v_stiction"])
            d.append(abs(1.0 - P["dissipation"] * pd[2]))
    if np.isfinite(P["tau_max"]):
        d.append(float(np.min(np.abs(np.abs(tau) - P["tau_max"]))) / P["tau_max"])
    return min(d)


# ---- test states
def _feet_z(table, q):
    """Heights of the four feet of one instance (the C oracle's kinematics: only used to place the draws)."""
    m = orc.model(table)
    z0 = np.zeros(18)
    return np.array([orc.foot_quantities(m, q, z0, c)[0][2] for c in range(4)])


def draw(cfg, n, seed):
    """Random states of BASELINE config `cfg` with the base height shifted so that, instance by instance, the lowest, second, third
    or highest foot sits within -1 .. +2 mm of penetration: feet in contact and feet clear of the ground in every mix."""
    from quadruped_drake_amd import load_model, workloads
    b = workloads.make_batch(cfg, n=n, seed=seed)
    t = load_model(b["model"])
    rng = np.random.default_rng(seed + 7)
    q, v = b["q"].copy(), b["v"].copy()
    for i in range(n):
        z = np.sort(_feet_z(t, q[:, i]))
        q[6, i] -= z[i % 4] + rng.uniform(-1e-3, 2e-3)
    tau = rng.uniform(-30.0, 30.0, (12, n))
    sp = rng.uniform(0.8, 1.2, n)
    we = rng.normal(0.0, 5.0, (6, n))
    return t, q, v, tau, sp, we


def draw_near_stance(model, n, seed):
    """States for multi-substep comparisons: the reference's stance with joints perturbed by +-2 mrad, small velocities, and the
    base set so that the lowest, second, third or highest foot sits within -0.5 .. +1 mm of penetration.  Deeper feet are left to
    the single-evaluation tests: with the Hunt-Crossley damping k phi d on the foot's small effective mass, an explicit substep
    of 125 us amplifies a perturbation at ANYmal's foot once phi exceeds ~1 mm, and rounding differences between two correct
    implementations then grow past any fixed tolerance within eight substeps."""
    from quadruped_drake_amd import load_model, workloads
    t = load_model(model)
    rng = np.random.default_rng(seed)
    q, v = workloads.nominal_state(model, n)
    q[7:] += rng.uniform(-2e-3, 2e-3, (12, n))
    q[0:4] += np.vstack([np.zeros(n), rng.normal(0.0, 2e-3, (3, n))])
    q[0:4] /= np.sqrt((q[0:4] ** 2).sum(0))
    v = rng.normal(0.0, 0.02, (18, n))
    for i in range(n):
        z = np.sort(_feet_z(t, q[:, i]))
        q[6, i] -= z[i % 4] + rng.uniform(-0.5e-3, 1e-3)
    tau = rng.uniform(-10.0, 10.0, (12, n))
    return t, q, v, tau, rng.uniform(0.8, 1.2, n), rng.normal(0.0, 5.0, (6, n))


# ---- the drop-and-rest experiment (tools/ground_sweep.py, tests/test_ground_cpu.py): a robot under a joint PD dropped from 5 mm
PD_GAINS = {"mini_cheetah": (300.0, 6.0), "anymal_b": (1800.0, 24.0)}


def feet_positions(table, q):
    """World positions [4, 3] of the feet of one instance (tests/energy_model.py)."""
    return np.array([f["p"] for f in em.bodies(table, q)[1]])


def drop_state(model, height=5e-3, n=1):
    """(model table, q, v): the reference's initial state with the base set so that the lowest foot is `height` above the ground."""
    from quadruped_drake_amd import load_model, workloads
    t = load_model(model)
    q, v = workloads.nominal_state(model, n)
    q[6] -= feet_positions(t, q[:, 0])[:, 2].min() - height
    return t, q, v


def pd_torque(table, model, q, v, q_ref):
    """Joint PD towards q_ref in actuator order, [12, N]."""
    kp, kd = PD_GAINS[model]
    gen = kp * (q_ref[7:] - q[7:]) - kd * v[6:]
    tau = np.zeros_like(gen)
    for k, j in enumerate(table.get("act_perm", range(12))):
        tau[k] = gen[j]
    return tau


def drop_test(model, engine="host", h=None, v_s=None, seconds=1.0, over=None):
    """Drop from 5 mm under the joint PD, the PD recomputed at every substep (the plant is stepped with dt = h, one substep per
    call: held over 1 ms this PD is itself unstable on Mini Cheetah's light shanks).  h None: the default max_substep.
    engine: "host" (tests/host_ground.py) or a backend of this file.
    -> dict(max_abs_v of the end state, load_error = mean(sum f_z) / weight - 1 over the last 0.1 s, finite, height)."""
    import host_ground as hg
    t, q, v = drop_state(model)
    q_ref = q.copy()
    over = dict(over or {})
    if v_s is not None:
        over["v_stiction"] = v_s
    P = params(t, over)
    h = P["max_substep"] if h is None else h
    weight = P["stiffness"] * DELTA
    steps = int(round(seconds / h))
    tail = int(round(0.1 / h))
    fz = []
    for k in range(steps):
        tau = pd_torque(t, model, q, v, q_ref)
        if engine == "host":
            o = hg.run(t["flat"], q, v, tau, params=over, act_perm=t.get("act_perm"), dt=h, substeps=1)
            q, v, f, fl = o["q"], o["v"], o["force"], o["flags"]
        else:
            q, v, f, _, fl = step(t, q, v, tau, h, 1, P=P, backend=engine)
        if fl[0] & BAD or not np.isfinite(q).all() or np.abs(v).max() > 1e3:
            return dict(max_abs_v=float("inf"), load_error=float("inf"), finite=False, height=float("nan"))
        if k >= steps - tail:
            fz.append(f[2::3, 0].sum())
    return dict(max_abs_v=float(np.abs(v).max()), load_error=float(np.mean(fz) / weight - 1.0), finite=True, height=float(q[6, 0]))
