"""Dense numpy restatement of the rigid-contact plant step (include/wbc_plant.h) -- test infrastructure.

Shares no algorithm with the arrowhead elimination of csrc/wbc_plant.hpp: M, Cv, tau_g come from the C oracle's inverse-dynamics
passes (oracle_py.calc_dynamics of the trunk-scaled model), J_c and Jdot_c v from oracle_py.foot_quantities, and the full
(18 + 3 nc) KKT system is solved with np.linalg.solve.  The integration is traj_oracle.integrate.  Joint rows in canonical order
(q_perm = identity); torques in actuator order through the model's act_perm.

backend="energy" fills the same KKT system from tests/energy_model.py instead: M, Cv, tau_g, J_c and Jdot_c v in closed form from
plain FK and Kane projection, the trunk scale s_p included (base mass and base inertia about the link origin times s_p, from
include/wbc.h's sentence) -- no number of oracle/ enters, only the model table and traj_oracle's integrator."""
import numpy as np

import energy_model as em
from oracle import oracle_py as orc
from oracle import traj_oracle

PULL, CONE, CLIP, BAD = 1, 2, 4, 8


def _terms(model, q, v, s_p, feet, backend):
    """(M, Cv, tau_g, [(J_c, Jdot_c v)], act_perm, weight) of the trunk-scaled model from the chosen backend."""
    if backend == "oracle":
        m = orc.model_scaled(model, s_p)
        M, Cv, tg = orc.calc_dynamics(m, q, v)
        weight = (m.base_mass + sum(m.link[l][k].mass for l in range(4) for k in range(3))) * m.gravity
        return M, Cv, tg, [orc.foot_quantities(m, q, v, c)[1:] for c in feet], list(m.act_perm), weight
    assert backend == "energy"
    t = em.load(model) if isinstance(model, str) else model
    M, Cv, tg = em.dynamics_exact(t, q, v, s_p)
    ft = em.foot_terms_exact(t, q, v)
    weight = (s_p * t["base"]["mass"] + sum(L["mass"] for leg in t["legs"] for L in leg["links"])) * t["gravity"]
    return M, Cv, tg, [(ft[c][1], ft[c][3]) for c in feet], list(t.get("act_perm", range(12))), weight


def forward_one(model, q, v, tau, mask, mu=1.0, s_p=1.0, kd=100.0, tau_max=np.inf, backend="oracle"):
    """One instance -> (vdot[18], force[12], flags).  model: a name or a model table (dict)."""
    q = np.asarray(q, float); v = np.asarray(v, float); tau = np.asarray(tau, float)
    flags = 0
    if np.any(np.abs(tau) > tau_max * (1 + 1e-9)):
        flags |= CLIP
    if (not np.all(np.isfinite(q)) or not np.all(np.isfinite(v)) or not np.all(np.isfinite(tau))
            or not (np.isfinite(mu) and mu > 0) or not (np.isfinite(s_p) and s_p > 0)):
        return np.zeros(18), np.zeros(12), flags | BAD
    ta = np.clip(tau, -tau_max, tau_max)
    feet = [c for c in range(4) if (mask >> c) & 1]
    M, Cv, tg, foot_terms, act_perm, weight = _terms(model, q, v, s_p, feet, backend)
    gen = np.zeros(18)
    for k in range(12):
        gen[6 + act_perm[k]] += ta[k]
    J = np.zeros((3 * len(feet), 18)); rhs_c = np.zeros(3 * len(feet))
    for j, (Jc, Jdv) in enumerate(foot_terms):
        J[3 * j:3 * j + 3] = Jc
        rhs_c[3 * j:3 * j + 3] = -kd * (Jc @ v) - Jdv
    nc = 3 * len(feet)
    K = np.zeros((18 + nc, 18 + nc))
    K[:18, :18] = M; K[:18, 18:] = -J.T; K[18:, :18] = J
    x = np.linalg.solve(K, np.concatenate([gen - Cv - tg, rhs_c]))
    vd = x[:18]
    f = np.zeros(12)
    for j, c in enumerate(feet):
        f[3 * c:3 * c + 3] = x[18 + 3 * j:21 + 3 * j]
    tol = 1e-9 * (sum(np.abs(f[3 * c:3 * c + 3]).sum() for c in feet) + weight)
    for c in feet:
        fx, fy, fz = f[3 * c:3 * c + 3]
        if fz < -tol:
            flags |= PULL
        if abs(fx) > mu * fz + tol or abs(fy) > mu * fz + tol:
            flags |= CONE
    return vd, f, flags


def forward(model, q, v, tau, mask, mu=None, mass_scale=None, kd=100.0, tau_max=np.inf, mu0=1.0, idx=None, backend="oracle"):
    """SoA batch (q[19, N] ...) -> vdot[18, N'], force[12, N'], flags[N'] for the instances `idx` (default all)."""
    n = q.shape[1]
    idx = np.arange(n) if idx is None else np.asarray(idx)
    vd = np.zeros((18, idx.size)); f = np.zeros((12, idx.size)); fl = np.zeros(idx.size, np.int32)
    for j, i in enumerate(idx):
        vd[:, j], f[:, j], fl[j] = forward_one(model, q[:, i], v[:, i], tau[:, i], int(mask[i]),
                                               mu0 if mu is None else mu[i], 1.0 if mass_scale is None else mass_scale[i], kd, tau_max, backend)
    return vd, f, fl


def step(model, q, v, tau, mask, dt, **kw):
    """forward + traj_oracle.integrate; a BAD instance keeps its state.  -> (q+, v+, vdot, force, flags)"""
    vd, f, fl = forward(model, q, v, tau, mask, **kw)
    qn, vn = traj_oracle.integrate(q, v, vd, dt)
    bad = (fl & BAD) != 0
    qn[:, bad] = q[:, bad]; vn[:, bad] = v[:, bad]
    return qn, vn, vd, f, fl


def margin(model, q, v, tau, mask, mu=1.0, s_p=1.0, kd=100.0, tau_max=np.inf, backend="oracle"):
    """Smallest relative distance of one instance's forces / torques to a flag threshold (for excluding borderline draws)."""
    vd, f, fl = forward_one(model, q, v, tau, mask, mu, s_p, kd, tau_max, backend)
    d = [np.inf]
    s = sum(np.abs(f[3 * c:3 * c + 3]).sum() for c in range(4) if (mask >> c) & 1) + 1e-300
    for c in range(4):
        if (mask >> c) & 1:
            fx, fy, fz = f[3 * c:3 * c + 3]
            d += [abs(fz) / s, abs(mu * fz - abs(fx)) / s, abs(mu * fz - abs(fy)) / s]
    if np.isfinite(tau_max):
        d.append(float(np.min(np.abs(np.abs(tau) - tau_max))) / tau_max)
    return min(d)
