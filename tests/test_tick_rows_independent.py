"""The two equality rows every law's QP contains, asserted on what the tick returns, with INDEPENDENT rigid-body terms.

Every law (ID, MPTC, PC, CLF) solves for x = [vd; tau; f] under (inverse_dynamics_controller.py:48-101 == mptc_controller.py:70-123)

    M vd + Cv + tau_g = S' tau + J_c' f          (dynamics)
    J_c vd + Jdot_c v = -Kd_contact J_c v        (stance feet do not accelerate, with damping)

The tick returns tau and, on request, vd.  Here M, Cv, tau_g, J_c and Jdot_c v come from tests/energy_model.py (closed form, plain FK
and Kane projection, trunk scale from include/wbc.h's sentence): no number of oracle/ and none of the kernels' CRBA / RNEA enters.
  * dynamics: r = M_e vd + Cv_e + tau_g,e - S' tau must lie in range(J_c,e'): the least-squares f over the stance feet is taken
    out and the remainder tested (with no stance foot, r itself).  f is not an output of the tick, and any f is allowed: the cone
    is the QP's business, the row is the physics'.
  * contact: J_c,e vd + (Jdot v)_e + Kd_contact J_c,e v on the stance feet.
  * both residuals are max-norms divided by 1 + max(|M_e vd|, |Cv_e|, |tau_g,e|, |tau|) of the instance.
A wrong velocity-product term, a wrong trunk scale or a wrong Jdot v in the kernels leaves a residual of the size of the term
(1e-3 .. 1); a term that oracle/ and the kernels have wrong in the same way does too, which no parity test can see.

Bar: 100 x the residual that the double oracle's own (tau, vd) leaves in the same independent rows on the same instances, but not
below IND_TOL = 1e-7, at which the project already holds vd (tests/test_reference_law.py); the oracle's own residual must itself
stay under IND_TOL, or the bar would follow a term that is wrong on both sides.  Measured on the CPU batches below
(configs 2, 3, 4, 5 at 48 instances, the 16 masks twice and ANYmal under a trunk scale of 0.5 .. 2.0, all four laws): the oracle leaves at most 2.5e-14 in the dynamics row and
5.2e-15 in the contact row, so 100 x that is 2.5e-12 and the bar is IND_TOL in every case; the host instantiation of the kernel
math leaves at most 1.6e-14 and 1.4e-15.  The -m gpu tests form their bar the same way, from the oracle's residual on their own
256-instance samples, and print their figures; measured on an MI355X (configs 3, 5 and the scaled ANYmal at N = 4096, four laws, and MPTC
with the torque box): oracle at most 3.0e-14 / 7.4e-15, so the bar is IND_TOL again; the HIP kernels leave at most 1.2e-14 / 1.9e-15."""
import functools

import numpy as np
import pytest

import energy_model as em
from oracle import oracle_py as orc
from quadruped_drake_amd import load_model, workloads

IND_TOL = 1e-7
LAWS = ["id", "mptc", "pc", "clf"]


@functools.lru_cache(maxsize=None)
def _table(model):
    return em.load(model)


def indep_terms(model, q, v, s):
    """(M, Cv, tau_g, [J_c], [Jdot_c v]) of one instance from the independent model; one FK pass."""
    t = _table(model)
    M, Cv, tg = em.dynamics_exact(t, q, v, s)
    ft = em.foot_terms_exact(t, q, v)
    return M, Cv, tg, [f[1] for f in ft], [f[3] for f in ft]


def row_residuals(terms, v, mask, tau, vd, kd, act_perm):
    """(dynamics, contact) residuals of one instance, scaled as the module docstring says."""
    M, Cv, tg, J, Jdv = terms
    gen = np.zeros(18)
    for k in range(12):
        gen[6 + act_perm[k]] += tau[k]
    Mvd = M @ vd
    r = Mvd + Cv + tg - gen
    scale = 1.0 + max(np.abs(Mvd).max(), np.abs(Cv).max(), np.abs(tg).max(), np.abs(tau).max())
    feet = [c for c in range(4) if (int(mask) >> c) & 1]
    if not feet:
        return np.abs(r).max() / scale, 0.0
    Jc = np.vstack([J[c] for c in feet])
    f = np.linalg.lstsq(Jc.T, r, rcond=None)[0]
    con = Jc @ vd + np.concatenate([Jdv[c] for c in feet]) + kd * (Jc @ v)
    return np.abs(r - Jc.T @ f).max() / scale, np.abs(con).max() / scale


def batch_terms(b, idx):
    ms = b.get("mass_scale")
    return [indep_terms(b["model"], b["q"][:, i], b["v"][:, i], 1.0 if ms is None else float(ms[i])) for i in idx]


def oracle_residuals(kind, b, idx, terms, tau_max=None):
    """Worst residuals the double oracle's own (tau, x[:18]) leaves in the independent rows; its status per instance."""
    p = orc.params(kind)
    if tau_max is not None:
        p.tau_max = tau_max
    act = list(load_model(b["model"]).get("act_perm", range(12)))
    worst = np.zeros(2); st = np.zeros(len(idx), np.int32)
    for j, i in enumerate(idx):
        m = orc.model(b["model"]) if b.get("mass_scale") is None else orc.model_scaled(b["model"], float(b["mass_scale"][i]))
        if b.get("mu") is not None:
            p.mu = float(b["mu"][i])
        ct = [(int(b["mask"][i]) >> k) & 1 for k in range(4)]
        tau, _, st[j], qp = orc.control_law(kind, m, p, b["q"][:, i], b["v"][:, i], b["targets"][:, i], ct, want_qp=True)
        if st[j] == 0:
            worst = np.maximum(worst, row_residuals(terms[j], b["v"][:, i], b["mask"][i], tau, qp["x"][:18], p.Kd_contact, act))
    return worst, st


def check(kind, b, idx, terms, tau, vd, ok, tau_max=None, label=""):
    """tau [12, len(idx)], vd [18, len(idx)]: the tick's outputs for the instances idx; ok: which of them to hold to the bar."""
    kd = orc.params(kind).Kd_contact
    act = list(load_model(b["model"]).get("act_perm", range(12)))
    res = np.array([row_residuals(terms[j], b["v"][:, i], b["mask"][i], tau[:, j], vd[:, j], kd, act) if ok[j] else (0.0, 0.0)
                    for j, i in enumerate(idx)])
    o_worst, o_st = oracle_residuals(kind, b, idx, terms, tau_max)
    bar = np.maximum(100.0 * o_worst, IND_TOL)
    print("%s %-4s n=%d  dynamics row: tick %.1e  oracle %.1e  bar %.1e | contact row: tick %.1e  oracle %.1e  bar %.1e" %
          (label, kind, int(np.sum(ok)), res[:, 0].max(), o_worst[0], bar[0], res[:, 1].max(), o_worst[1], bar[1]))
    assert np.array_equal(o_st == 0, np.asarray(ok, bool))          # the oracle answers the same instances
    # the oracle's residual is a rounding level only while the oracle itself is right: it is held to the same rows, so that a term
    # wrong in oracle/ and in the kernels alike cannot raise the bar it is measured against
    assert (o_worst <= IND_TOL).all(), (kind, label, o_worst)
    assert res[:, 0].max() <= bar[0], (kind, label, int(res[:, 0].argmax()), res[:, 0].max())
    assert res[:, 1].max() <= bar[1], (kind, label, int(res[:, 1].argmax()), res[:, 1].max())
    return res


# ---- CPU: the host instantiation of the kernel math (16-lane mapping)
N_CPU = 48


def _scaled_anymal(n):
    """Config 4 with a trunk scale of 0.5 .. 2.0 and mu of 0.4 .. 1.0.  ANYmal's trunk has its CoM off the link origin (Mini
    Cheetah's, the robot of config 5, has not), so only here does it matter about which point the trunk inertia is scaled."""
    b = workloads.make_batch(4, n=n)
    rng = np.random.default_rng(404)
    b["mu"] = rng.uniform(0.4, 1.0, n); b["mass_scale"] = rng.uniform(0.5, 2.0, n)
    return b


@functools.lru_cache(maxsize=None)
def _cpu_batch(cfg):
    if cfg == "masks16":
        b = workloads.make_batch(3, n=32, seed=77)
        b["mask"] = (np.arange(32) % 16).astype(np.uint8)
    elif cfg == "4scaled":
        b = _scaled_anymal(N_CPU)
    else:
        b = workloads.make_batch(cfg, n=N_CPU)
    idx = np.arange(b["q"].shape[1])
    return b, idx, batch_terms(b, idx)


@pytest.mark.parametrize("cfg", [2, 3, 4, 5, "masks16", "4scaled"])
@pytest.mark.parametrize("kind", LAWS)
def test_host_tick_satisfies_the_independent_rows(kind, cfg):
    import host_tick as ht
    b, idx, terms = _cpu_batch(cfg)
    flat = np.array(load_model(b["model"])["flat"])
    tau, met, st, it, vd = ht.run(kind, flat, b["q"], b["v"], b["targets"], b["mask"], b["mu"], b["mass_scale"], hexv=True,
                                  want_vdot=True)
    assert (st == 0).all()                     # nobody is left out
    check(kind, b, idx, terms, tau, vd, st == 0, label="host cfg %s" % cfg)


def test_the_rows_see_a_wrong_term():
    """The check itself: the same outputs against independent terms with one defect each fail the bar by orders of magnitude."""
    import host_tick as ht
    b, idx, terms = _cpu_batch(5)
    flat = np.array(load_model(b["model"])["flat"])
    tau, met, st, it, vd = ht.run("mptc", flat, b["q"], b["v"], b["targets"], b["mask"], b["mu"], b["mass_scale"], hexv=True,
                                  want_vdot=True)
    kd = orc.params("mptc").Kd_contact
    worst = lambda tt: np.array([row_residuals(tt[j], b["v"][:, i], b["mask"][i], tau[:, j], vd[:, j], kd, list(range(12)))
                                 for j, i in enumerate(idx)]).max(0)
    assert (worst(terms) < IND_TOL).all()
    no_scale = [indep_terms(b["model"], b["q"][:, i], b["v"][:, i], 1.0) for i in idx]
    assert worst(no_scale)[0] > 1e4 * IND_TOL
    half_cv = [(M, 0.5 * Cv, tg, J, Jdv) for M, Cv, tg, J, Jdv in terms]
    assert worst(half_cv)[0] > 1e3 * IND_TOL
    no_jdv = [(M, Cv, tg, J, [0 * x for x in Jdv]) for M, Cv, tg, J, Jdv in terms]
    assert worst(no_jdv)[1] > 1e4 * IND_TOL


# ---- GPU: the HIP kernels through the C ABI
def _gpu_tick(kind, b, params=None):
    import torch
    from quadruped_drake_amd import IDController, MPTCController, PCController, CLFController
    cls = {"id": IDController, "mptc": MPTCController, "pc": PCController, "clf": CLFController}[kind]
    n = b["q"].shape[1]
    ctrl = cls(model=b["model"], max_batch=n, device=0, params=params)
    up = lambda x: None if x is None else torch.tensor(np.ascontiguousarray(x), device="cuda:0")
    vd = torch.zeros((18, n), dtype=torch.float64, device="cuda:0")
    ctrl.set_vdot_output(vd)
    tau, met, st = ctrl.step(up(b["q"]), up(b["v"]), up(b["targets"]), up(b["mask"]), up(b["mu"]), up(b["mass_scale"]))
    ctrl.sync()
    out = tau.cpu().numpy(), st.cpu().numpy(), vd.cpu().numpy()
    ctrl.close()
    return out


@functools.lru_cache(maxsize=None)
def _gpu_batch(cfg):
    b = _scaled_anymal(4096) if cfg == "4scaled" else workloads.make_batch(cfg, n=4096)
    idx = np.random.default_rng(11).choice(4096, 256, replace=False)
    return b, idx, batch_terms(b, idx)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [3, 5, "4scaled"])
@pytest.mark.parametrize("kind", LAWS)
def test_hip_tick_satisfies_the_independent_rows(kind, cfg):
    b, idx, terms = _gpu_batch(cfg)
    tau, st, vd = _gpu_tick(kind, b)
    assert (st == 0).all()
    check(kind, b, idx, terms, tau[:, idx], vd[:, idx], st[idx] == 0, label="hip cfg %s" % cfg)


@pytest.mark.gpu
def test_hip_tick_with_the_torque_box_satisfies_the_independent_rows():
    """tau_max = 10 on the config-3 trots under MPTC (test_torque_box's case): the dynamics row holds with the clamped torques."""
    b, idx, terms = _gpu_batch(3)
    tm = 10.0
    tau, st, vd = _gpu_tick("mptc", b, params={"tau_max": tm})
    ok = st[idx] == 0
    assert ok.sum() > 200                                                   # a box can be infeasible for violent states
    assert (np.abs(np.abs(tau[:, idx][:, ok]) - tm) < 1e-6).sum() > 50       # the box binds on the sample
    assert np.abs(tau[:, idx][:, ok]).max() <= tm + 1e-9
    check("mptc", b, idx, terms, tau[:, idx], vd[:, idx], ok, tau_max=tm, label="hip cfg 3 box")
