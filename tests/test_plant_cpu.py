"""Rigid-contact plant step (include/wbc_plant.h), no GPU: the host instantiation of csrc/wbc_plant.hpp against the dense numpy
plant (tests/plant_oracle.py), and the argument checks of the C ABI that return before any device is touched.  The dense plant
runs over both of its backends at the same tolerances: "oracle" (terms of oracle/) and "energy" (closed-form terms of
tests/energy_model.py, trunk scale included; nothing of oracle/ in the loop)."""
import ctypes as C

import numpy as np
import pytest

import host_plant as hp
import plant_oracle as po
from quadruped_drake_amd import load_model, workloads

MODELS = [(3, "mini_cheetah"), (4, "anymal_b")]
BACKENDS = ["oracle", "energy"]


def _draw(cfg, n, seed):
    b = workloads.make_batch(cfg, n=n, seed=seed)
    rng = np.random.default_rng(seed + 7)
    tau = rng.uniform(-30.0, 30.0, (12, n))
    mask = (np.arange(n) % 16).astype(np.uint8)           # every mask, 16 instances each at n = 256
    sp = rng.uniform(0.8, 1.2, n)
    return b, tau, mask, sp


def _rel(a, b):
    return np.abs(a - b).max() / (1.0 + np.abs(b).max())


@pytest.mark.parametrize("cfg,model", MODELS)
def test_host_plant_matches_dense_oracle(cfg, model):
    n = 256
    b, tau, mask, sp = _draw(cfg, n, 11)
    t = load_model(model)
    out = hp.run(t["flat"], b["q"], b["v"], tau, mask, mass_scale=sp, act_perm=t.get("act_perm"))
    for backend in BACKENDS:
        vd, f, fl = po.forward(t, b["q"], b["v"], tau, mask, mass_scale=sp, backend=backend)
        assert _rel(out["vdot"], vd) < 1e-10, backend
        assert _rel(out["force"], f) < 1e-10, backend
        # the draws left out of the flag comparison are chosen by this backend alone, and stay within the cap
        keep = np.array([po.margin(t, b["q"][:, i], b["v"][:, i], tau[:, i], int(mask[i]), 1.0, sp[i], backend=backend) > 1e-6
                         for i in range(n)])
        assert keep.sum() > 0.9 * n, backend
        assert (out["flags"][keep] == fl[keep]).all(), backend
        assert ((fl & (po.PULL | po.CONE)) != 0).any() and ((fl & (po.PULL | po.CONE)) == 0).any()   # both outcomes are exercised
    assert (out["force"][np.repeat(((mask[None, :] >> np.arange(4)[:, None]) & 1) == 0, 3, axis=0)] == 0).all()   # swing feet: 0


@pytest.mark.parametrize("cfg,model", MODELS)
def test_host_plant_step_matches_dense_oracle(cfg, model):
    n = 64
    b, tau, mask, sp = _draw(cfg, n, 12)
    t = load_model(model)
    time = np.linspace(0.0, 1.0, n); counts = np.zeros((4, n), np.int32)
    out = hp.run(t["flat"], b["q"], b["v"], tau, mask, mass_scale=sp, act_perm=t.get("act_perm"), dt=2e-3, time=time, counts=counts)
    for backend in BACKENDS:
        qn, vn, vd, f, fl = po.step(t, b["q"], b["v"], tau, mask, 2e-3, mass_scale=sp, backend=backend)
        assert _rel(out["q"], qn) < 1e-12 and _rel(out["v"], vn) < 1e-10, backend
    assert np.array_equal(out["time"], time + 2e-3)
    for bit in range(4):
        assert np.array_equal(out["counts"][bit], (out["flags"] >> bit) & 1)


def test_straight_stance_knee_is_answered():
    t = load_model("mini_cheetah")
    q, v = workloads.nominal_state("mini_cheetah", 4)
    rng = np.random.default_rng(3)
    v = rng.normal(0.0, 0.3, v.shape)
    q[7 + 2] = 0.0          # LF knee exactly straight, in stance on every instance
    q[7 + 8] = 0.0          # LH knee too
    tau = rng.uniform(-20.0, 20.0, (12, 4))
    mask = np.array([0b1111, 0b0101, 0b0001, 0b1001], np.uint8)
    out = hp.run(t["flat"], q, v, tau, mask, act_perm=t.get("act_perm"))
    assert (out["flags"] & po.BAD == 0).all()
    assert np.isfinite(out["vdot"]).all() and np.isfinite(out["force"]).all()
    for backend in BACKENDS:
        vd, f, fl = po.forward(t, q, v, tau, mask, backend=backend)
        assert _rel(out["vdot"], vd) < 1e-8 and _rel(out["force"], f) < 1e-8, backend


def test_non_finite_input_is_bad_and_leaves_state():
    t = load_model("mini_cheetah")
    b, tau, mask, sp = _draw(3, 6, 5)
    q, v = b["q"].copy(), b["v"].copy()
    q[9, 0] = np.nan; v[3, 1] = np.inf; tau[5, 2] = np.nan
    mu = np.array([1.0, 1.0, 1.0, -0.5, 1.0, 1.0]); sp[4] = np.inf
    out = hp.run(t["flat"], q, v, tau, mask, mu=mu, mass_scale=sp, act_perm=t.get("act_perm"), dt=1e-3)
    bad = np.array([1, 1, 1, 1, 1, 0], bool)
    assert np.array_equal((out["flags"] & po.BAD) != 0, bad)
    assert (out["vdot"][:, bad] == 0).all() and (out["force"][:, bad] == 0).all()
    assert np.array_equal(out["q"][:, bad], q[:, bad], equal_nan=True) and np.array_equal(out["v"][:, bad], v[:, bad], equal_nan=True)
    assert not np.array_equal(out["q"][:, 5], q[:, 5])


def test_torque_clipping_against_oracle():
    t = load_model("anymal_b")
    b, tau, mask, sp = _draw(4, 128, 9)
    tm = 20.0
    out = hp.run(t["flat"], b["q"], b["v"], tau, mask, mass_scale=sp, act_perm=t.get("act_perm"), params3=[100.0, tm, 1.0])
    clip = (np.abs(tau) > tm).any(0)
    assert clip.any() and not clip.all()
    assert np.array_equal((out["flags"] & po.CLIP) != 0, clip)
    for backend in BACKENDS:
        vd, f, fl = po.forward(t, b["q"], b["v"], tau, mask, mass_scale=sp, tau_max=tm, backend=backend)
        assert _rel(out["vdot"], vd) < 1e-10 and _rel(out["force"], f) < 1e-10, backend
        # clipping changes the answer: the unclipped dense plant differs
        vd_u, _, _ = po.forward(t, b["q"], b["v"], tau, mask, mass_scale=sp, backend=backend)
        assert _rel(vd_u[:, clip], vd[:, clip]) > 1e-3


# ---- C ABI argument checks that return before any device is touched
def _abi():
    from quadruped_drake_amd import plant
    return plant._L()


def _err(L):
    return L.wbc_last_error().decode()


def test_abi_plant_misuse_without_device():
    from quadruped_drake_amd import plant
    L = _abi()
    P = C.c_void_p(1)   # never dereferenced: the size checks come first
    fwd = lambda h, n, ld: L.wbc_plant_forward(h, None, n, ld, *([P] * 4), None, None, None, None, None)
    assert fwd(None, 4, 4) < 0 and "null plant" in _err(L)
    assert fwd(P, 8, 4) < 0 and "ld must be >= n" in _err(L)
    assert fwd(P, (1 << 23) + 1, (1 << 23) + 1) < 0 and "WBC_MAX_LD" in _err(L)
    st = L.wbc_plant_step(None, None, 4, 4, 1e-3, P, P, None, P, P, None, None, None, None, None, None)
    assert st < 0 and "null plant" in _err(L)
    ro = L.wbc_plant_rollout(None, None, None, None, 1, 1e-3, 4, 4, *([P] * 15))
    assert ro < 0 and "null" in _err(L)
    assert L.wbc_plant_kernel_info(None, None, None, None, None) < 0
    assert L.wbc_plant_params_default(None) < 0
    p = plant.WbcPlantParams()
    assert L.wbc_plant_params_default(C.byref(p)) == 0
    assert (p.Kd_contact, p.tau_max, p.mu) == (100.0, float("inf"), 1.0)
    assert L.wbc_plant_destroy(None) == 0
