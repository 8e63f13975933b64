"""Terrain of the compliant-ground plant (include/wbc_ground.h), no GPU: the host instantiation of csrc/wbc_ground.hpp with its
TERRAIN force law (tests/host_terrain.py) against the dense numpy plant (tests/terrain_oracle.py) over both of its backends, exact
relations that need no oracle, the physics of a slope, a swing foot against a riser, and the argument checks of the C ABI that
return before any device is touched."""
import ctypes as C
import math

import numpy as np
import pytest

import ground_oracle as go
import host_ground as hg
import host_terrain as ht
import plant_edges as pe
import terrain_oracle as to
from quadruped_drake_amd import terrain as tr

MODELS = [(3, "mini_cheetah"), (4, "anymal_b")]
BACKENDS = ["oracle", "energy"]


def _rel(a, b):
    return np.abs(a - b).max() / (1.0 + np.abs(b).max())


def _keep(t, q, v, tau, sp, profiles, tid, tsc, backend):
    return np.array([to.margin(t, q[:, i], v[:, i], tau[:, i], profiles[tid[i]], tsc[i], s_p=sp[i], backend=backend) > 1e-6
                     for i in range(q.shape[1])])


def _segments(profiles, reach=0.4):
    """Every (profile, piece) within `reach` of the profile's origin: the level ground before the knots (-1), the segments, the
    level ground after the last knot (the slope's own end, 100 m away, is not among them)."""
    out = []
    for k, p in enumerate(profiles):
        edges = [-math.inf] + p.s + [math.inf]
        out += [(k, j - 1) for j in range(len(edges) - 1) if edges[j] < reach and edges[j + 1] > -reach]
    return out


@pytest.mark.parametrize("cfg,model", MODELS)
def test_host_terrain_forward_matches_dense_oracle(cfg, model):
    n = 256
    t, q, v, tau, sp, we, profiles, tid, tsc = to.draw(cfg, n, 51)
    out = ht.run(t["flat"], q, v, tau, mass_scale=sp, ext_wrench=we, act_perm=t.get("act_perm"), profiles=profiles, terrain_id=tid,
                 terrain_scale=tsc)
    bits = (out["contact"][None, :] >> np.arange(4)[:, None]) & 1
    assert bits.mean() >= 0.2 and (1 - bits).mean() >= 0.2          # feet on both sides of the surface
    assert (out["force"][np.repeat(bits == 0, 3, axis=0)] == 0).all()   # clear feet: exactly 0
    hits = to.segment_hits(t, q, v, profiles, tid, tsc)
    print(model, "feet per (profile, piece)", sorted(hits.items()))
    assert all(hits.get(key, 0) > 0 for key in _segments(profiles)), sorted(hits.items())
    assert tsc.min() < -0.9 and tsc.max() > 1.4
    for backend in BACKENDS:
        vd, f, ct, fl = to.forward(t, q, v, tau, profiles, tid, tsc, mass_scale=sp, ext_wrench=we, backend=backend)
        print(model, backend, "vdot", _rel(out["vdot"], vd), "force", _rel(out["force"], f))
        assert _rel(out["vdot"], vd) < 1e-9, backend
        assert _rel(out["force"], f) < 1e-9, backend
        assert np.array_equal(out["contact"], ct), backend
        keep = _keep(t, q, v, tau, sp, profiles, tid, tsc, backend)
        assert keep.sum() >= 0.9 * n, backend
        assert np.array_equal(out["flags"][keep], fl[keep]), backend
        assert ((fl & go.SLIP) != 0).any() and ((fl & go.SLIP) == 0).any()
        # the terrain matters: the plane z = 0 gives another answer
        assert _rel(go.forward(t, q, v, tau, mass_scale=sp, ext_wrench=we, backend=backend)[1], f) > 1e-3


@pytest.mark.parametrize("cfg,model", MODELS)
def test_host_terrain_step_of_eight_substeps(cfg, model):
    n, dt = 64, 1e-3
    t, q, v, tau, sp, we, profiles, tid, tsc = to.draw(cfg, n, 52, near_stance=True)
    assert set(tid.tolist()) == {0, 1, 2, 3}
    hits = to.segment_hits(t, q, v, profiles, tid, tsc)
    assert sum(c for (k, j), c in hits.items() if 0 <= j < len(profiles[k].s) - 1) > 0       # feet on inclined segments
    kw = dict(mass_scale=sp, ext_wrench=we, act_perm=t.get("act_perm"), profiles=profiles, terrain_id=tid, terrain_scale=tsc)
    out = ht.run(t["flat"], q, v, tau, dt=dt, params={"max_substep": dt / 8}, **kw)
    assert out["substeps"] == 8
    for backend in BACKENDS:
        qn, vn, fm, ct, fl = to.step(t, q, v, tau, dt, 8, profiles, tid, tsc, mass_scale=sp, ext_wrench=we, backend=backend)
        print(model, backend, "q", _rel(out["q"], qn), "v", _rel(out["v"], vn), "force", _rel(out["force"], fm))
        assert _rel(out["q"], qn) < 1e-9 and _rel(out["v"], vn) < 1e-9 and _rel(out["force"], fm) < 1e-9, backend
        assert np.array_equal(out["contact"], ct), backend
        keep = _keep(t, q, v, tau, sp, profiles, tid, tsc, backend)
        assert keep.sum() >= 0.9 * n, backend
        assert np.array_equal(out["flags"][keep], fl[keep]), backend
    # the same eight substeps one call at a time: identical state
    qs, vs = q, v
    for _ in range(8):
        o = ht.run(t["flat"], qs, vs, tau, dt=dt / 8, substeps=1, **kw)
        qs, vs = o["q"], o["v"]
    assert np.array_equal(out["q"], qs) and np.array_equal(out["v"], vs)


# ---- exact relations that need no oracle
def _both(t, q, v, tau, **kw):
    """forward and one step of 8 substeps"""
    f = ht.run(t["flat"], q, v, tau, act_perm=t.get("act_perm"), **kw)
    s = ht.run(t["flat"], q, v, tau, act_perm=t.get("act_perm"), dt=1e-3, substeps=8, **kw)
    return dict(vdot=f["vdot"], force=f["force"], contact=f["contact"], flags=f["flags"], q=s["q"], v=s["v"], step_force=s["force"],
                step_contact=s["contact"], step_flags=s["flags"])


def _close(a, b, skip=()):
    for k in a:
        if k in skip:
            continue
        if a[k].dtype == np.float64:
            assert _rel(a[k], b[k]) < 1e-9, k
        else:
            assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("model", ["mini_cheetah", "anymal_b"])
def test_raised_flat_ground_and_zero_scale_are_the_flat_plant(model):
    n, H = 32, 0.37
    t, q, v, tau, sp, we = go.draw_near_stance(model, n, 61)
    kw = dict(mass_scale=sp, ext_wrench=we)
    plain = _both(t, q, v, tau, **kw)
    qr = q.copy(); qr[6] += H
    raised = _both(t, qr, v, tau, profiles=[tr.flat(H)], **kw)
    raised["q"][6] -= H
    _close(raised, plain)
    # a scale of 0 flattens any profile, whatever segment the feet are over
    q2 = q.copy(); q2[4:6] = np.random.default_rng(3).uniform(-0.4, 0.4, (2, n))
    plain2 = _both(t, q2, v, tau, **kw)
    profiles = to.four_profiles()
    tid = (np.arange(n) % 4).astype(np.uint8)
    _close(_both(t, q2, v, tau, profiles=profiles, terrain_id=tid, terrain_scale=np.zeros(n), **kw), plain2)
    assert not np.array_equal(_both(t, q2, v, tau, profiles=profiles, terrain_id=tid, **kw)["force"], plain2["force"])


def _rotz(a, x):
    c, s = math.cos(a), math.sin(a)
    return np.stack([c * x[0] - s * x[1], s * x[0] + c * x[1], x[2]])


def _rotate_state(a, q, v):
    q2, v2 = q.copy(), v.copy()
    rw, rz = math.cos(a / 2), math.sin(a / 2)
    w, x, y, z = q[0], q[1], q[2], q[3]
    q2[0:4] = np.stack([rw * w - rz * z, rw * x - rz * y, rw * y + rz * x, rw * z + rz * w])
    q2[4:7] = _rotz(a, q[4:7])
    v2[0:3], v2[3:6] = _rotz(a, v[0:3]), _rotz(a, v[3:6])
    return q2, v2


@pytest.mark.parametrize("cfg,model", MODELS)
def test_rotating_the_world_about_z_rotates_the_answer(cfg, model):
    n, a = 64, 0.83
    t, q, v, tau, sp, we, profiles, tid, tsc = to.draw(cfg, n, 62, near_stance=True)
    kw = dict(mass_scale=sp, terrain_id=tid, terrain_scale=tsc)
    base = _both(t, q, v, tau, ext_wrench=we, profiles=profiles, **kw)
    q2, v2 = _rotate_state(a, q, v)
    we2 = np.vstack([_rotz(a, we[0:3]), _rotz(a, we[3:6])])
    rot = _both(t, q2, v2, tau, ext_wrench=we2, profiles=[p.rotated(a) for p in profiles], **kw)
    want = dict(base)
    want["q"], want["v"] = _rotate_state(a, base["q"], base["v"])
    want["vdot"] = _rotate_state(a, q, base["vdot"])[1]
    for k in ("force", "step_force"):
        want[k] = np.vstack([_rotz(a, base[k][3 * c:3 * c + 3]) for c in range(4)])
    _close(rot, want)
    assert (base["contact"] != 0).any() and _rel(rot["force"], base["force"]) > 1e-3       # and it is no identity


def test_no_profiles_is_the_flat_host_bit_for_bit():
    """The tool without a terrain runs the flat instantiation: the bits of host_ground_batch (on the device: a terrain set and
    cleared against a fresh handle, tests/test_terrain_gpu.py)."""
    t, q, v, tau, sp, we = go.draw(3, 48, 63)
    for dt in (None, 1e-3):
        kw = dict(mass_scale=sp, ext_wrench=we, act_perm=t.get("act_perm"), dt=dt)
        a, b = hg.run(t["flat"], q, v, tau, **kw), ht.run(t["flat"], q, v, tau, profiles=None, **kw)
        for k, x in a.items():
            if isinstance(x, np.ndarray):
                assert pe.same_bits(x, b[k]), (dt, k)


def test_bad_terrain_instances_on_the_host():
    """terrain_id beyond the table, NaN and inf scale: BAD, state untouched, everyone else keeps their bits; the oracle alike."""
    n = 16
    t, q, v, tau, sp, we, profiles, tid, tsc = to.draw(3, n, 64, near_stance=True)
    kw = dict(mass_scale=sp, ext_wrench=we, act_perm=t.get("act_perm"), profiles=profiles, dt=1e-3)
    clean = ht.run(t["flat"], q, v, tau, terrain_id=tid, terrain_scale=tsc, **kw)
    tid2, tsc2 = tid.copy(), tsc.copy()
    tid2[3] = 4; tid2[7] = 255; tsc2[9] = np.nan; tsc2[12] = -np.inf
    out = ht.run(t["flat"], q, v, tau, terrain_id=tid2, terrain_scale=tsc2, **kw)
    bad = np.zeros(n, bool); bad[[3, 7, 9, 12]] = True
    assert (out["flags"][bad] == go.BAD).all() and (clean["flags"] & go.BAD == 0).all()
    assert (out["force"][:, bad] == 0).all() and (out["contact"][bad] == 0).all()
    assert pe.same_bits(out["q"][:, bad], q[:, bad]) and pe.same_bits(out["v"][:, bad], v[:, bad])
    for k in ("q", "v", "force", "contact", "flags"):
        assert pe.same_bits(out[k][..., ~bad], clean[k][..., ~bad]), k
    with np.errstate(all="ignore"):
        fl = to.step(t, q, v, tau, 1e-3, 16, profiles, tid2, tsc2, mass_scale=sp, ext_wrench=we)[4]
    assert np.array_equal(fl & go.BAD, out["flags"] & go.BAD)


# ---- physics on a slope of tan(alpha) = 0.2
# What the dense numpy plant measures ("energy" agrees with "oracle" to 13 digits).  They are recorded, not recomputed here, because
# the dense run takes 5 s ("oracle") to 30 s ("energy") per case.  After a change to the oracle or to the scenario, regenerate with
#   cd tests && python -c "import terrain_oracle as to; print([to.slope_slide('mini_cheetah', mu, 'oracle') for mu in (1.0, 0.1)])"
# and take `speed` of the first and `accel` of the second.
SLOPE_ORACLE = {1.0: dict(speed=0.010618032412850784), 0.1: dict(accel=0.9619960801771976)}


@pytest.mark.parametrize("mu_p", [1.0, 0.1])
def test_slope_creep_and_slide(mu_p):
    """Mini Cheetah under the joint PD of ground_oracle.drop_test, square on a slope of tan(alpha) = 0.2 for 0.4 s, measured over
    the last 0.1 s (terrain_oracle.slope_slide).  mu_p = 1.0: no SLIP, and the trunk creeps downhill at the speed the regularised
    law predicts, v_s tan(alpha) / mu_p = 0.01 m/s.  mu_p = 0.1: SLIP, and the downhill acceleration is g (sin(alpha) - mu_p
    cos(alpha)) = 0.962 m/s^2.  The PD-held legs make both approximate: the dense numpy plant's own run of the scenario deviates
    from the formulas by
        mu_p = 1.0:  speed 0.0106180 m/s,   +6.18e-2 of the formula (still settling: its acceleration is -0.035 m/s^2)
        mu_p = 0.1:  acceleration 0.9619961 m/s^2,   +4.9e-5 of the formula
    (SLOPE_ORACLE) and the bars are 2 x those deviations.  The host instantiation reproduces the oracle's figures to 13 digits."""
    tan_a, g, vs = 0.2, 9.81, 0.05
    alpha = math.atan(tan_a)
    r = to.slope_slide("mini_cheetah", mu_p, "host", tan_alpha=tan_a)
    print("mu_p", mu_p, r)
    assert r["finite"]
    if mu_p == 1.0:
        want = vs * tan_a / mu_p
        assert not r["slip"]
        print("creep", r["speed"], "formula", want, "relative deviation", r["speed"] / want - 1.0)
        bar = 2.0 * abs(SLOPE_ORACLE[mu_p]["speed"] / want - 1.0)
        assert 0.1 < bar < 0.15 and abs(r["speed"] / want - 1.0) <= bar
    else:
        want = g * (math.sin(alpha) - mu_p * math.cos(alpha))
        assert r["slip"]
        print("acceleration", r["accel"], "formula", want, "relative deviation", r["accel"] / want - 1.0)
        bar = 2.0 * abs(SLOPE_ORACLE[mu_p]["accel"] / want - 1.0)
        assert 5e-5 < bar < 2e-4 and abs(r["accel"] / want - 1.0) <= bar


# ---- a swing foot driven horizontally into a riser
def test_swing_foot_against_a_riser():
    """Mini Cheetah in its stance, three feet 1 mm into level ground, the left front foot lifted 2 cm and moving horizontally at
    0.5 m/s along the profile's s into the riser of a ramp_step of 8 cm (its foot 1.5 cm into the riser's run, below its surface).
    The riser pushes back: f . (cos psi, sin psi) < 0.  The other feet stand before the step: their forces are, bit for bit, those
    of the same state with the step moved out of reach."""
    import energy_model as em
    model, psi, lift = "mini_cheetah", 0.3, 0.02
    t, q, v = go.drop_state(model, height=-1e-3)
    q[8, 0] -= 0.07; q[9, 0] += 0.14                      # bend the left front leg (abduction, HIP, KNEE rows 7, 8, 9): the foot lifts
    feet = go.feet_positions(t, q[:, 0])
    assert feet[0, 2] > feet[1:, 2].max() + 0.5 * lift    # the left front foot is clearly the one in the air
    q[6, 0] -= feet[1:, 2].min() + 1e-3                   # the three others 1 mm into z = 0
    feet = go.feet_positions(t, q[:, 0])
    d = np.array([math.cos(psi), math.sin(psi), 0.0])
    J = em.foot_terms_exact(t, q[:, 0], v[:, 0])[0][1]
    v[6:9, 0] = np.linalg.solve(J[:, 6:9], 0.5 * d)       # the leg's own joints drive the foot
    assert np.allclose(J @ v[:, 0], 0.5 * d, atol=1e-12)
    # the riser's run [0, 0.03) starts 1.5 cm before the foot; its height there, 0.5 * 8 cm, is above the foot
    x0, y0 = feet[0, :2] - 0.015 * d[:2]
    step = tr.ramp_step(0.0, 0.08, yaw=psi, x0=x0, y0=y0)
    far = tr.ramp_step(100.0, 0.08, yaw=psi, x0=x0, y0=y0)
    H, n = tr.evaluate(step, feet[:, 0], feet[:, 1])
    assert H[0] > feet[0, 2] > 0.5 * lift and n[0, 2] < 0.5 and (H[1:] == 0).all() and (n[1:, 2] == 1).all()
    tau = np.zeros((12, 1))
    a = ht.run(t["flat"], q, v, tau, act_perm=t.get("act_perm"), profiles=[step])
    b = ht.run(t["flat"], q, v, tau, act_perm=t.get("act_perm"), profiles=[far])
    f = a["force"][:, 0]
    print("force on the swing foot", f[0:3], "along s", f[0:3] @ d)
    assert a["contact"][0] == 15 and b["contact"][0] == 14
    assert f[0:3] @ d < 0          # (f_z is negative here: at mu_p = 1 the friction down the steep face outweighs the normal's z)
    assert (b["force"][0:3, 0] == 0).all()
    assert pe.same_bits(a["force"][3:], b["force"][3:]) and (a["force"][5::3] > 0).all()
    fo = to.forward(t, q, v, tau, [step], backend="energy")[1]
    assert _rel(a["force"], fo) < 1e-9


# ---- profiles and evaluate() of quadruped_drake_amd/terrain.py
def test_profile_constructors_and_evaluate():
    p = tr.stairs(1.0, 0.4, [0.2, 0.2], run=0.03)
    assert p.s == pytest.approx([1.0, 1.03, 1.43, 1.46]) and p.h == pytest.approx([0.0, 0.2, 0.2, 0.4])
    assert tr.ridge(1.0, 1.0, 1.0, 0.7).h == [0.0, 0.7, 0.0] and tr.flat(0.3).h == [0.3]
    for bad in (lambda: tr.Profile([0, 0], [0, 1]), lambda: tr.Profile([1, 0], [0, 1]), lambda: tr.Profile([0], [np.nan]),
                lambda: tr.Profile(range(9), range(9)), lambda: tr.Profile([], []), lambda: tr.Profile([0.0], [0.0], yaw=np.inf)):
        with pytest.raises(ValueError):
            bad()
    rng = np.random.default_rng(5)
    for prof in to.four_profiles() + [tr.ridge(-0.2, 0.3, 0.1, 0.2, yaw=1.0)]:
        x, y = rng.uniform(-0.6, 0.6, (2, 200))
        for scale in (1.0, -0.7):
            H, n = tr.evaluate(prof, x, y, scale)
            ref = [to.surface(prof, scale, a, b) for a, b in zip(x, y)]
            assert np.allclose(H, [r[0] for r in ref], rtol=0, atol=1e-15) and np.allclose(n, [r[1] for r in ref], rtol=0, atol=1e-15)
    # a slope is the plane it says: H = tan(angle) * (s - start), normal tilted back by the angle
    H, n = tr.evaluate(tr.slope(0.3, start=0.5), np.array([0.0, 1.5]), np.zeros(2))
    assert H == pytest.approx([0.0, math.tan(0.3)]) and n[1] == pytest.approx([-math.sin(0.3), 0.0, math.cos(0.3)])


# ---- C ABI argument checks that return before any device is touched
def test_abi_terrain_misuse_without_device():
    from quadruped_drake_amd import plant
    L = plant._L()
    err = lambda: L.wbc_last_error().decode()

    def check(profiles, count=None):
        arr = tr.c_array(profiles)
        return L.wbc_terrain_check(C.cast(arr, C.c_void_p), len(profiles) if count is None else count)

    def raw(nk, s, h, **kw):
        p = tr.flat(0.0, **{k: x for k, x in kw.items() if np.isfinite(x)})
        p.s, p.h = list(s), list(h)
        for k, x in kw.items():
            setattr(p, k, x)
        c = p.c_struct() if 1 <= len(p.s) <= 8 else tr.flat(0.0).c_struct()
        c.nk = nk
        return c

    def check_raw(c):
        arr = (tr.WbcTerrainProfile * 1)(c)
        return L.wbc_terrain_check(C.cast(arr, C.c_void_p), 1)

    good = to.four_profiles()
    assert check(good) == 0 and check([tr.flat(0.0)] * 16) == 0
    assert check(good, 0) < 0 and "count" in err()
    assert check([tr.flat(0.0)] * 17) < 0 and "count" in err()
    assert L.wbc_terrain_check(None, 1) < 0 and "null" in err()
    assert check_raw(raw(0, [0.0], [0.0])) < 0 and "nk" in err()
    assert check_raw(raw(9, [0.0], [0.0])) < 0 and "nk" in err()
    assert check_raw(raw(2, [0.5, 0.5], [0.0, 1.0])) < 0 and "increasing" in err()
    assert check_raw(raw(3, [0.0, 1.0, 0.5], [0.0, 1.0, 2.0])) < 0 and "increasing" in err()
    assert check_raw(raw(2, [0.0, 1.0], [0.0, np.nan])) < 0 and "finite" in err()
    assert check_raw(raw(2, [0.0, np.inf], [0.0, 1.0])) < 0 and "finite" in err()
    assert check_raw(raw(1, [0.0], [0.0], yaw=np.nan)) < 0 and "finite" in err()
    assert check_raw(raw(1, [0.0], [0.0], x0=-np.inf)) < 0 and "finite" in err()
    assert check([good[0], tr.flat(0.0)]) == 0
    bad2 = tr.c_array([good[0], good[1]]); bad2[1].nk = 9                    # the message names the profile
    assert L.wbc_terrain_check(C.cast(bad2, C.c_void_p), 2) < 0 and "profile 1" in err()
    arr = tr.c_array(good)
    assert L.wbc_ground_set_terrain(None, C.cast(arr, C.c_void_p), 4, None, None) < 0 and "null ground" in err()
    assert L.wbc_ground_terrain_kernel_info(None, None, None, None, None) < 0 and "null ground" in err()


def test_terrain_specs_and_simulate_arguments():
    """--terrain NAME[:PARAM] of simulate.py and tools/ground_bench.py: every name of terrain.SPECS, valid only with --plant ground;
    the default plant is the plan, as before."""
    from quadruped_drake_amd import simulate
    for name in tr.SPECS:
        assert isinstance(tr.from_spec(name), tr.Profile) and isinstance(tr.from_spec(name + ":0.07"), tr.Profile)
    H, n = tr.evaluate(tr.from_spec("slope:0.2"), np.array([0.0, 1.0]), np.zeros(2))
    assert H == pytest.approx([0.0, math.tan(0.2)]) and n[0] == pytest.approx([-math.sin(0.2), 0.0, math.cos(0.2)])
    for bad in ("bog", "slope:steep"):
        with pytest.raises(ValueError):
            tr.from_spec(bad)
    a = simulate.parse([])
    assert a.plant == "plan" and a.terrain is None
    a = simulate.parse(["--plant", "ground", "--terrain", "slope:0.2"])
    assert a.plant == "ground" and a.terrain == "slope:0.2"
    for argv in (["--terrain", "slope:0.2"], ["--plant", "rigid", "--terrain", "flat"], ["--plant", "ground", "--terrain", "bog"],
                 ["--plant", "mud"]):
        with pytest.raises(SystemExit):
            simulate.parse(argv)
    # a trunk placed by stance_pose stands along the normal, its origin `height` above the surface
    quat, pos = tr.stance_pose(tr.from_spec("slope:0.2"), 0.4, -0.1, 0.3)
    H, n = tr.evaluate(tr.from_spec("slope:0.2"), 0.4, -0.1)
    w, x, y, z = quat
    zaxis = np.array([2 * (x * z + w * y), 2 * (y * z - w * x), 1 - 2 * (x * x + y * y)])
    assert zaxis == pytest.approx(n) and pos == pytest.approx(np.array([0.4, -0.1, H]) + 0.3 * n)


# ---- FELL on a terrain, and a foot radius
def _trunk_clearance(q, profiles, tid, tsc):
    """Height of every trunk origin above ITS ground (terrain_oracle.surface)."""
    return np.array([q[6, i] - to.surface(profiles[tid[i]], tsc[i], q[4, i], q[5, i])[0] for i in range(q.shape[1])])


@pytest.mark.parametrize("cfg,model", MODELS)
def test_fell_is_judged_against_the_ground_under_the_trunk(cfg, model):
    """The counterpart of test_ground_cpu.test_fell_flag_and_fall_height on the four-profile batch: fall_height at the median
    height of the trunks above their own ground, so that FELL splits the sample -- in the given state (forward) and in the end
    state (step).  The flat rule, trunk height against fall_height alone, gives another answer on the same states."""
    n, dt = 128, 1e-3
    for near, run_dt in ((False, None), (True, dt)):
        t, q, v, tau, sp, we, profiles, tid, tsc = to.draw(cfg, n, 53, near_stance=near)
        fh = float(np.median(_trunk_clearance(q, profiles, tid, tsc)))
        kw = dict(mass_scale=sp, ext_wrench=we, act_perm=t.get("act_perm"), profiles=profiles, terrain_id=tid, terrain_scale=tsc)
        out = ht.run(t["flat"], q, v, tau, dt=run_dt, substeps=0 if run_dt is None else 8, params={"fall_height": fh}, **kw)
        assert (out["flags"] & go.BAD == 0).all()
        fell = (out["flags"] & go.FELL) != 0
        qe = q if run_dt is None else out["q"]
        assert np.array_equal(fell, _trunk_clearance(qe, profiles, tid, tsc) <= fh)      # the header's sentence, on the end state
        assert 0.3 * n < fell.sum() < 0.7 * n
        flat_rule = ~(qe[6] > fh)
        assert (fell != flat_rule).sum() > 0.1 * n, (fell != flat_rule).sum()
        # without the scale, or with H under another point, the answer would differ too
        assert (fell != (_trunk_clearance(qe, profiles, tid, np.ones(n)) <= fh)).any()
        P = go.params(t, {"fall_height": fh})
        for backend in BACKENDS:
            if run_dt is None:
                fl = to.forward(t, q, v, tau, profiles, tid, tsc, mass_scale=sp, ext_wrench=we, P=P, backend=backend)[3]
            else:
                fl = to.step(t, q, v, tau, dt, 8, profiles, tid, tsc, mass_scale=sp, ext_wrench=we, P=P, backend=backend)[4]
            keep = np.array([to.margin(t, q[:, i], v[:, i], tau[:, i], profiles[tid[i]], tsc[i], s_p=sp[i], P=P, backend=backend) > 1e-6
                             for i in range(n)])
            assert keep.sum() >= 0.9 * n, backend
            assert np.array_equal(out["flags"][keep], fl[keep]), backend
            assert ((fl & go.FELL) != 0).any() and ((fl & go.FELL) == 0).any()


@pytest.mark.parametrize("cfg,model", MODELS)
def test_foot_radius_is_measured_along_the_normal(cfg, model):
    """phi = foot_radius - (p_z - H) n_z: with a radius of 3 mm the feet on inclined segments tell this apart from
    (foot_radius - (p_z - H)) n_z, which differs by radius (1 - n_z): 2 % of the radius on the slope of 0.2, most of it on a riser.
    A foot whose phi the other reading changes by 1 % changes its force by 1 %, seven orders above the bar."""
    n, r = 256, 3e-3
    t, q, v, tau, sp, we, profiles, tid, tsc = to.draw(cfg, n, 54)
    P = go.params(t, {"foot_radius": r})
    out = ht.run(t["flat"], q, v, tau, mass_scale=sp, ext_wrench=we, act_perm=t.get("act_perm"), profiles=profiles, terrain_id=tid,
                 terrain_scale=tsc, params={"foot_radius": r})
    told, other_contact = 0, 0
    for i in range(n):
        for p, J in go.terms(t, q[:, i], v[:, i], sp[i], "energy")[3]:
            H, nrm, _, _ = to.surface(profiles[tid[i]], tsc[i], p[0], p[1])
            phi, alt = r - (p[2] - H) * nrm[2], (r - (p[2] - H)) * nrm[2]
            told += int(phi > 0 and abs(phi - alt) > 0.01 * phi)
            other_contact += int((phi > 0) != (alt > 0))
    print(model, "feet in contact whose phi the other reading changes by > 1 %:", told, "; whose contact bit it flips:", other_contact)
    assert told >= 10
    for backend in BACKENDS:
        vd, f, ct, fl = to.forward(t, q, v, tau, profiles, tid, tsc, mass_scale=sp, ext_wrench=we, P=P, backend=backend)
        assert _rel(out["vdot"], vd) < 1e-9 and _rel(out["force"], f) < 1e-9, backend
        assert np.array_equal(out["contact"], ct), backend
    r0 = ht.run(t["flat"], q, v, tau, mass_scale=sp, ext_wrench=we, act_perm=t.get("act_perm"), profiles=profiles, terrain_id=tid,
                terrain_scale=tsc)
    assert not np.array_equal(r0["contact"], out["contact"])
    # and through a step of 8 substeps near the stance, at the 0.7 mm of plant_edges.odd_ground_params
    t, q, v, tau, sp, we, profiles, tid, tsc = to.draw(cfg, 64, 55, near_stance=True)
    kw = dict(mass_scale=sp, ext_wrench=we)
    o = ht.run(t["flat"], q, v, tau, act_perm=t.get("act_perm"), profiles=profiles, terrain_id=tid, terrain_scale=tsc, dt=1e-3, substeps=8,
               params={"foot_radius": 0.7e-3}, **kw)
    qn, vn, fm, ct, fl = to.step(t, q, v, tau, 1e-3, 8, profiles, tid, tsc, P=go.params(t, {"foot_radius": 0.7e-3}), backend="energy", **kw)
    assert _rel(o["q"], qn) < 1e-9 and _rel(o["v"], vn) < 1e-9 and _rel(o["force"], fm) < 1e-9 and np.array_equal(o["contact"], ct)
