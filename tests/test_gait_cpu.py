"""The gait planner (include/wbc_gait.h), no GPU: the host instantiation of csrc/wbc_gait.hpp (tests/host_gait.py) against the
numpy restatement of the header's sentences (tests/gait_oracle.py), the half-open rule on exact boundaries, relations that need no
oracle, the argument checks that return before any device is touched, the binding table against the header, gait.STRIDES against
the reference's text, malformed instances, and the closed loop on the host twins: ID walking at a commanded velocity on the plane
and up a slope of grade 0.2 with followed targets, and failing on that slope with level ones.

The bars of the comparison with the oracle are measured here, per row group (positions, velocities, accelerations): 100 x the
largest difference between the oracle in double and in extended precision on the same inputs ("GAIT ..." lines print them)."""
import ctypes as C
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import gait_oracle as go
import host_gait as hg
import plant_edges as pe
from quadruped_drake_amd import gait

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = "/root/reference/towr/src/quadruped_gait_generator.cc"
POS = [0, 1, 2, 9, 10, 11] + [18 + 9 * f + k for f in range(4) for k in range(3)]
VEL = [r + 3 for r in POS]
ACC = [r + 6 for r in POS]
GROUPS = (("positions", POS), ("velocities", VEL), ("accelerations", ACC))
DT_SAMPLE, T_END, OFFSET = 7.3e-3, 20.0, 1.234e-4
# (c_x, c_y, omega): |c| <= 1.5 m/s, |omega| <= 2 rad/s, omega = 0, and omega = 2e-5 rad/s, whose |omega theta / 2| crosses 1e-4 at
# theta = 10 s, inside the 20 s of samples
COMMANDS = [(0.2, 0.0, 0.0), (1.5, 0.0, 2.0), (-0.9, 1.2, -2.0), (0.4, 0.0, 0.5), (0.0, 0.0, 0.0), (0.7, -0.3, 2e-5), (0.0, 0.5, -1.1),
            (-1.06, -1.06, 1e-3), (0.3, 0.1, -2e-5)]
SCALES = [0.5, 0.77, 1.0, 1.3, 2.0]
STARTS = [(0.0, 0.0, 0.0), (0.3, -0.2, 0.9), (-1.0, 2.0, -2.5), (0.05, 0.0, 3.0)]


def sample_batch(shift, wait_time=0.0):
    """The test's samples: a time every 7.3 ms over 0 .. 20 s (offset by 0.1234 ms, which keeps every sample off every boundary of
    every stride at every scale of SCALES: both are whole numbers of 1e-7 s, the samples 234 mod 1000 of them, the boundaries 0),
    preceded by 24 samples with tau < 0; commands, scales and starts are dealt round, `shift` moving the deal."""
    t = np.r_[-np.arange(1, 25) * 0.011, np.arange(int(T_END / DT_SAMPLE)) * DT_SAMPLE + OFFSET] + wait_time
    i = np.arange(t.size) + shift
    cmd = np.array(COMMANDS)[i % len(COMMANDS)].T.copy()
    sc = np.array(SCALES)[(i // 2) % len(SCALES)].copy()
    st = np.array(STARTS)[(i // 3) % len(STARTS)].T.copy()
    return t, cmd, sc, st


@pytest.mark.parametrize("name", list(gait.STRIDES))
def test_host_twin_matches_the_oracle_on_every_stride(name):
    P = hg.params(wait_time=0.25)
    S = [gait.stride(name)]
    for shift in (0, 4):
        t, cmd, sc, st = sample_batch(shift, P["wait_time"])
        dist = go.boundary_distance(S[0][0], t, P["wait_time"], sc)
        assert t.size == 24 + 2739 and float(dist[24:].min()) >= 1e-9, float(dist[24:].min())        # no sample dropped, none on a boundary
        got, gmask = hg.run([name], t, cmd, None, sc, st, p=P)
        want, wmask = go.targets(P, S, t, cmd, None, sc, st)
        wide, lmask = go.targets(P, S, t, cmd, None, sc, st, dtype=np.longdouble)
        assert (gmask == wmask).all() and (wmask == lmask).all()
        assert (gmask[:24] == 0xF).all() and np.isfinite(got).all()
        assert float(np.abs(cmd[2] * 20 / 2).max()) > 1e-4 > float(np.abs(cmd[2][cmd[2] != 0] * 1e-3).min())
        for group, rows in GROUPS:
            bar = 100.0 * float(np.abs(want[rows] - wide[rows]).max())
            worst = float(np.abs(got[rows] - wide[rows]).max())
            print("GAIT twin-to-oracle %-12s %-13s worst %.3g bar %.3g" % (name, group, worst, bar))
            assert bar > 0 and worst < bar, (name, group, worst, bar)
    if name != "stand":
        assert np.abs(got[[20, 29, 38, 47]]).max() > 0.04                                                # and feet were lifted


DYADIC = ((0.25, 0.125, 0.25, 0.125), (0b1001, 0b1111, 0b0110, 0b1111))


@pytest.mark.parametrize("scale", [1.0, 0.5, 2.0])
def test_exact_boundaries_follow_the_half_open_rule(scale):
    """tau on every boundary of four strides of a stride with dyadic durations (every product and sum of the clock is then exact):
    stride number, phase, mask, the run's start and u -- as gait_foot itself computes them and hands them out -- are those of the
    half-open rule, nothing excluded."""
    d, m = DYADIC
    B = [Fraction(0)]
    for x in d:
        B.append(B[-1] + Fraction(x))
    s = Fraction(scale)
    T = s * B[-1]
    cases = [(k, j) for k in range(4) for j in range(4)] + [(4, 0)]
    tau = np.array([float(k * T + s * B[j]) for k, j in cases])
    n = tau.size
    cmd = np.tile([[0.3], [0.1], [0.4]], (1, n))
    P = hg.params(ramp_time=0.0)
    for f in range(4):
        got, mask, diag = hg.run([DYADIC], tau, cmd, None, np.full(n, scale), None, p=P, diag_foot=f)
        _, omask = go.targets(P, [DYADIC], tau, cmd, None, np.full(n, scale))
        _, _, _, ophase = go.clock(d, tau, np.full(n, scale))
        for i, (k, j) in enumerate(cases):
            contact, lo, hi, _, _ = go.runs(m, f, j)
            at = lambda b: k * T + s * (B[b % 4] + (b // 4) * B[4])
            assert diag[0, i] == k and diag[1, i] == j == ophase[i] and mask[i] == m[j] == omask[i], (f, k, j)
            assert diag[3, i] == float(at(lo)), (f, k, j)
            assert diag[2, i] == float((Fraction(tau[i]) - at(lo)) / (at(hi) - at(lo))), (f, k, j)
            if not contact and lo % 4 == j:
                assert diag[2, i] == 0.0 and got[18 + 9 * f + 2, i] == 0.0          # lift-off: u = 0, the foot on the ground
            assert (got[18 + 9 * f + 2, i] > 0) == (not contact and lo % 4 != j)


# ---- exact relations, on the oracle and on the twin
def _twin(P, S, t, cmd, sc=None, st=None):
    return hg.run(S, t, cmd, None, sc, st, p=P)[0]


def _oracle(P, S, t, cmd, sc=None, st=None):
    return go.targets(P, [gait.stride(s) for s in S], t, cmd, None, sc, st)[0]


ENGINES = [("twin", _twin), ("oracle", _oracle)]
XY_ROWS = [0, 3, 6] + [18 + 9 * f + 3 * d for f in range(4) for d in range(3)]


def _rotz_rows(a, t):
    c, s = math.cos(a), math.sin(a)
    out = t.copy()
    for r in XY_ROWS:
        out[r], out[r + 1] = c * t[r] - s * t[r + 1], s * t[r] + c * t[r + 1]
    return out


@pytest.mark.parametrize("engine", ENGINES, ids=lambda e: e[0])
def test_turning_the_start_turns_every_answer_about_z(engine):
    """Bars: a foothold or a body position carries a dozen roundings of numbers of up to 30 m, e = 2e-14.  Positions: 10 e.  A swing
    foot's rates multiply the step B - A by sigma' / D <= 1.875 / D and sigma'' / D^2 <= 5.774 / D^2, D >= 0.15 s the shortest swing
    of these strides at scale 0.5: velocities 2.5e-13, accelerations 5.2e-12."""
    t, cmd, sc, st = sample_batch(1)
    a = 0.83
    st2 = st.copy()
    st2[0], st2[1] = math.cos(a) * st[0] - math.sin(a) * st[1], math.sin(a) * st[0] + math.cos(a) * st[1]
    st2[2] = st[2] + a
    P = hg.params()
    for name in ("trot", "gallop", "walk"):
        base = engine[1](P, [name], t, cmd, sc, st)
        got = engine[1](P, [name], t, cmd, sc, st2)
        want = _rotz_rows(a, base)
        want[11] = base[11] + a
        for rows, bar in ((POS, 2e-13), (VEL, 2.5e-13), (ACC, 5.2e-12)):
            assert float(np.abs(got[rows] - want[rows]).max()) < bar, (name, bar, float(np.abs(got[rows] - want[rows]).max()))
        assert float(np.abs(got - base).max()) > 0.1


@pytest.mark.parametrize("engine", ENGINES, ids=lambda e: e[0])
def test_zero_command_leaves_the_footholds_at_the_start_stance_and_the_body_at_rest(engine):
    t, _, sc, st = sample_batch(2)
    P = hg.params()
    for name in gait.STRIDES:
        got = engine[1](P, [name], t, np.zeros((3, t.size)), sc, st)
        assert (got[0:2] == st[0:2]).all() and (got[2] == P["height"]).all() and (got[11] == st[2]).all()
        assert (got[[3, 4, 5, 6, 7, 8, 9, 10, 12, 13, 14, 15, 16, 17]] == 0).all()
        for f in range(4):
            c, s = np.cos(st[2]), np.sin(st[2])
            fx = st[0] + (c * P["stance"][f, 0] - s * P["stance"][f, 1])
            fy = st[1] + (s * P["stance"][f, 0] + c * P["stance"][f, 1])
            r = 18 + 9 * f
            assert float(np.abs(got[r] - fx).max()) < 1e-15 and float(np.abs(got[r + 1] - fy).max()) < 1e-15     # one rounding of order one
            assert (got[[r + 3, r + 4, r + 6, r + 7]] == 0).all()


def _run_times(name, scale, strides=(2, 3, 4)):
    """[(foot, contact, a, b)] of every run that starts in the given strides of `name` at `scale`, absolute times"""
    d, m = gait.stride(name)
    B = go.boundaries(d)
    out = []
    for f in range(4):
        for k in strides:
            for j in range(len(d)):
                contact, lo, hi, _, _ = go.runs(m, f, j)
                if lo is not None and lo == j:
                    out.append((f, contact, scale * (k * B[-1] + go.boundary(B, lo)), scale * (k * B[-1] + go.boundary(B, hi))))
    return out


@pytest.mark.parametrize("engine", ENGINES, ids=lambda e: e[0])
def test_at_mid_stance_the_foot_is_under_the_body(engine):
    """foot = p_body + Rz(psi) stance_f at the middle of every stance run; bar 1e-13: a dozen roundings of numbers of order one"""
    P = hg.params()
    cmd1 = (0.4, -0.1, 0.5)
    for name in gait.STRIDES:
        if name == "stand":
            continue
        for scale in (0.5, 1.0):
            stance = [(f, 0.5 * (a + b)) for f, contact, a, b in _run_times(name, scale) if contact]
            t = np.array([x[1] for x in stance])
            n = t.size
            assert n >= 12
            st = np.tile([[0.2], [-0.1], [0.7]], (1, n))
            got = engine[1](P, [name], t, np.tile(np.array(cmd1)[:, None], (1, n)), np.full(n, scale), st)
            for i, (f, _) in enumerate(stance):
                c, s = math.cos(got[11, i]), math.sin(got[11, i])
                want = got[0:2, i] + [c * P["stance"][f, 0] - s * P["stance"][f, 1], s * P["stance"][f, 0] + c * P["stance"][f, 1]]
                r = 18 + 9 * f
                assert np.abs(got[r:r + 2, i] - want).max() < 1e-13 and (got[r + 2:r + 9, i] == 0).all(), (name, scale, f)


@pytest.mark.parametrize("engine", ENGINES, ids=lambda e: e[0])
def test_feet_are_continuous_across_every_lift_off_and_touch_down(engine):
    """Position, velocity and acceleration of the foot eps = 1e-9 s before and after every boundary of its runs.  With u = eps / D on
    the swing side, D >= 0.05 s the shortest swing here (limp at scale 0.5) and L <= 1.2 m the longest step: |dp| <= (10 L + 64 h) u^3
    < 1e-12 (+ a rounding of the position, 1e-14), |dv| <= (30 L + 192 h) u^2 / D < 1e-12, |da| <= (60 L + 384 h) u / D^2 < 1e-3."""
    P = hg.params()
    eps = 1e-9
    cmd1 = (0.5, 0.1, 0.4)
    for name in gait.STRIDES:
        if name == "stand":
            continue
        for scale in (0.5, 1.0):
            edges = [(f, x) for f, _, a, b in _run_times(name, scale) for x in (a, b)]
            tb = np.array([x[1] for x in edges])
            n = tb.size
            cmd = np.tile(np.array(cmd1)[:, None], (1, n))
            lo = engine[1](P, [name], tb - eps, cmd, np.full(n, scale))
            hi = engine[1](P, [name], tb + eps, cmd, np.full(n, scale))
            lifted = 0
            for i, (f, _) in enumerate(edges):
                r = 18 + 9 * f
                d = np.abs(hi[r:r + 9, i] - lo[r:r + 9, i])
                assert d[0:3].max() < 1e-12 + 1e-14 and d[3:6].max() < 1e-12 and d[6:9].max() < 1e-3, (name, scale, f, d)
                lifted += (lo[r + 2, i] > 0) != (hi[r + 2, i] > 0)
            assert lifted == n                                                       # every edge separates a stance from a swing


def test_central_differences_reproduce_the_rates():
    """pd and pdd of the body and of every foot against central differences of p and pd.  The bar is the difference's truncation,
    h^2 / 6 times the next derivative, plus its rounding, 2 eps |f| / h.  Trot at scale 1 (swing D = 0.3 s), command (0.5, 0.1, 0.4):
    steps L <= 0.6 m, so |p'''| <= 60 L / D^3 + 64 h 60 / D^3 < 1500 + 7200 and |p''''| <= 360 (L + 64 h / 3) / D^4 < 8e4.  Oracle in
    extended precision, h = 1e-6: 2e-9 and 2e-8 (rounding 1e-13).  Twin in double, h = 1e-5: 2e-7 + 1e-10 and 2e-6 + 1e-9."""
    P = hg.params()
    t = np.arange(200, 2400) * DT_SAMPLE / 4 + OFFSET
    n = t.size
    cmd = np.tile([[0.5], [0.1], [0.4]], (1, n))
    S = [gait.stride("trot")]
    wide = lambda x: go.targets(P, S, x, cmd, dtype=np.longdouble)[0]
    for label, f, h, bars in (("oracle", wide, 1e-6, (2e-9, 2e-8)), ("twin", lambda x: _twin(P, ["trot"], x, cmd), 1e-5, (3e-7, 3e-6))):
        # the difference is taken of the answers at t - h and t + h as double rounds those times: divide by what they are apart
        lo, hi = t - h, t + h
        span = (hi.astype(np.longdouble) - lo.astype(np.longdouble)) if label == "oracle" else hi - lo
        mid, a, b = f(t), f(lo), f(hi)
        for order, (src, dst) in enumerate(((POS, VEL), (VEL, ACC))):
            worst = float(np.abs((b[src] - a[src]) / span - mid[dst]).max())
            print("GAIT central difference %s %s: worst %.3g bar %.3g" % (label, ("pd", "pdd")[order], worst, bars[order]))
            assert worst < bars[order]


@pytest.mark.parametrize("engine", ENGINES, ids=lambda e: e[0])
def test_the_arc_meets_the_straight_line_as_the_yaw_rate_goes_to_zero(engine):
    """omega = 0: p = p0 + theta Rz(psi0) c to 1e-13.  omega = 1e-12 rad/s: the arc leaves that line by |c| theta^2 omega / 2 <
    1.5 * 400 * 1e-12 / 2 = 3e-10 over 20 s; bar 4e-10."""
    t, cmd, sc, st = sample_batch(3)
    t, cmd, sc, st = t[24:], cmd[:, 24:], sc[24:], st[:, 24:]
    P = hg.params()
    cmd[2] = 0.0
    line = engine[1](P, ["trot"], t, cmd, sc, st)
    th = go.theta(P["ramp_time"], t)[0]
    c, s = np.cos(st[2]), np.sin(st[2])
    want = st[0:2] + th * np.stack([c * cmd[0] - s * cmd[1], s * cmd[0] + c * cmd[1]])
    assert float(np.abs(line[0:2] - want).max()) < 1e-13
    cmd[2] = 1e-12
    arc = engine[1](P, ["trot"], t, cmd, sc, st)
    worst = float(np.abs(arc[POS] - line[POS]).max())
    assert 0 < worst < 4e-10, worst


# ---- malformed instances
MALFORMED = [("time", math.nan), ("time", math.inf), ("cmd0", math.nan), ("cmd1", -math.inf), ("cmd2", math.inf), ("start0", math.nan),
             ("start1", math.inf), ("start2", -math.inf), ("scale", 0.0), ("scale", -1.0), ("scale", math.inf), ("scale", math.nan),
             ("gait_id", None)]


def spoil(case, value, i, count, time, cmd, gid, sc, st):
    """instance i of the arrays made malformed in the way `case` names"""
    if case == "time":
        time[i] = value
    elif case == "scale":
        sc[i] = value
    elif case == "gait_id":
        gid[i] = count
    else:
        (cmd if case.startswith("cmd") else st)[int(case[-1]), i] = value


def malformed_batch(n, count, seed=5):
    rng = np.random.default_rng(seed)
    time = rng.uniform(0.0, 6.0, n)
    cmd = np.stack([rng.uniform(-1, 1, n), rng.uniform(-0.5, 0.5, n), rng.uniform(-2, 2, n)])
    gid = (np.arange(n) % count).astype(np.uint8)
    sc = rng.uniform(0.5, 2.0, n)
    st = rng.uniform(-1, 1, (3, n))
    return time, cmd, gid, sc, st


def test_malformed_instances_get_nan_rows_and_a_full_mask_and_their_neighbours_nothing():
    names = ["trot", "walk", "pace"]
    twin = None
    n = 3 * len(MALFORMED) + 2
    clean = malformed_batch(n, len(names))
    dirty = [a.copy() for a in clean]
    bad = np.zeros(n, bool)
    for k, (case, value) in enumerate(MALFORMED):
        spoil(case, value, 3 * k + 1, len(names), *dirty)
        bad[3 * k + 1] = True
    P = hg.params()
    S = [gait.stride(s) for s in names]
    for label, f in (("twin", lambda a: hg.run(names, a[0], a[1], a[2], a[3], a[4], p=P)),
                     ("oracle", lambda a: go.targets(P, S, a[0], a[1], a[2], a[3], a[4]))):
        ct, cm = f(clean)
        dt_, dm = f(dirty)
        twin = ct if label == "twin" else twin
        assert np.isfinite(ct).all(), label
        assert np.isnan(dt_[:, bad]).all() and (dm[bad] == 0xF).all(), label
        assert pe.same_bits(dt_[:, ~bad], ct[:, ~bad]) and (dm[~bad] == cm[~bad]).all(), label
    # padding columns n .. ld are not the batch's
    wide = (np.full((54, n), 7.5), np.full(n, 0x55, np.uint8))
    hg.run(names, *clean, p=P, n=n - 5, out=wide)
    assert (wide[0][:, n - 5:] == 7.5).all() and (wide[1][n - 5:] == 0x55).all() and pe.same_bits(wide[0][:, :n - 5], twin[:, :n - 5])


# ---- what returns before any device is touched
def _stride(durations, masks):
    return gait.c_strides([(durations, masks)])


def test_abi_gait_misuse_without_device():
    from quadruped_drake_amd import _lib
    L = _lib.lib()
    err = lambda: L.wbc_last_error().decode()
    P = hg.params()
    cp = gait.c_params(P["stance"], P["height"], P["swing_height"], P["ramp_time"], P["wait_time"])
    trot = gait.c_strides(["trot"])
    h = C.c_void_p()
    for fn, tail in ((L.wbc_gait_check, ()), (L.wbc_gait_create, (0, C.byref(h)))):
        name = fn.__name__
        assert fn(None, trot, 1, *tail) < 0 and "null" in err()
        assert fn(C.byref(cp), None, 1, *tail) < 0 and "null" in err()
        for count in (0, 17, -1):
            assert fn(C.byref(cp), gait.c_strides(["trot"] * 17), count, *tail) < 0 and "count" in err() and name in err()
        s = gait.c_strides(["trot"])
        for nphase in (0, 9):
            s[0].nphase = nphase
            assert fn(C.byref(cp), s, 1, *tail) < 0 and "nphase" in err()
        for bad in (0.0, -0.3, math.inf, math.nan):
            assert fn(C.byref(cp), _stride((0.3, bad, 0.3, 0.2), (9, 15, 6, 15)), 1, *tail) < 0 and "duration" in err()
        assert fn(C.byref(cp), _stride((0.3, 0.2), (0b1101, 0b0101)), 1, *tail) < 0 and "every foot" in err()      # RF never stands
        s = gait.c_strides(["trot"])
        s[0].contact[1] = 0x1F
        assert fn(C.byref(cp), s, 1, *tail) < 0 and "0xF" in err()
        for field, value in (("ramp_time", -0.1), ("ramp_time", math.nan), ("height", math.inf), ("swing_height", math.nan), ("wait_time", math.inf)):
            cq = gait.c_params(P["stance"], P["height"], P["swing_height"], P["ramp_time"], P["wait_time"])
            setattr(cq, field, value)
            assert fn(C.byref(cq), trot, 1, *tail) < 0 and field in err()
        assert not h.value
    assert L.wbc_gait_check(C.byref(cp), gait.c_strides(list(gait.STRIDES)), len(gait.STRIDES)) == 0
    assert L.wbc_gait_create(C.byref(cp), trot, 1, 0, None) < 0 and "null" in err()
    assert L.wbc_gait_create(C.byref(cp), trot, 1, -1, C.byref(h)) < 0 and "device" in err()
    # a handle needs no device until its first wbc_gait_set_commands
    assert L.wbc_gait_create(C.byref(cp), trot, 1, 0, C.byref(h)) == 0 and h.value
    buf, tm, mk = np.zeros((54, 4)), np.zeros(4), np.zeros(4, np.uint8)
    p = lambda a: C.c_void_p(a.ctypes.data)
    assert L.wbc_gait_targets(None, None, 4, 4, p(tm), p(buf), p(mk)) < 0 and "null gait handle" in err()
    assert L.wbc_gait_targets(h, None, 4, 3, p(tm), p(buf), p(mk)) < 0 and "ld must be >= n" in err()
    assert L.wbc_gait_targets(h, None, -1, 4, p(tm), p(buf), p(mk)) < 0 and "n out of range" in err()
    assert L.wbc_gait_targets(h, None, (1 << 24) + 1, 1 << 25, p(tm), p(buf), p(mk)) < 0 and "WBC_MAX_LD" in err()
    assert L.wbc_gait_targets(h, None, 4, 4, None, p(buf), p(mk)) < 0 and "are required" in err()
    assert L.wbc_gait_targets(h, None, 4, 4, p(tm), None, p(mk)) < 0 and "are required" in err()
    assert L.wbc_gait_targets(h, None, 4, 4, p(tm), p(buf), None) < 0 and "are required" in err()
    assert L.wbc_gait_targets(h, None, 4, 4, p(tm), p(buf), p(mk)) < 0 and "wbc_gait_set_commands" in err()
    assert L.wbc_gait_targets(h, None, 0, 0, None, None, None) < 0 and "wbc_gait_set_commands" in err()
    assert L.wbc_gait_set_commands(None, p(buf), None, None, None) < 0 and "null gait handle" in err()
    assert L.wbc_gait_set_commands(h, None, None, None, None) < 0 and "cmd is required" in err()
    assert L.wbc_gait_kernel_info(None, None, None, None, None) < 0 and "null gait handle" in err()
    assert L.wbc_ground_set_gait(None, h) < 0 and "null ground handle" in err()
    assert L.wbc_plant_set_gait(None, h) < 0 and "null plant handle" in err()
    assert (buf == 0).all() and (mk == 0).all()
    assert L.wbc_gait_destroy(h) == 0 and L.wbc_gait_destroy(None) == 0
    with pytest.raises(ValueError):
        gait.stride("canter")
    with pytest.raises(ValueError):
        gait.stride(((0.1,) * 9, (15,) * 9))


def test_closed_loop_with_a_trajectory_touches_no_entry_point_of_the_gait(monkeypatch):
    """A library from before the gait planner (WBC_HIP_LIB: the A/B timing of tools/*_bench.py) lacks every name that
    include/wbc_gait.h declares, and lib() leaves them unbound.  closed_loop with an ordinary trajectory must then run as it did: here both plants' loops are
    driven, without a device, over a stand-in library that raises on any of those names and records the rollout it is asked for."""
    import types
    import torch
    import test_abi_cpu as abi
    from quadruped_drake_amd import _lib, plant
    gait_names = set(abi._header_prototypes("wbc_gait.h"))
    assert len(gait_names) == 8

    class OldLibrary:
        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            if name in gait_names:
                raise AttributeError("undefined symbol: " + name)
            assert name in _lib.PROTOTYPES and name not in _lib._NEWER, name

            def call(*args):
                self.calls.append((name, args))
                return 0
            return call

    assert "WBC_HIP_LIB" in os.environ or not gait_names & set(_lib._MAY_LACK)
    monkeypatch.setattr(plant, "_dev_ptr", lambda a, *rest: None if a is None else C.c_void_p(a.data_ptr()))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda d=None: types.SimpleNamespace(cuda_stream=0))
    n = 3
    for cls, entry in ((plant.GroundContactPlant, "wbc_ground_rollout"), (plant.RigidContactPlant, "wbc_plant_rollout")):
        L = OldLibrary()
        p = object.__new__(cls)
        p._L, p._h, p.device, p._terrain = L, C.c_void_p(8), 0, None
        ctrl = types.SimpleNamespace(host_ptrs=False, _h=C.c_void_p(16))
        traj = types.SimpleNamespace(_h=C.c_void_p(24))
        q, v, tm = torch.zeros((19, n), dtype=torch.float64), torch.zeros((18, n), dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
        out = plant.closed_loop(ctrl, p, traj, 4, 5e-3, q, v, tm)
        assert [c[0] for c in L.calls] == [entry] and L.calls[0][1][2] is traj._h and len(out) == (8 if entry == "wbc_ground_rollout" else 7)
        p._h = None                                            # nothing to destroy
        # and with a gait the setter is what is missing: the error names it
        g = object.__new__(gait.GaitPlanner)
        g._h, g._n, g.device = C.c_void_p(32), n, 0
        with pytest.raises(AttributeError, match="set_gait"):
            plant.closed_loop(ctrl, p, g, 4, 5e-3, q, v, tm)
        g._h = None


# ---- gait.STRIDES against the reference's text
@pytest.mark.skipif(not os.path.exists(REFERENCE), reason="the reference's quadruped_gait_generator.cc is not on this machine")
def test_strides_are_the_reference_s():
    text = open(REFERENCE).read()
    bit = {"LF": 1, "RF": 2, "LH": 4, "RH": 8}
    state = {"II_": 0, "BB_": 15}
    for name, foot in re.findall(r"(\w\w_)\.at\((\w\w)\)\s*=\s*true", text):
        state[name] = state.get(name, 0) | bit[foot]
    assert len(state) == 16 and state["bP_"] == 0b1001 and state["Pb_"] == 0b0110
    functions = {"stand": "Stand", "walk": "Walk", "walk_overlap": "WalkOverlap", "trot": "Trot", "trot_fly": "TrotFly", "pace": "Pace",
                 "bound": "Bound", "pronk": "Pronk", "gallop": "Gallop", "limp": "Limp"}
    assert sorted(functions) == sorted(gait.STRIDES)
    for name, fn in functions.items():
        body = re.search(r"GetStride%s \(\) const\s*\{(.*?)\n\}" % fn, text, flags=re.S).group(1)
        body = re.sub(r"//[^\n]*", "", body)
        values = {k: float(v) for k, v in re.findall(r"double\s+(\w+)\s*=\s*([0-9.]+)\s*;", body)}
        lists = re.findall(r"=\s*\{(.*?)\}\s*;", body, flags=re.S)
        assert len(lists) == 2, name
        times = [values[x] if x in values else float(x) for x in re.findall(r"[\w.]+", lists[0])]
        masks = [state[x] for x in re.findall(r"\w\w_", lists[1])]
        assert (tuple(times), tuple(masks)) == gait.STRIDES[name], name
    assert gait.STRIDES["trot"] == ((0.3, 0.2, 0.3, 0.2), (0b1001, 0b1111, 0b0110, 0b1111))


def test_simulate_gait_arguments():
    from quadruped_drake_amd import simulate
    a = simulate.parse(["--planner", "gait", "--plant", "ground", "--cmd", "0.2,0,0.5"])
    assert (a.gait, a.cmd, a.cmd_spread, a.stride_scale) == ("trot", (0.2, 0.0, 0.5), (0.0, 0.0, 0.0), 0.5)
    a = simulate.parse(["--planner", "gait", "--plant", "rigid", "--gait", "walk", "--cmd", "0.1,0,0", "--cmd-spread", "0.1,0.05,0.3",
                        "--stride-scale", "1.0"])
    assert (a.gait, a.cmd_spread, a.stride_scale) == ("walk", (0.1, 0.05, 0.3), 1.0)
    for argv in (["--planner", "gait"], ["--planner", "gait", "--plant", "plan"], ["--planner", "gait", "--plant", "ground", "--gait", "canter"],
                 ["--planner", "gait", "--plant", "ground", "--cmd", "0.2,0"], ["--planner", "gait", "--plant", "ground", "--stride-scale", "0"],
                 ["--planner", "gait", "--plant", "ground", "--cmd", "a,b,c"], ["--planner", "gait", "--plant", "ground", "--cmd-spread", "-1,0,0"]):
        with pytest.raises(SystemExit):
            simulate.parse(argv)
    cmd = simulate.draw_commands(a, 64)
    assert cmd.shape == (3, 64) and (np.abs(cmd - np.array(a.cmd)[:, None]) <= np.array(a.cmd_spread)[:, None]).all()
    assert (cmd == simulate.draw_commands(a, 64)).all() and len(set(cmd[0])) == 64
    assert "defaults to 0.5" in simulate.__doc__


# ---- the closed loop on the host twins
SLIP, FELL, BAD = 1, 2, 8


def host_walk(cmd, grade=None, follow="fit", scale=0.5, ticks=600, dt=5e-3, model="mini_cheetah"):
    """ID under the gait's targets, every tick: gait (host_gait) -> follow (host_follow, on a slope) -> tick (host_tick) -> ground step
    (host_terrain / host_ground).  Trot at stride scale `scale`, GaitPlanner's defaults.  grade None: the plane, else
    terrain_oracle.slope_stance(model, grade).  -> dict(status: ticks with a non-zero status, flags: OR of the plant's flags,
    first_bad / first_fell: the first tick that raised BAD / FELL or None, off: final distance of the trunk's (x, y) from the planned
    body position, dx, dy: its components, height: final trunk height above the ground under it)"""
    import host_follow as hf
    import host_ground as hgr
    import host_terrain as ht
    import host_tick as hk
    import terrain_oracle as to
    from quadruped_drake_amd import terrain as tr, workloads
    from quadruped_drake_amd.controller import load_model
    if grade is None:
        t, prof = load_model(model), None
        q, v = workloads.nominal_state(model, 1)
    else:
        t, q, v, prof = to.slope_stance(model, grade)
    P = hg.params(model)
    c = np.array(cmd, dtype=np.float64)[:, None]
    sc = np.array([scale])
    out = dict(status=0, flags=0, first_bad=None, first_fell=None)
    for k in range(ticks):
        tg, mask = hg.run(["trot"], np.array([k * dt]), c, None, sc, None, p=P)
        if prof is not None:
            tg = hf.run([prof], tg, follow)
        tau, _, status, _ = hk.run("id", t["flat"], q, v, tg, mask, act_perm=t.get("act_perm"))
        if prof is None:
            o = hgr.run(t["flat"], q, v, tau, act_perm=t.get("act_perm"), dt=dt)
        else:
            o = ht.run(t["flat"], q, v, tau, act_perm=t.get("act_perm"), dt=dt, profiles=[prof])
        q, v = o["q"], o["v"]
        out["status"] += int(status[0] != 0)
        out["flags"] |= int(o["flags"][0])
        for key, flag in (("first_bad", BAD), ("first_fell", FELL)):
            if out[key] is None and o["flags"][0] & flag:
                out[key] = k
        if o["flags"][0] & BAD:
            break
    plan = go.targets(P, [gait.stride("trot")], np.array([ticks * dt]), c, None, sc)[0][:, 0]
    out["dx"], out["dy"] = float(q[4, 0] - plan[0]), float(q[5, 0] - plan[1])
    out["off"] = math.hypot(out["dx"], out["dy"])
    ground = 0.0 if prof is None else float(tr.evaluate(prof, q[4, 0], q[5, 0])[0])
    out["height"] = float(q[6, 0] - ground)
    out["x"], out["y"] = float(q[4, 0]), float(q[5, 0])
    return out


WALKS = [((0.2, 0.0, 0.0), None), ((-0.2, 0.0, 0.0), None), ((0.4, 0.0, 0.5), None), ((0.2, 0.0, 0.0), 0.2)]


@pytest.mark.parametrize("cmd,grade", WALKS, ids=["forward", "backward", "arc", "slope_0.2_fit"])
def test_id_walks_at_the_commanded_velocity_on_the_host_twins(cmd, grade):
    """Mini Cheetah, ID, dt 5 ms, trot at stride scale 0.5, 600 ticks (3 s), ramp 0.5 s: no FELL, no BAD, status 0 on every tick, the
    trunk within 0.03 m of the planned body position and its height above the ground under it within 5 mm of 0.3 m.  SLIP is raised in
    every run (a trot's feet creep), so the loop is not contractive to rounding and the bars are about ten times the measured figures,
    which the "GAIT host walk" lines print.  Measured: forward x 0.5511 (plan 0.5500), 1.1 mm and 2.2 mm off in x and y; backward 2.3 mm
    and 5.8 mm; the arc 0.8 mm and 0.7 mm; the slope 1.4 mm and 3.0 mm; heights 0.2999, 0.3001, 0.2999 and, above the slope, 0.2996 m."""
    r = host_walk(cmd, grade)
    print("GAIT host walk cmd %s grade %s: x %.4f y %.4f dx %+.4f dy %+.4f height %.4f flags %d status %d" %
          (cmd, grade, r["x"], r["y"], r["dx"], r["dy"], r["height"], r["flags"], r["status"]))
    assert not r["flags"] & (FELL | BAD) and r["status"] == 0
    assert r["off"] < 0.03 and abs(r["height"] - 0.3) < 5e-3


def test_id_does_not_walk_up_the_slope_with_level_targets():
    """The same slope of grade 0.2 at stride scale 0.5 with level targets: BAD before tick 600 (measured: tick 47)."""
    r = host_walk((0.2, 0.0, 0.0), 0.2, follow="off")
    print("GAIT host walk, slope 0.2, level targets:", r)
    assert r["first_bad"] is not None and r["first_bad"] < 600
