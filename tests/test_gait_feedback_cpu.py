"""The gait planner's foot-placement feedback (include/wbc_gait_feedback.h) without a GPU: the host instantiation of
csrc/wbc_gait_feedback.hpp (tools/host_gait_feedback.cpp through tests/host_gait_feedback.py) against the numpy restatement of the
header (tests/gait_feedback_oracle.py) in double and in extended precision, the law's exact relations on both, damaged instances,
what the C ABI refuses before any device is touched, the binding, the twin under the sanitizers as a stand-alone program, and ID
walking on the host twins with the pass after the gait.  Measured figures: profiles/r16/gait_feedback.md."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import gait_feedback_oracle as gfo
import gait_oracle as go
import host_gait as hg
import host_gait_feedback as hgf
import host_gait_schedule as hgs
import test_gait_cpu as tgc
from quadruped_drake_amd import gait, workloads

ROOT = tgc.ROOT
FELL, BAD = tgc.FELL, tgc.BAD
N, TICKS, DT = 9, 400, 2.5e-3
POS = [18 + 9 * f + k for f in range(4) for k in range(2)]
GROUPS = (("positions", POS), ("velocities", [r + 3 for r in POS]), ("accelerations", [r + 6 for r in POS]))
# the twin test's parameters: a position gain as well, and a d_max that the perturbation below crosses on part of the run
PAR = dict(k_v=math.sqrt(0.3 / 9.81), k_p=0.5, d_max=0.05, u_hold=0.5)


# ---- the two engines behind one face
class Twin:
    name = "twin"

    def __init__(self, n):
        self.st = hgf.State(n)

    def step(self, par, P, names, t, q, v, tg, mask, gid, sc):
        rows, off = hgf.run(names, par, t, q, v, tg.copy(), mask, self.st, gid, sc, p=P)
        return rows, off

    def packed(self):
        return self.st.state.copy(), self.st.prev.copy()


class Oracle:
    name = "oracle"

    def __init__(self, n, dtype=np.float64):
        self.st, self.dtype = gfo.State(n, dtype), dtype

    def step(self, par, P, names, t, q, v, tg, mask, gid, sc):
        rows, off, self.decisions, self.near, self.skipped = gfo.step(par, P, [gait.stride(x) for x in names], t, q, v, tg, mask, self.st, gid, sc,
                                                                      dtype=self.dtype)
        return rows, off

    def packed(self):
        return self.st.packed(), self.st.prev.copy()


ENGINES = [Twin, Oracle]


def sequence(name, ticks=TICKS, n=N, scales=(0.4, 1.2), seed=3):
    """The twin test's inputs for one stride: n instances with their own command (test_gait_cpu.COMMANDS), stride scale (spread over
    `scales`) and wait (the handle's wait_time is 0.25 s; instance i's clock is shifted by 0.03 i s), `ticks` ticks of 2.5 ms, off every
    boundary by test_gait_cpu's 0.1234 ms; and a perturbation of the measured trunk: three sinusoids per component, amplitudes drawn
    from `seed` and scaled so that their sum reaches 0.05 m in position and 0.3 m/s in velocity.
    -> (P, cmd [3, n], sc [n], times [ticks, n], dq [ticks, 2, n], dv [ticks, 2, n])"""
    P = hg.params(wait_time=0.25)
    i = np.arange(n)
    cmd = np.array(tgc.COMMANDS)[i % len(tgc.COMMANDS)].T.copy()
    sc = np.linspace(scales[0], scales[1], n)
    times = (np.arange(ticks)[:, None] * DT + tgc.OFFSET) + 0.2 - 0.03 * i[None, :]
    rng = np.random.default_rng([seed, sum(map(ord, name))])
    amp = rng.uniform(0.5, 1.0, (2, 2, 3, n))
    amp /= amp.sum(2, keepdims=True)
    freq, ph = rng.uniform(0.7, 9.0, (2, 2, 3, n)), rng.uniform(0, 2 * math.pi, (2, 2, 3, n))
    wave = (amp[None] * np.sin(2 * math.pi * freq[None] * times[:, None, None, None, :] + ph[None])).sum(3)   # [ticks, 2, 2, n]
    return P, cmd, sc, times, 0.05 * wave[:, 0], 0.3 * wave[:, 1]


def measured(tg, dq, dv):
    """q [19, n], v [18, n]: the plan's trunk plus the perturbation in (x, y); the rest of a state the pass does not read"""
    n = tg.shape[1]
    q, v = np.zeros((19, n)), np.zeros((18, n))
    q[0] = 1.0; q[6] = 0.3
    q[4:6] = tg[0:2] + dq
    v[3:5] = tg[3:5] + dv
    return q, v


def run_three(name, par, ticks, schedule=None, scales=(0.4, 1.2)):
    """The twin, the oracle in double and the oracle in extended precision over sequence(name), all three fed with the rows and mask the
    gait's twin wrote (the pass is what is compared; the gait has its own tests).  An instance leaves the comparison at its first
    near-tie: the oracle's two runs disagree on a decision, or u within 1e-9 of u_hold, or |d_raw| within 1e-9 of d_max.
    -> dict(bar, worst: per group; left: instance-ticks left out; clamp: fraction of the compared instance-ticks on which the clamp binds;
    lifts: lift-offs + touch-downs per foot over the batch; bound: the largest |cur|, |to| / d_max)"""
    P, cmd, sc, times, dq, dv = sequence(name, ticks, scales=scales)
    n = cmd.shape[1]
    eng = [Twin(n), Oracle(n), Oracle(n, np.longdouble)]
    alive = np.ones(n, bool)
    bar, worst = {g: 0.0 for g, _ in GROUPS}, {g: 0.0 for g, _ in GROUPS}
    left = clamp = compared = 0
    edges, bound = np.zeros(4, int), 0.0
    prev = np.full(n, 0xF, np.uint8)
    for k in range(ticks):
        if schedule is None:
            tg, mask = hg.run([name], times[k], cmd, None, sc, None, p=P)
        else:
            tg, mask = hgs.run([name], times[k], cmd, *schedule, None, sc, None, p=P)
        q, v = measured(tg, dq[k], dv[k])
        (rt, ot), (rd, od), (rw, ow) = (e.step(par, P, [name], times[k], q, v, tg, mask, None, sc) for e in eng)
        tie = (eng[1].decisions != eng[2].decisions).any(1) | eng[1].near | eng[2].near
        alive &= ~tie
        left += int((~alive).sum())
        st = [e.packed() for e in eng]
        assert (st[0][1] == st[1][1]).all() and (st[1][1] == mask).all()
        for g, rows in GROUPS:
            sets = [(rt[rows], rd[rows], rw[rows])]
            if g == "positions":
                sets += [(ot, od, ow), (st[0][0].reshape(6, n, 4), st[1][0].reshape(6, n, 4), st[2][0].reshape(6, n, 4))]
            for a, b, w in sets:
                sel = (slice(None), alive) + ((slice(None),) if a.ndim == 3 else ())
                if alive.any():
                    bar[g] = max(bar[g], float(np.abs(b[sel] - w[sel]).max()))
                    worst[g] = max(worst[g], float(np.abs(a[sel] - w[sel]).max()))
        clamp += int(eng[1].decisions[alive, 0].sum()); compared += int(alive.sum())
        for f in range(4):
            edges[f] += int((((mask >> f) & 1) != ((prev >> f) & 1)).sum())
        prev = mask
        bound = max(bound, float(np.abs(st[0][0]).max()) / par["d_max"], float(np.abs(st[1][0]).max()) / par["d_max"])
        # the offsets' norm, not their components, is what the law bounds
        for s in (st[0][0], st[1][0]):
            for r0 in (0, 4):
                assert float(np.hypot(s[r0], s[r0 + 1]).max()) <= par["d_max"] * (1 + 4 * 2.0**-52)
    return dict(bar={g: 4 * x for g, x in bar.items()}, worst=worst, left=left, clamp=clamp / max(compared, 1), lifts=edges, bound=bound, total=n * ticks)


@pytest.mark.parametrize("name", list(gait.STRIDES))
def test_host_twin_matches_the_oracle_on_every_stride(name):
    """9 instances, 400 ticks of 2.5 ms, rows, offsets and state at every tick.  The bar is 4 x the largest difference between the
    oracle in double and in extended precision on these inputs (the twin may round where the oracle does, in another order: the swing's
    polynomials are nested there and written in powers here).  At most 2 % of the instance-ticks are left out after a near-tie; the
    clamp binds on part of the compared ticks and not on all.  Measured over the ten strides (profiles/r16/gait_feedback.md): bars
    4.8e-16 .. 7.6e-16 m, 1.9e-15 .. 3.6e-14 m/s, 3.2e-14 .. 7.3e-12 m/s^2; the twin's worst 0.16 .. 0.28 of its bar; 0 instance-ticks
    left out on every stride; the clamp binds on 7.5 .. 13.8 % of them."""
    r = run_three(name, PAR, TICKS)
    print("GAIT-FEEDBACK twin-to-oracle %-12s left out %d of %d, clamp binds on %.3f, edges per foot %s" % (name, r["left"], r["total"], r["clamp"], r["lifts"]))
    for g, _ in GROUPS:
        print("GAIT-FEEDBACK twin-to-oracle %-12s %-13s worst %.3g bar %.3g" % (name, g, r["worst"][g], r["bar"][g]))
    assert r["left"] <= 0.02 * r["total"]
    assert 0.0 < r["clamp"] < 1.0
    if name != "stand":
        assert (r["lifts"] >= 4).all()                              # every foot lifted and landed at least twice over the batch
    for g, _ in GROUPS:
        if name == "stand":
            assert r["worst"][g] == 0.0 and r["bar"][g] == 0.0     # no foot ever swings: the offsets stay zero
        else:
            assert r["bar"][g] > 0 and r["worst"][g] <= r["bar"][g], (name, g, r["worst"][g], r["bar"][g])


# ---- exact relations
def _walk(Engine, name, par, ticks, measure, schedule=None, scales=(0.4, 1.2), each=None):
    """`ticks` calls of Engine's pass over sequence(name); measure(k, tg) -> (q, v).  each(k, tg, mask, rows, off, engine) after every call."""
    P, cmd, sc, times, dq, dv = sequence(name, ticks, scales=scales)
    e = Engine(cmd.shape[1])
    for k in range(ticks):
        if schedule is None:
            tg, mask = hg.run([name], times[k], cmd, None, sc, None, p=P)
        else:
            tg, mask = hgs.run([name], times[k], cmd, *schedule, None, sc, None, p=P)
        q, v = measure(k, tg, dq[k], dv[k])
        rows, off = e.step(par, P, [name], times[k], q, v, tg, mask, None, sc)
        if each:
            each(k, tg, mask, rows, off, e)
    return e


@pytest.mark.parametrize("Engine", ENGINES, ids=lambda e: e.name)
def test_zero_gains_or_a_measurement_on_the_plan_change_no_bit(Engine):
    def same(k, tg, mask, rows, off, e):
        assert (rows == tg).all() and (off == 0).all() and (e.packed()[0] == 0).all()

    for name in ("trot", "walk", "gallop"):
        _walk(Engine, name, dict(PAR, k_v=0.0, k_p=0.0), 200, lambda k, tg, dq, dv: measured(tg, dq, dv), each=same)
        _walk(Engine, name, PAR, 200, lambda k, tg, dq, dv: measured(tg, 0.0, 0.0), each=same)


@pytest.mark.parametrize("Engine", ENGINES, ids=lambda e: e.name)
def test_a_constant_velocity_error_puts_every_stance_foot_at_the_clamped_gain_times_it(Engine):
    """k_p = 0, commands without a yaw rate, past the ramp: v - pd is then the same bits on every tick, and once every foot has
    completed a swing each stance offset is clamp(k_v e_v) to the last bit.  Some of instances 0 .. 3 stay under d_max = 0.025 m, 5 .. 8 are clamped."""
    par = dict(PAR, k_p=0.0, d_max=0.025)
    n = N
    e_v = np.stack([0.05 * (np.arange(n) - 3.0), 0.02 * (np.arange(n) + 1.0)])
    P = hg.params(wait_time=0.0)
    cmd = np.stack([0.1 + 0.05 * np.arange(n), 0.02 * np.arange(n) - 0.05, np.zeros(n)])
    sc = np.linspace(0.4, 0.6, n)
    for name in ("trot", "walk", "pace"):
        e = Engine(n)
        for k in range(700):
            t = np.full(n, 0.6 + k * DT + tgc.OFFSET)
            tg, mask = hg.run([name], t, cmd, None, sc, None, p=P)
            q, v = measured(tg, 0.0, e_v)
            rows, off = e.step(par, P, [name], t, q, v, tg, mask, None, sc)
        want, m = gfo.offset(par, q, v, tg)
        assert (m[:4] < par["d_max"]).any() and (m[5:] > par["d_max"]).all()
        seen = 0
        for f in range(4):
            down = ((mask >> f) & 1).astype(bool)
            assert (off[2 * f:2 * f + 2, down] == want[:, down]).all(), (name, f)
            seen += int(down.sum())
        assert seen >= n                                                    # feet on the ground were compared


def _edge_times(name, scale, strides=(2, 3)):
    return sorted((x, f) for f, _, a, b in tgc._run_times(name, scale, strides) for x in (a, b))


@pytest.mark.parametrize("Engine", ENGINES, ids=lambda e: e.name)
def test_feet_stay_continuous_across_every_lift_off_and_touch_down_under_a_constant_error(Engine):
    """Position, velocity and acceleration of every foot eps either side of every boundary of its runs, with the pass called tick by tick
    up to there (5 ms ticks, then boundary - eps, boundary + eps) and a measurement that is the plan plus a constant: the bars of
    test_gait_cpu's continuity test, 1e-12 + 1e-14 m, 1e-12 m/s and 1e-3 m/s^2.  Those bars were derived for eps = 1e-9 s (u = eps / D
    with D >= 0.05 s: the swing's own velocity step is (30 L + 192 h) u^2 / D, which is 4e-13 at 1e-9 s and 4e-9 at 1e-7 s), so they are
    held at eps = 1e-9 s, as there; at 1e-7 s the same polynomial bounds give 1e-8 m/s and 1e-1 m/s^2, which are asserted as well.
    Measured, with the pass and for the gait alone alike: 1.1e-15 m, 7.7e-14 m/s, 1.5e-4 m/s^2 at 1e-9 s; 4.4e-16 m, 7.7e-10 m/s,
    1.5e-2 m/s^2 at 1e-7 s (the swing's own z rows set both)."""
    P = hg.params()
    par = dict(PAR, k_p=0.0, d_max=0.10)
    cmd1, e_v = (0.5, 0.1, 0.4), np.array([[0.25], [-0.15]])
    for eps, bars in ((1e-9, (1e-12 + 1e-14, 1e-12, 1e-3)), (1e-7, (1e-12 + 1e-14, 1e-8, 1e-1))):
        for name in gait.STRIDES:
            if name == "stand":
                continue
            scale = 0.5
            edges = _edge_times(name, scale)
            e = Engine(1)
            cmd, sc = np.array(cmd1)[:, None], np.array([scale])
            now, checked = 0.0, 0

            def call(t):
                tg, mask = hg.run([name], np.array([t]), cmd, None, sc, None, p=P)
                q, v = measured(tg, 0.0, e_v)
                return e.step(par, P, [name], np.array([t]), q, v, tg, mask, None, sc)[0], mask

            for tb, f in edges:
                while now < tb - 2.5e-3:
                    call(now + 1.234e-4)
                    now += 5e-3
                (lo, mlo), (hi, mhi) = call(tb - eps), call(tb + eps)
                r = 18 + 9 * f
                d = np.abs(hi[r:r + 9, 0] - lo[r:r + 9, 0])
                assert d[0:3].max() < bars[0] and d[3:6].max() < bars[1] and d[6:9].max() < bars[2], (name, f, tb, eps, d)
                checked += ((mlo[0] >> f) & 1) != ((mhi[0] >> f) & 1)
            assert checked == len(edges)
            assert float(np.abs(e.packed()[0]).max()) > 0.02                # and the offsets were not nothing


@pytest.mark.parametrize("Engine", ENGINES, ids=lambda e: e.name)
def test_under_a_schedule_the_pass_adds_the_same_offsets(Engine):
    """m = 3 switches, blend 0.5: the same errors give the offsets of the walk without a schedule.  The pass forms its errors as
    measured - planned, and the planned body differs between the two walks, so the two errors differ by the rounding of a sum and a
    difference of numbers below 4 (2 x 2^-51 each); through k_v + k_p < 1 and the offset's own roundings that is below 1e-15."""
    par = dict(PAR, d_max=0.04)
    name, ticks = "trot", 400
    n = N
    m = np.full(n, 3, np.uint8)
    when = np.zeros((7, n)); when[0], when[1], when[2] = 0.05, 0.25, 0.5
    cmds = np.zeros((21, n)); cmds[0], cmds[3], cmds[5], cmds[6] = 0.4, 0.2, 0.5, -0.3
    offs = {}
    for key, schedule in (("plain", None), ("schedule", (m, when, cmds, 0.15))):
        got = []
        _walk(Engine, name, par, ticks, lambda k, tg, dq, dv: measured(tg, dq, dv), schedule=schedule,
              each=lambda k, tg, mask, rows, off, e: got.append((off.copy(), tg[0:2].copy(), e.decisions[:, 0].copy() if hasattr(e, "decisions") else None)))
        offs[key] = got
    moved = max(float(np.abs(a[1] - b[1]).max()) for a, b in zip(offs["plain"], offs["schedule"]))
    assert moved > 0.05                                                    # the schedule did steer the body elsewhere
    # an instance leaves at a tick where |d_raw| is within 1e-9 of d_max: the clamp may then bind in one walk and not in the other
    P, cmd, sc, times, dq, dv = sequence(name, ticks)
    alive = np.ones(n, bool)
    worst = 0.0
    for k, (a, b) in enumerate(zip(offs["plain"], offs["schedule"])):
        raw = par["k_v"] * dv[k] + par["k_p"] * dq[k]
        alive &= np.abs(np.hypot(raw[0], raw[1]) - par["d_max"]) > 1e-9
        worst = max(worst, float(np.abs(a[0][:, alive] - b[0][:, alive]).max()))
    print("GAIT-FEEDBACK %s: offsets with and without a schedule differ by at most %.3g; %d of %d instances compared to the end" % (Engine.name, worst, alive.sum(), n))
    assert alive.sum() >= n - 1 and worst < 1e-15


# ---- damage
DAMAGE = [("q4", math.nan), ("q5", math.inf), ("v3", -math.inf), ("v4", math.nan), ("p0", math.nan), ("p1", math.inf), ("pd0", math.nan),
          ("pd1", -math.inf), ("time", math.nan), ("time", math.inf), ("gait_id", 200), ("row", math.nan)]


@pytest.mark.parametrize("Engine", ENGINES, ids=lambda e: e.name)
def test_a_damaged_instance_is_left_as_it_is_and_its_neighbours_keep_their_bits(Engine):
    """One instance of 9, on tick 150 of a trot: NaN or inf in each of the eight trunk numbers, in the time, NaN rows through a gait_id
    past the table, and a NaN in one foot row.  Its rows, state and previous mask are bit for bit what they were; the other eight are
    those of the undamaged batch on that tick and on the next 50."""
    name, hit, at = "trot", 4, 150
    P, cmd, sc, times, dq, dv = sequence(name, at + 51)
    n = N
    gid0 = np.zeros(n, np.uint8)

    def tick(e, k, damage=None):
        t, gid = times[k].copy(), gid0.copy()
        if damage and damage[0] == "time":
            t[hit] = damage[1]
        if damage and damage[0] == "gait_id":
            gid[hit] = damage[1]
        tg, mask = hg.run([name], t, cmd, gid, sc, None, p=P)
        q, v = measured(np.where(np.isfinite(tg), tg, 0.0), dq[k], dv[k])
        if damage:
            where = {"q4": (q, 4), "q5": (q, 5), "v3": (v, 3), "v4": (v, 4), "p0": (tg, 0), "p1": (tg, 1), "pd0": (tg, 3), "pd1": (tg, 4), "row": (tg, 31)}
            if damage[0] in where:
                a, r = where[damage[0]]
                a[r, hit] = damage[1]
        rows, off = e.step(PAR, P, [name], t, q, v, tg, mask, gid, sc)
        return tg, rows, off

    base = Engine(n)
    for k in range(at):
        tick(base, k)
    clean = Engine(n)
    clean.st = base.st.copy()
    ref = [(tick(clean, k), clean.packed()) for k in range(at, at + 51)]
    others = np.arange(n) != hit
    for damage in DAMAGE:
        e = Engine(n)
        e.st = base.st.copy()
        s0, p0 = e.packed()
        tg, rows, off = tick(e, at, damage)
        s1, p1 = e.packed()
        assert rows[:, hit].tobytes() == tg[:, hit].tobytes() and np.isnan(off[:, hit]).all(), damage
        assert s1.reshape(6, n, 4)[:, hit].tobytes() == s0.reshape(6, n, 4)[:, hit].tobytes() and p1[hit] == p0[hit], damage
        for j, k in enumerate(range(at, at + 51)):
            if j:
                tg, rows, off = tick(e, k)
            (_, rrows, roff), (rs, rp) = ref[j]
            assert rows[:, others].tobytes() == rrows[:, others].tobytes() and off[:, others].tobytes() == roff[:, others].tobytes(), (damage, k)
            s, p = e.packed()
            assert s.reshape(6, n, 4)[:, others].tobytes() == rs.reshape(6, n, 4)[:, others].tobytes() and (p[others] == rp[others]).all(), (damage, k)


# ---- what returns before any device is touched, and the binding
def test_abi_gait_feedback_misuse_without_device():
    from quadruped_drake_amd import _lib
    L = _lib.lib()
    err = lambda: L.wbc_last_error().decode()
    P = hg.params()
    cp = gait.c_params(P["stance"], P["height"], P["swing_height"], P["ramp_time"], P["wait_time"])
    fp = _lib.WbcGaitFeedbackParams()
    assert L.wbc_gait_feedback_params_default(C.byref(cp), C.byref(fp)) == 0
    assert (fp.k_v, fp.k_p, fp.d_max, fp.u_hold) == (math.sqrt(P["height"] / 9.81), 0.0, 0.10, 0.5) and gfo.defaults(P["height"])["k_v"] == fp.k_v
    assert L.wbc_gait_feedback_params_default(None, C.byref(fp)) < 0 and "null" in err()
    assert L.wbc_gait_feedback_params_default(C.byref(cp), None) < 0 and "null" in err()
    assert L.wbc_gait_feedback_check(C.byref(fp)) == 0
    assert L.wbc_gait_feedback_check(None) < 0 and "null params" in err()
    h = C.c_void_p()
    assert L.wbc_gait_create(C.byref(cp), gait.c_strides(["trot"]), 1, 0, C.byref(h)) == 0
    for field, values in (("k_v", (-0.1, math.nan, math.inf)), ("k_p", (-1.0, math.nan, math.inf)), ("d_max", (0.0, -0.1, math.nan, math.inf)),
                          ("u_hold", (-0.1, 1.5, math.nan, math.inf))):
        for x in values:
            bad = _lib.WbcGaitFeedbackParams(fp.k_v, fp.k_p, fp.d_max, fp.u_hold)
            setattr(bad, field, x)
            assert L.wbc_gait_feedback_check(C.byref(bad)) < 0 and field in err() and "wbc_gait_feedback_check" in err(), (field, x)
            assert L.wbc_gait_set_feedback(h, C.byref(bad), 4) < 0 and field in err() and "wbc_gait_set_feedback" in err()
    for u in (0.0, 1.0):
        ok = _lib.WbcGaitFeedbackParams(0.0, 0.0, 1e-3, u)
        assert L.wbc_gait_feedback_check(C.byref(ok)) == 0
    assert L.wbc_gait_set_feedback(None, C.byref(fp), 4) < 0 and "null gait handle" in err()
    assert L.wbc_gait_set_feedback(h, None, 4) < 0 and "null params" in err()
    for n in (0, -1, (1 << 24) + 1):
        assert L.wbc_gait_set_feedback(h, C.byref(fp), n) < 0 and "n out of range" in err()
    assert L.wbc_gait_clear_feedback(None) < 0 and "null gait handle" in err()
    assert L.wbc_gait_clear_feedback(h) == 0                                       # nothing set: nothing to clear
    assert L.wbc_gait_feedback_kernel_info(None, None, None, None, None) < 0 and "null gait handle" in err()
    buf, tm, mk, q, v, off = np.zeros((54, 4)), np.zeros(4), np.zeros(4, np.uint8), np.zeros((19, 4)), np.zeros((18, 4)), np.zeros((8, 4))
    p = lambda a: C.c_void_p(a.ctypes.data)
    f = L.wbc_gait_targets_measured
    assert f(None, None, 4, 4, p(tm), p(q), p(v), p(buf), p(mk), p(off)) < 0 and "null gait handle" in err()
    for n, ld, what in ((-1, 4, "n out of range"), ((1 << 24) + 1, 1 << 25, "WBC_MAX_LD"), (4, 3, "ld must be >= n"), (4, (1 << 24) + 1, "WBC_MAX_LD")):
        assert f(h, None, n, ld, p(tm), p(q), p(v), p(buf), p(mk), p(off)) < 0 and what in err() and "wbc_gait_targets_measured" in err(), (n, ld, err())
    for k in range(5):
        args = [p(tm), p(q), p(v), p(buf), p(mk)]
        args[k] = None
        assert f(h, None, 4, 4, *args, p(off)) < 0 and "are required" in err()
    assert f(h, None, 4, 4, p(tm), p(q), p(v), p(buf), p(mk), None) < 0 and "wbc_gait_set_commands" in err()   # offsets are optional
    assert (buf == 0).all() and (mk == 0).all() and (off == 0).all()
    assert L.wbc_gait_destroy(h) == 0
    # the Python layer's own checks
    g = object.__new__(gait.GaitPlanner)
    g._n = g._h = None
    with pytest.raises(ValueError, match="set_commands"):
        g.targets_measured(None, None, None)
    g2 = object.__new__(gait.GaitPlanner)
    g2._L, g2._h, g2.params = L, None, cp
    with pytest.raises(ValueError, match="unknown parameter"):
        g2.set_feedback(4, gain=1.0)
    assert g2.feedback_defaults() == gfo.defaults(P["height"]) and not g2.has_feedback


def test_the_twin_runs_clean_under_the_sanitizers_as_a_stand_alone_program(tmp_path):
    """tools/host_gait_feedback_check.cpp + tools/host_gait_feedback.cpp + tools/host_gait.cpp built with -fsanitize=address,undefined (no
    recovery) and run: a walk of every kind of instance, zero gains, a constant error, damage, arrays exactly as long as the batch."""
    exe = tmp_path / "check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "include"), "-o", str(exe), os.path.join(ROOT, "tools", "host_gait_feedback_check.cpp"), os.path.join(ROOT, "tools", "host_gait_feedback.cpp"),
                    os.path.join(ROOT, "tools", "host_gait.cpp")], check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "0 things out of place" in r.stdout and not r.stderr


def test_simulate_gait_feedback_and_push_arguments():
    from quadruped_drake_amd import simulate
    base = ["--planner", "gait", "--plant", "ground"]
    a = simulate.parse(base)
    assert a.gait_feedback is None and a.push is None
    assert simulate.parse(base + ["--gait-feedback"]).gait_feedback == {}
    a = simulate.parse(base + ["--gait-feedback", "0.2,0.5,0.08,0.8", "--push", "1.5:1.6:0,20"])
    assert a.gait_feedback == dict(k_v=0.2, k_p=0.5, d_max=0.08, u_hold=0.8) and a.push == (1.5, 1.6, 0.0, 20.0)
    assert simulate.parse(["--plant", "ground", "--push", "0:0.1:5,-5"]).push == (0.0, 0.1, 5.0, -5.0)
    for argv in (["--gait-feedback"], base + ["--gait-feedback", "0.2,0.5,0.08"], base + ["--gait-feedback", "0.2,0.5,0,0.5"],
                 base + ["--gait-feedback", "0.2,0.5,0.1,1.5"], base + ["--gait-feedback", "-0.2,0.5,0.1,0.5"], base + ["--gait-feedback", "a,b,c,d"],
                 base + ["--terrain", "ramp_step:0.1", "--gait-terrain", "fit", "--gait-feedback"],
                 ["--planner", "gait", "--plant", "rigid", "--push", "1:2:0,20"], base + ["--push", "2:1:0,20"], base + ["--push", "1:2:20"],
                 base + ["--push", "1:2"], base + ["--push", "x"]):
        with pytest.raises(SystemExit):
            simulate.parse(argv)
    assert "--gait-feedback" in simulate.__doc__ and "--push" in simulate.__doc__


# ---- the closed loop on the host twins
GRID = [10.0 * math.sqrt(2.0) ** k for k in range(12)]          # the pushes' forces [N]: factor sqrt(2) from 10 N up
PUSH_TICKS = (300, 320)


def host_walk(cmd, forces=(0.0,), par=None, ticks=600, dt=5e-3, scale=0.5, model="mini_cheetah", push=PUSH_TICKS):
    """test_gait_cpu.host_walk's loop on the plane with the pass after the gait, for a batch: instance i is pushed with the lateral force
    forces[i] [N] (row 4 of ext_wrench) during the ticks `push`.  gait (host_gait) -> feedback (host_gait_feedback; par None: none) ->
    tick (host_tick, ID) -> ground step (host_ground).  Trot at stride scale `scale`, GaitPlanner's defaults.
    -> dict(flags [n]: OR of the plant's flags, first [n]: the first tick with FELL or BAD (-1: none), status: ticks x instances with a
    non-zero status, dx, dy [n]: the final trunk's offset from the planned body position, height [n], reach: the largest offset the pass
    applied)"""
    import host_ground as hgr
    import host_tick as hk
    from quadruped_drake_amd.controller import load_model
    forces = np.asarray(forces, dtype=np.float64)
    n = forces.size
    t = load_model(model)
    q, v = workloads.nominal_state(model, n)
    P = hg.params(model)
    c = np.tile(np.array(cmd, dtype=np.float64)[:, None], (1, n))
    sc = np.full(n, scale)
    st = hgf.State(n)
    flags, first, status, reach = np.zeros(n, np.int64), np.full(n, -1), 0, 0.0
    for k in range(ticks):
        tm = np.full(n, k * dt)
        tg, mask = hg.run(["trot"], tm, c, None, sc, None, p=P)
        if par is not None:
            tg, off = hgf.run(["trot"], par, tm, q, v, tg, mask, st, None, sc, p=P)
            if np.isfinite(off).any():
                reach = max(reach, float(np.nanmax(np.abs(off))))
        tau, _, s, _ = hk.run("id", t["flat"], q, v, tg, mask, act_perm=t.get("act_perm"))
        w = np.zeros((6, n))
        if push[0] <= k < push[1]:
            w[4] = forces
        o = hgr.run(t["flat"], q, v, tau, act_perm=t.get("act_perm"), dt=dt, ext_wrench=w)
        q, v = o["q"], o["v"]
        flags |= o["flags"]
        first = np.where((first < 0) & ((o["flags"] & (FELL | BAD)) != 0), k, first)
        status += int((s != 0).sum())
    plan = go.targets(P, [gait.stride("trot")], np.full(n, ticks * dt), c, None, sc)[0]
    return dict(flags=flags, first=first, status=status, dx=q[4] - plan[0], dy=q[5] - plan[1], height=q[6].copy(), reach=reach)


def survived(flags):
    """the largest grid force survived with every smaller one survived too (0.0: not even the first), from the flags of GRID's pushes"""
    ok = (np.asarray(flags) & (FELL | BAD)) == 0
    k = 0
    while k < len(ok) and ok[k]:
        k += 1
    return GRID[k - 1] if k else 0.0


@pytest.mark.parametrize("cmd", [w[0] for w in tgc.WALKS[:3]], ids=["forward", "backward", "arc"])
def test_id_walks_unpushed_with_the_default_feedback_on_the_host_twins(cmd):
    """Mini Cheetah, ID, dt 5 ms, trot at stride scale 0.5, 600 ticks, wbc_gait_feedback_params_default: no FELL, no BAD, status 0 on
    every tick, the trunk within 0.03 m of the planned body position and its height within 5 mm of 0.3 m -- test_gait_cpu's bars for
    the gait without feedback.  Measured, dx and dy off the plan with feedback (without): forward +1.4 mm, +3.2 mm (+1.1, +2.2);
    backward +3.8 mm, +18.1 mm (+2.3, +5.8); the arc -0.1 mm, -0.0 mm (-0.8, +0.7); the pass moved a foothold by at most 4.2 mm,
    16.1 mm and 7.9 mm.

    The pushed walks are not asserted.  The sweep the issue asks for (host_walk over GRID, a lateral push during ticks 300 .. 319) gave
    F_off = 14.1 N and F_on = 14.1 N with the defaults, and no pair of k_v in {0.5, 1, 1.5} sqrt(h / g) and u_hold in {0.5, 0.8} did
    better (three did worse: 10 N, 10 N and none): the law as it stands does not extend the survivable push, and the defaults stay the
    first guesses (profiles/r16/gait_feedback.md has the table)."""
    par = gfo.defaults(workloads.NOMINAL_HEIGHT["mini_cheetah"])
    r, plain = host_walk(cmd, par=par), host_walk(cmd)
    print("GAIT-FEEDBACK host walk cmd %s: dx %+.4f dy %+.4f height %.4f flags %d status %d reach %.4f; without feedback dx %+.4f dy %+.4f" %
          (cmd, r["dx"][0], r["dy"][0], r["height"][0], r["flags"][0], r["status"], r["reach"], plain["dx"][0], plain["dy"][0]))
    assert not r["flags"][0] & (FELL | BAD) and r["status"] == 0
    assert math.hypot(r["dx"][0], r["dy"][0]) < 0.03 and abs(r["height"][0] - 0.3) < 5e-3
    assert r["reach"] > 0                                                   # the pass did move footholds
