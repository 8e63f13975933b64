"""The gait planner's terrain (include/wbc_gait_terrain.h), no GPU: the host instantiation of the TERRAIN law of
csrc/wbc_gait.hpp (tests/host_gait_terrain.py) against the numpy restatement of the header's sentences (tests/gait_terrain_oracle.py),
relations that need no oracle, the clearance of every swing over random profiles, continuity and central differences, malformed
instances, the argument checks that return before any device is touched, the binding table against the header, and the closed loop
on the host twins: ID walking over a kerb of 0.10 m, stairs of 0.08 m and a yawed kerb on an arc -- and raising BAD on that kerb with
the plain gait and followed targets.

The bars of the comparison with the oracle are measured here, per kind of row: 100 x the largest difference between the oracle in
double and in extended precision on the same inputs ("GAIT-TERRAIN ..." lines print them; profiles/r14/gait_terrain.md keeps them)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import follow_oracle as fo
import gait_oracle as go
import gait_terrain_oracle as gto
import host_gait as hg
import host_gait_terrain as hgt
import plant_edges as pe
import test_gait_cpu as tgc
from quadruped_drake_amd import gait, terrain as tr

ROOT = tgc.ROOT
XYZ = [0, 1, 2] + [18 + 9 * f + k for f in range(4) for k in range(3)]
GROUPS = (("positions", XYZ), ("velocities", [r + 3 for r in XYZ]), ("accelerations", [r + 6 for r in XYZ]), ("attitude", [9, 10, 11]),
          ("attitude rates", [12, 13, 14, 15, 16, 17]))
ZROWS = [2, 5, 8] + [18 + 9 * f + 3 * d + 2 for f in range(4) for d in range(3)]
NEAR = 1e-9
# 0.45 is at least 0.03 from |scale x slope| of every piece of the sixteen profiles at every scale of SCALES (asserted below): whether a
# piece is steep is then no matter of rounding
MAX_GRADE = 0.45


def sixteen():
    """(profiles, terrain_id, terrain_scale) dealt over a batch: follow_oracle's sixteen profiles -- flat, slopes, a kerb, stairs, a
    ridge, a full table of eight knots, yawed and shifted copies -- at the scales 1, 0, -0.7 and 2.5"""
    profiles = fo.sixteen_profiles()
    return profiles, (lambda n: (np.arange(n) % 16).astype(np.uint8)), (lambda n: np.array(fo.SCALES)[(np.arange(n) // 16) % 4].copy())


def test_no_piece_of_the_test_profiles_is_steep_by_a_rounding():
    for p in fo.sixteen_profiles():
        for j in range(len(p.s) - 1):
            for scale in fo.SCALES:
                assert abs(abs(scale * (p.h[j + 1] - p.h[j]) / (p.s[j + 1] - p.s[j])) - MAX_GRADE) > 1e-3, (p, j, scale)


@pytest.mark.parametrize("name", list(gait.STRIDES))
def test_host_twin_matches_the_oracle_on_every_stride_and_profile(name):
    """All ten strides on the sixteen profiles at four scales (negative and zero included), both body modes, test_gait_cpu's nine
    commands, five stride scales and four starts, 2739 samples over 20 s and 24 with tau < 0.  A sample is left out only where a
    foothold's s lies within 1e-9 of a knot, of an end of a forbidden interval or of the tie between the two ends -- at most 1 %."""
    P = hg.params(wait_time=0.25)
    S = [gait.stride(name)]
    profiles, ids, scales = sixteen()
    for body, shift in (("fit", 0), ("lift", 4)):
        tp = gto.tparams(body=body, max_grade=MAX_GRADE)
        t, cmd, sc, st = tgc.sample_batch(shift, P["wait_time"])
        tid, tsc = ids(t.size), scales(t.size)
        assert float(go.boundary_distance(S[0][0], t, P["wait_time"], sc)[24:].min()) >= 1e-9
        got, gmask = hgt.run([name], profiles, t, cmd, None, sc, st, tid, tsc, tp=tp, p=P)
        info = {}
        want, wmask = gto.targets(P, S, tp, profiles, t, cmd, None, sc, st, tid, tsc)
        wide, lmask = gto.targets(P, S, tp, profiles, t, cmd, None, sc, st, tid, tsc, dtype=np.longdouble, info=info)
        keep = np.asarray(info["near"] >= NEAR)
        print("GAIT-TERRAIN twin-to-oracle %-12s %-4s left out %d of %d" % (name, body, int((~keep).sum()), t.size))
        assert (~keep).sum() <= 0.01 * t.size
        assert (gmask == wmask).all() and (wmask == lmask).all()                       # masks: on every sample
        assert (gmask[:24] == 0xF).all() and np.isfinite(got).all()
        for group, rows in GROUPS:
            bar = 100.0 * float(np.abs(want[rows][:, keep] - wide[rows][:, keep]).max())
            worst = float(np.abs(got[rows][:, keep] - wide[rows][:, keep]).max())
            print("GAIT-TERRAIN twin-to-oracle %-12s %-4s %-14s worst %.3g bar %.3g" % (name, body, group, worst, bar))
            if body == "lift" and group != "attitude" and group.startswith("attitude"):
                assert (got[[12, 13, 15, 16]] == 0).all()
            assert bar > 0 and worst < bar, (name, body, group, worst, bar)
        if body == "lift":
            assert (got[9:11] == 0).all()
        elif name != "stand":
            assert np.abs(got[9:11]).max() > 0.05                                       # the fit turned the trunk
    if name != "stand":
        plain = hg.run([name], t, cmd, None, sc, st, p=P)[0]
        assert np.abs(got[ZROWS] - plain[ZROWS]).max() > 0.04                            # and the terrain did something


# ---- exact relations, on the oracle and on the twin
def _twin(P, S, tp, profiles, t, cmd, sc=None, st=None, tid=None, tsc=None):
    return hgt.run(S, profiles, t, cmd, None, sc, st, tid, tsc, tp=tp, p=P)[0]


def _oracle(P, S, tp, profiles, t, cmd, sc=None, st=None, tid=None, tsc=None):
    return gto.targets(P, [gait.stride(s) for s in S], tp, profiles, t, cmd, None, sc, st, tid, tsc)[0]


ENGINES = [("twin", _twin), ("oracle", _oracle)]
PLAIN = {"twin": lambda P, S, t, cmd, sc, st: hg.run(S, t, cmd, None, sc, st, p=P)[0],
         "oracle": lambda P, S, t, cmd, sc, st: go.targets(P, [gait.stride(s) for s in S], t, cmd, None, sc, st)[0]}
FOOT_ROWS = list(range(18, 54))


@pytest.mark.parametrize("engine", ENGINES, ids=lambda e: e[0])
def test_flat_terrain_at_zero_and_scale_zero_give_the_plain_gait(engine):
    """Foot rows bit for bit, body z within one rounding of the height, attitude (0, 0, psi) exactly, the other body rows bit for bit:
    on level ground at height 0, on any profile at terrain_scale 0, with either body mode."""
    P = hg.params()
    t, cmd, sc, st = tgc.sample_batch(1)
    n = t.size
    profiles, ids, _ = sixteen()
    for name in ("trot", "gallop", "walk"):
        plain = PLAIN[engine[0]](P, [name], t, cmd, sc, st)
        for body in ("fit", "lift"):
            tp = gto.tparams(body=body, max_grade=MAX_GRADE)
            for label, got in (("flat", engine[1](P, [name], tp, [tr.flat(0.0, yaw=0.7, x0=0.1)], t, cmd, sc, st)),
                               ("scale 0", engine[1](P, [name], tp, profiles, t, cmd, sc, st, ids(n), np.zeros(n)))):
                assert pe.same_bits(got[FOOT_ROWS] + 0.0, plain[FOOT_ROWS] + 0.0), (name, body, label)      # (+ 0.0: -0.0 is 0.0)
                assert np.abs(got[2] - plain[2]).max() <= np.spacing(P["height"]) and (got[[5, 8]] == 0).all(), (name, body, label)
                assert (got[[9, 10, 12, 13, 15, 16]] == 0).all() and pe.same_bits(got[[0, 1, 3, 4, 6, 7, 11, 14, 17]], plain[[0, 1, 3, 4, 6, 7, 11, 14, 17]])


@pytest.mark.parametrize("engine", ENGINES, ids=lambda e: e[0])
def test_flat_terrain_at_a_height_raises_every_z_by_it_and_nothing_else(engine):
    """Stance feet and the body: exactly (c + c + c + c) / 4 = c; a swing foot's z is c + a b(u), one rounding of a number below 0.4."""
    P = hg.params()
    t, cmd, sc, st = tgc.sample_batch(2)
    c = 0.3125
    tp = gto.tparams(max_grade=MAX_GRADE)
    for name in ("trot", "limp"):
        base = engine[1](P, [name], tp, [tr.flat(0.0)], t, cmd, sc, st)
        got = engine[1](P, [name], tp, [tr.flat(c, yaw=-1.1, y0=0.2)], t, cmd, sc, st)
        other = [r for r in range(54) if r not in (2, 20, 29, 38, 47)]
        assert pe.same_bits(got[other], base[other]) and (got[2] == base[2] + c).all()
        assert np.abs(got[[20, 29, 38, 47]] - (base[[20, 29, 38, 47]] + c)).max() <= np.spacing(0.4)


@pytest.mark.parametrize("engine", ENGINES, ids=lambda e: e[0])
def test_a_plane_along_the_heading_pitches_the_trunk_by_its_grade(engine):
    """A plane of grade gamma rising along the heading, a straight command, trot: FIT gives pitch = -atan(gamma), roll 0 and no
    attitude rates.  The centred stance is symmetric, so the two feet of a diagonal pair have lever arms x and -x and the same footholds'
    timing: what a pair adds to sum xt g beyond gamma xt^2 cancels.  Bars: a foothold's s carries a dozen roundings of numbers of up to
    4 m (0.2 m/s for 20 s), 5e-15; g = gamma s, and P sums four of them with lever weights xt / sum xt^2 = 1.33 / m: gamma 5e-15 x 1.33
    x 4 = 8e-15 at gamma = 0.3, hence on the angle: 1e-14.  The rates multiply the same errors of z_B - z_A by sigma' / D <= 1.875 / D
    and sigma'' / D^2 <= 5.774 / D^2 at D = 0.15 s, the swing of a trot at scale 0.5: 12.5 and 257 times, 1e-13 and 2.1e-12; bars 2e-13
    and 4e-12."""
    P = hg.params()
    centred = P["stance"] - P["stance"].mean(0)
    assert np.allclose(np.abs(centred), np.abs(centred[0]))                             # the lever arms: symmetric about both axes
    t, _, sc, _ = tgc.sample_batch(0)
    n = t.size
    for gamma, psi0 in ((0.2, 0.0), (-0.15, 0.9), (0.3, -2.5)):
        prof = tr.Profile([-50.0, 50.0], [-50.0 * gamma, 50.0 * gamma], yaw=psi0, x0=0.3, y0=-0.2)
        st = np.tile([[0.3], [-0.2], [psi0]], (1, n))
        cmd = np.tile([[0.2], [0.0], [0.0]], (1, n))
        got = engine[1](P, ["trot"], gto.tparams(max_grade=0.5), [prof], t, cmd, sc, st)
        assert np.abs(got[10] + math.atan(gamma)).max() < 1e-14 and np.abs(got[9]).max() < 1e-14, (gamma, np.abs(got[10] + math.atan(gamma)).max())
        assert np.abs(got[[12, 13]]).max() < 2e-13 and np.abs(got[[15, 16]]).max() < 4e-12
        th = go.theta(P["ramp_time"], np.maximum(t, 0.0))[0] * (t >= 0)
        assert np.abs(got[2] - (P["height"] + gamma * 0.2 * th)).max() < 0.07             # the body climbs with the plane (footholds lead or lag it by up to half a stride, 0.2 m)


@pytest.mark.parametrize("engine", ENGINES, ids=lambda e: e[0])
def test_turning_world_start_and_profile_about_z_turns_the_answer(engine):
    """Bars: test_gait_cpu's for the x-y rows (2e-13, 2.5e-13, 5.2e-12); heights and attitude carry the foothold's s, a dozen
    roundings of numbers of up to 30 m, times a slope of at most 3 (the ridge at scale 2.5): 10 x 3 x 2e-14 = 6e-13, and their rates
    1.875 / D and 5.774 / D^2 of that at D >= 0.15 s: 8e-12 and 1.6e-10.  The samples within 1e-9 of a decision are left out."""
    P = hg.params()
    t, cmd, sc, st = tgc.sample_batch(1)
    n = t.size
    a = 0.83
    ca, sa = math.cos(a), math.sin(a)
    st2 = np.stack([ca * st[0] - sa * st[1], sa * st[0] + ca * st[1], st[2] + a])
    profiles, ids, scales = sixteen()
    turned = [p.rotated(a) for p in profiles]
    tp = gto.tparams(max_grade=MAX_GRADE)
    info, info2 = {}, {}
    gto.targets(P, [gait.stride("trot")], tp, profiles, t, cmd, None, sc, st, ids(n), scales(n), dtype=np.longdouble, info=info)
    gto.targets(P, [gait.stride("trot")], tp, turned, t, cmd, None, sc, st2, ids(n), scales(n), dtype=np.longdouble, info=info2)
    keep = np.asarray((info["near"] >= NEAR) & (info2["near"] >= NEAR))
    assert keep.mean() > 0.99
    base = engine[1](P, ["trot"], tp, profiles, t, cmd, sc, st, ids(n), scales(n))
    got = engine[1](P, ["trot"], tp, turned, t, cmd, sc, st2, ids(n), scales(n))
    want = tgc._rotz_rows(a, base)
    want[11] = base[11] + a
    for (_, rows), bar in zip(GROUPS, (6e-13, 8e-12, 1.6e-10, 6e-13, 1.6e-10)):
        worst = float(np.abs(got[rows][:, keep] - want[rows][:, keep]).max())
        assert worst < bar, (rows, worst, bar)
    assert float(np.abs(got - base).max()) > 0.1


# ---- clearance
def _random_profile(rng, yaw, x0):
    gaps = rng.uniform(0.02, 0.25, 7)
    s = -0.4 + np.r_[0.0, np.cumsum(gaps)]
    return tr.Profile(s, rng.uniform(-0.08, 0.12, 8), yaw=yaw, x0=x0, y0=rng.uniform(-0.1, 0.1))


def _b(u):
    return 64.0 * u**3 * (1.0 - u)**3


@pytest.mark.parametrize("edge_margin", [0.0, 0.03])
def test_every_swing_clears_the_terrain_by_the_flat_swing_profile(edge_margin):
    """Sixteen random 8-knot profiles (heights in [-0.08, 0.12], knots at least 0.02 m apart), apex_max out of reach, trot and walk,
    dense samples: z - H(x, y) >= swing_height b(u) - 1e-12 under every swing foot, in the oracle and in the twin (1e-12 m: four
    orders above the rounding of heights of this size).  And no foothold of a run with a > 0 lies inside a forbidden interval where
    the treads around the steep pieces are longer than 2 edge_margin."""
    rng = np.random.default_rng(77)
    profiles = [_random_profile(rng, rng.uniform(-3, 3), rng.uniform(-0.2, 0.6)) for _ in range(16)]
    P = hg.params()
    tp = gto.tparams(max_grade=0.5, edge_margin=edge_margin, apex_max=10.0)
    t = np.arange(6000) * 1.1e-3 + 1.234e-4
    n = t.size
    tid = (np.arange(n) % 16).astype(np.uint8)
    cmd = np.array([(0.4, 0.0, 0.0), (0.3, 0.1, 0.3), (-0.3, 0.0, -0.4)])[(np.arange(n) // 16) % 3].T.copy()
    sc = np.full(n, 0.5)
    swings = steep_checked = 0
    for name in ("trot", "walk"):
        info = {}
        for label, f in (("oracle", lambda: gto.targets(P, [gait.stride(name)], tp, profiles, t, cmd, None, sc, None, tid, info=info)),
                         ("twin", lambda: hgt.run([name], profiles, t, cmd, None, sc, None, tid, tp=tp, p=P))):
            got, mask = f()
            d = go.clock(gait.stride(name)[0], t, sc)
            for foot in range(4):
                r = 18 + 9 * foot
                H = np.array([float(gto.height(profiles[tid[i]], 1.0, gto.coordinate(profiles[tid[i]], got[r, i], got[r + 1, i]))) for i in range(n)])
                swing = ((mask >> foot) & 1) == 0
                # u of the swing, from the oracle's restatement of the runs
                u = np.zeros(n)
                B = go.boundaries(gait.stride(name)[0])
                for j in range(len(B) - 1):
                    contact, lo, hi, _, _ = go.runs(gait.stride(name)[1], foot, j)
                    if not contact:
                        inj = swing & (d[3] == j)
                        a, b = d[1] + sc * go.boundary(B, lo), d[1] + sc * go.boundary(B, hi)
                        u = np.where(inj, (t - a) / (b - a), u)
                gap = got[r + 2] - H - P["swing_height"] * _b(u)
                assert float(gap[swing].min()) >= -1e-12, (label, name, foot, float(gap[swing].min()))
                assert np.abs((got[r + 2] - H)[~swing]).max() < 1e-12                                  # stance feet: on the surface
                swings += int(swing.sum())
                if edge_margin > 0:
                    for i in np.nonzero(~swing & ~info["fixed"][foot])[0]:
                        p = profiles[tid[i]]
                        s = float(gto.coordinate(p, got[r, i], got[r + 1, i]))
                        steep = [abs((p.h[j + 1] - p.h[j]) / (p.s[j + 1] - p.s[j])) > 0.5 for j in range(7)]
                        for j in range(7):
                            # the pass is one pass: the guarantee holds where the neighbours of a steep piece are long level treads
                            long_treads = all(k < 0 or k > 6 or steep[k] or p.s[k + 1] - p.s[k] > 2 * edge_margin for k in (j - 1, j + 1)) and \
                                not any(steep[k] for k in (j - 1, j + 1) if 0 <= k <= 6)
                            if steep[j] and long_treads:
                                steep_checked += 1
                                assert not (p.s[j] - edge_margin + 1e-12 < s < p.s[j + 1] + edge_margin - 1e-12), (label, name, foot, i, j, s)
        assert float(np.nanmax(info["apex"])) > 0.08                                                   # swings were raised
    assert swings > 10000 and (edge_margin == 0 or steep_checked > 1000)


# ---- continuity
def test_feet_body_height_and_attitude_are_continuous_across_every_lift_off_and_touch_down():
    """Foot rows, body z and roll / pitch eps = 1e-9 s before and after every boundary of every foot's runs, on the kerb, the stairs
    and the eight-knot profile at scale 2.5.  With u = eps / D, D >= 0.05 s (limp at scale 0.5), steps L <= 1.2 m, rises dz <= 0.5 m and
    apex <= apex_max = 0.25 m the swing side leaves the foothold by |dp| <= (10 (L + dz) + 64 a) u^3 < 1e-12, |dv| <= (30 (L + dz) +
    192 a) u^2 / D < 1e-12, |da| <= (60 (L + dz) + 384 a) u / D^2 < 1.6e-3.  The body rows are means and fits of the four g_f, lever
    weights below 1.5 / m: they move by their own rates over 2 eps -- |g'| <= 1.875 dz / D < 19 m/s, |g''| <= 5.774 dz / D^2 < 1200
    m/s^2, |g'''| <= 60 dz / D^3 < 2.4e5 m/s^3 -- which gives 4e-8, 2.4e-6 and 5e-4 (+ the foot's own 1.6e-3 / 4) for z and 1.5 x 4
    times that for the angles."""
    P = hg.params()
    eps = 1e-9
    profiles = [tr.ramp_step(0.3, 0.10), tr.stairs(0.3, 0.2, [0.08] * 3), fo.sixteen_profiles()[6]]
    tsc = [1.0, 1.0, 2.5]
    tp = gto.tparams(max_grade=MAX_GRADE)
    for engine in ENGINES:
        for name in ("trot", "walk", "gallop", "limp"):
            for scale in (0.5, 1.0):
                edges = [(f, x) for f, _, a, b in tgc._run_times(name, scale) for x in (a, b)]
                tb = np.array([x[1] for x in edges])
                n = tb.size
                cmd = np.tile([[0.5], [0.1], [0.4]], (1, n))
                tid = (np.arange(n) % 3).astype(np.uint8)
                sc = np.full(n, scale)
                ts = np.array(tsc)[tid]
                lo = engine[1](P, [name], tp, profiles, tb - eps, cmd, sc, None, tid, ts)
                hi = engine[1](P, [name], tp, profiles, tb + eps, cmd, sc, None, tid, ts)
                for i, (f, _) in enumerate(edges):
                    r = 18 + 9 * f
                    d = np.abs(hi[r:r + 9, i] - lo[r:r + 9, i])
                    assert d[0:3].max() < 1e-12 + 1e-14 and d[3:6].max() < 1e-12 and d[6:9].max() < 1.6e-3, (engine[0], name, scale, f, d)
                dz = np.abs(hi - lo)
                assert dz[2].max() < 4e-8 and dz[5].max() < 2.4e-6 and dz[8].max() < 9e-4, (engine[0], name, dz[[2, 5, 8]].max(1))
                assert dz[9:11].max() < 2.4e-7 and dz[12:14].max() < 1.5e-5 and dz[15:17].max() < 5.4e-3, (engine[0], name)
                assert np.abs(hi[9:11]).max() > 0.01


def test_central_differences_reproduce_the_rates():
    """pd and pdd of every row against central differences of p and pd, trot at scale 1 (swing D = 0.3 s) over the kerb of 0.10 m on
    an arc, FIT.  Truncation h^2 / 6 times the next derivative: with L <= 0.6 m, dz <= 0.2 m, apex <= 0.25 m, |p'''| <= (60 (L + dz) +
    3840 a) / D^3 < 3.8e4 and |p''''| <= 360 (L + dz + 64 a / 3) / D^4 < 2.8e5; the attitude rows carry lever weights of 1.5 / m on
    each of four feet, times 6.  Oracle in extended precision, h = 1e-6: 7e-9 and 5e-8 (x 6).  Twin in double, h = 1e-5 (rounding 2 eps
    |f| / h: 1e-10, 1e-9): 7e-7 and 5e-6 (x 6)."""
    P = hg.params()
    t = np.arange(200, 2400) * tgc.DT_SAMPLE / 4 + tgc.OFFSET
    n = t.size
    cmd = np.tile([[0.5], [0.1], [0.4]], (1, n))
    prof = [tr.ramp_step(0.3, 0.10)]
    tp = gto.tparams()
    S = [gait.stride("trot")]
    wide = lambda x: gto.targets(P, S, tp, prof, x, cmd, dtype=np.longdouble)[0]
    twin = lambda x: hgt.run(["trot"], prof, x, cmd, tp=tp, p=P)[0]
    lin = [r for r in XYZ]
    for label, f, h, bars in (("oracle", wide, 1e-6, (7e-9, 5e-8)), ("twin", twin, 1e-5, (7e-7, 5e-6))):
        lo, hi = t - h, t + h
        span = (hi.astype(np.longdouble) - lo.astype(np.longdouble)) if label == "oracle" else hi - lo
        mid, a, b = f(t), f(lo), f(hi)
        for order in (0, 1):
            for kind, rows, k in (("xyz", lin, 1.0), ("attitude", [9, 10, 11], 6.0)):
                src, dst = [r + 3 * order for r in rows], [r + 3 * order + 3 for r in rows]
                worst = float(np.abs((b[src] - a[src]) / span - mid[dst]).max())
                print("GAIT-TERRAIN central difference %s %s %s: worst %.3g bar %.3g" % (label, kind, ("pd", "pdd")[order], worst, k * bars[order]))
                assert worst < k * bars[order]
    assert np.abs(mid[[5, 13]]).max() > 0.05                                           # the body's z and pitch moved


# ---- malformed instances
MALFORMED = tgc.MALFORMED + [("terrain_id", None), ("terrain_scale", math.nan), ("terrain_scale", math.inf), ("terrain_scale", -math.inf)]


def spoil(case, value, i, count, tcount, time, cmd, gid, sc, st, tid, tsc):
    if case == "terrain_id":
        tid[i] = tcount
    elif case == "terrain_scale":
        tsc[i] = value
    else:
        tgc.spoil(case, value, i, count, time, cmd, gid, sc, st)


def malformed_batch(n, count, tcount, seed=5):
    rng = np.random.default_rng(seed + 100)
    return tgc.malformed_batch(n, count, seed) + ((np.arange(n) % tcount).astype(np.uint8), rng.uniform(-1.0, 2.0, n))


def test_malformed_instances_get_nan_rows_and_a_full_mask_and_their_neighbours_nothing():
    names = ["trot", "walk", "pace"]
    profiles = fo.sixteen_profiles()[:5]
    n = 3 * len(MALFORMED) + 2
    clean = malformed_batch(n, len(names), len(profiles))
    dirty = [a.copy() for a in clean]
    bad = np.zeros(n, bool)
    for k, (case, value) in enumerate(MALFORMED):
        spoil(case, value, 3 * k + 1, len(names), len(profiles), *dirty)
        bad[3 * k + 1] = True
    P = hg.params()
    S = [gait.stride(s) for s in names]
    tp = gto.tparams(max_grade=MAX_GRADE)
    twin = None
    for label, f in (("twin", lambda a: hgt.run(names, profiles, *a, tp=tp, p=P)),
                     ("oracle", lambda a: gto.targets(P, S, tp, profiles, *a))):
        ct, cm = f(clean)
        dt_, dm = f(dirty)
        twin = ct if label == "twin" else twin
        assert np.isfinite(ct).all(), label
        assert np.isnan(dt_[:, bad]).all() and (dm[bad] == 0xF).all(), label
        assert pe.same_bits(dt_[:, ~bad], ct[:, ~bad]) and (dm[~bad] == cm[~bad]).all(), label
    wide = (np.full((54, n), 7.5), np.full(n, 0x55, np.uint8))
    hgt.run(names, profiles, *clean, tp=tp, p=P, n=n - 5, out=wide)
    assert (wide[0][:, n - 5:] == 7.5).all() and (wide[1][n - 5:] == 0x55).all() and pe.same_bits(wide[0][:, :n - 5], twin[:, :n - 5])


# ---- what returns before any device is touched
def test_abi_gait_terrain_misuse_without_device():
    from quadruped_drake_amd import _lib
    L = _lib.lib()
    err = lambda: L.wbc_last_error().decode()
    P = hg.params()
    cp = gait.c_params(P["stance"], P["height"], P["swing_height"], P["ramp_time"], P["wait_time"])
    h = C.c_void_p()
    assert L.wbc_gait_create(C.byref(cp), gait.c_strides(["trot"]), 1, 0, C.byref(h)) == 0 and h.value       # host work only
    prof = tr.c_array([tr.ramp_step(0.3, 0.1)])
    pp = C.cast(prof, C.c_void_p)
    ok = gait.c_terrain_params()
    calls = ((lambda tp, p, count: L.wbc_gait_terrain_check(tp, p, count), "wbc_gait_terrain_check"),
             (lambda tp, p, count: L.wbc_gait_set_terrain(h, tp, p, count, None, None), "wbc_gait_set_terrain"))
    assert L.wbc_gait_terrain_check(C.byref(ok), pp, 1) == 0
    assert L.wbc_gait_terrain_check(None, pp, 1) < 0 and "null params" in err()
    assert L.wbc_gait_terrain_check(C.byref(ok), None, 1) < 0 and "null profiles" in err()
    for fn, name in calls:
        for field, value, word in (("body_mode", 2, "body_mode"), ("body_mode", -1, "body_mode"), ("max_grade", 0.0, "max_grade"),
                                   ("max_grade", math.nan, "max_grade"), ("max_grade", math.inf, "max_grade"), ("edge_margin", -0.01, "edge_margin"),
                                   ("edge_margin", math.nan, "edge_margin"), ("edge_margin", math.inf, "edge_margin"), ("apex_max", math.nan, "apex_max"),
                                   ("apex_max", math.inf, "apex_max")):
            q = gait.c_terrain_params()
            setattr(q, field, value)
            assert fn(C.byref(q), pp, 1) < 0 and word in err() and name in err(), (name, field, value, err())
        for count in (17, -1):
            assert fn(C.byref(ok), C.cast(tr.c_array([tr.flat()] * 17), C.c_void_p), count) < 0 and "count" in err()
        bent = tr.c_array([tr.ramp_step(0.3, 0.1)])
        bent[0].s[1] = bent[0].s[0]
        assert fn(C.byref(ok), C.cast(bent, C.c_void_p), 1) < 0 and "strictly increasing" in err()
    assert L.wbc_gait_set_terrain(None, C.byref(ok), pp, 1, None, None) < 0 and "null gait handle" in err()
    assert L.wbc_gait_set_terrain(h, None, pp, 1, None, None) < 0 and "null params" in err()
    low = gait.c_terrain_params(apex_max=0.04)                                          # below the gait's swing_height of 0.05
    assert L.wbc_gait_terrain_check(C.byref(low), pp, 1) == 0
    assert L.wbc_gait_set_terrain(h, C.byref(low), pp, 1, None, None) < 0 and "swing_height" in err()
    # FIT needs lever arms: a stance on one line has none
    line = C.c_void_p()
    cq = gait.c_params(np.array([[0.2, 0.1], [0.2, -0.1], [0.2, 0.05], [0.2, -0.05]]), P["height"], P["swing_height"], P["ramp_time"], P["wait_time"])
    assert L.wbc_gait_create(C.byref(cq), gait.c_strides(["trot"]), 1, 0, C.byref(line)) == 0
    assert L.wbc_gait_set_terrain(line, C.byref(ok), pp, 1, None, None) < 0 and "FIT" in err()
    # taking the terrain away is host work, and the handle is then as it was: still without commands
    for g in (h, line):
        assert L.wbc_gait_set_terrain(g, None, None, 0, None, None) == 0 and L.wbc_gait_set_terrain(g, C.byref(ok), None, 1, None, None) == 0
        assert L.wbc_gait_set_terrain(g, C.byref(ok), pp, 0, None, None) == 0
    buf, tm, mk = np.zeros((54, 4)), np.zeros(4), np.zeros(4, np.uint8)
    p = lambda a: C.c_void_p(a.ctypes.data)
    assert L.wbc_gait_targets(h, None, 4, 4, p(tm), p(buf), p(mk)) < 0 and "wbc_gait_set_commands" in err()
    assert L.wbc_gait_terrain_kernel_info(None, None, None, None, None) < 0 and "null gait handle" in err()
    assert L.wbc_gait_destroy(h) == 0 and L.wbc_gait_destroy(line) == 0
    # the twin refuses the same
    t1, c1 = np.zeros(1), np.zeros((3, 1))
    assert hgt.run(["trot"], [tr.flat()], t1, c1, tp=dict(max_grade=0.0), rc=True) == -2
    assert hgt.run(["trot"], [tr.flat()], t1, c1, tp=dict(apex_max=0.01), rc=True) == -4
    assert hgt.run(["trot"], [tr.flat()], t1, c1, stance=[[0.2, 0.1, 0], [0.2, -0.1, 0], [0.2, 0.05, 0], [0.2, -0.05, 0]], rc=True) == -4
    with pytest.raises(ValueError):
        gait.c_terrain_params(body="tilt")


def test_simulate_gait_terrain_arguments():
    from quadruped_drake_amd import simulate
    base = ["--planner", "gait", "--plant", "ground", "--terrain", "ramp_step:0.1"]
    a = simulate.parse(base + ["--gait-terrain", "fit"])
    assert (a.gait_terrain, a.follow, a.terrain) == ("fit", "off", "ramp_step:0.1")
    assert simulate.parse(base).gait_terrain == "off" and simulate.parse(base + ["--gait-terrain", "lift"]).gait_terrain == "lift"
    for argv in (base + ["--gait-terrain", "fit", "--follow", "fit"], base + ["--gait-terrain", "tilt"],
                 ["--planner", "gait", "--plant", "ground", "--gait-terrain", "fit"],
                 ["--planner", "basic", "--plant", "ground", "--terrain", "ramp_step:0.1", "--gait-terrain", "lift"]):
        with pytest.raises(SystemExit):
            simulate.parse(argv)


def test_closed_loop_refuses_a_terrain_gait_on_a_plant_that_follows():
    """Before any pointer is taken: the planner's targets are finished, the plant's follow pass would lift them a second time."""
    import types
    import torch
    from quadruped_drake_amd import plant
    n = 3
    p = object.__new__(plant.GroundContactPlant)
    p._L, p._h, p.device, p._terrain, p._follow = None, None, 0, ([tr.flat()], None, None, None), "fit"
    g = object.__new__(gait.GaitPlanner)
    g._h, g._n, g.device, g._terrain = None, n, 0, ([tr.flat()], None, None, None, "fit")
    ctrl = types.SimpleNamespace(host_ptrs=False, _h=C.c_void_p(16))
    q, v, tm = torch.zeros((19, n), dtype=torch.float64), torch.zeros((18, n), dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    assert g.has_terrain
    with pytest.raises(ValueError, match="follow"):
        plant.closed_loop(ctrl, p, g, 4, 5e-3, q, v, tm)
    g._terrain = ([tr.flat()], None, None, n + 1, "fit")
    p._follow = "off"
    with pytest.raises(ValueError, match="terrain_id"):
        plant.closed_loop(ctrl, p, g, 4, 5e-3, q, v, tm)


# ---- the closed loop on the host twins
SLIP, FELL, BAD = 1, 2, 8


def host_walk(prof, cmd, body="fit", kind="id", ticks=800, dt=5e-3, scale=0.5, model="mini_cheetah", plain_follow=None):
    """test_gait_cpu.host_walk's loop on a terrain, from workloads.nominal_state at the origin: terrain gait (host_gait_terrain) -> tick
    (host_tick) -> ground step (host_terrain).  plain_follow "lift" / "fit": the path without this law instead -- plain gait
    (host_gait) -> follow (host_follow) -> tick -> ground step.  -> dict(status, flags, first_bad, first_fell, x, y, z, dx, dy, dz: the
    trunk's final distance from the planned body position of the terrain gait)"""
    import host_follow as hf
    import host_terrain as ht
    import host_tick as hk
    from quadruped_drake_amd import workloads
    from quadruped_drake_amd.controller import load_model
    t = load_model(model)
    q, v = workloads.nominal_state(model, 1)
    P = hg.params(model)
    tp = gto.tparams(body=body)
    c = np.array(cmd, dtype=np.float64)[:, None]
    sc = np.array([scale])
    out = dict(status=0, flags=0, first_bad=None, first_fell=None)
    for k in range(ticks):
        if plain_follow is None:
            tg, mask = hgt.run(["trot"], [prof], np.array([k * dt]), c, None, sc, None, tp=tp, p=P)
        else:
            tg, mask = hg.run(["trot"], np.array([k * dt]), c, None, sc, None, p=P)
            tg = hf.run([prof], tg, plain_follow)
        tau, _, status, _ = hk.run(kind, t["flat"], q, v, tg, mask, act_perm=t.get("act_perm"))
        o = ht.run(t["flat"], q, v, tau, act_perm=t.get("act_perm"), dt=dt, profiles=[prof])
        q, v = o["q"], o["v"]
        out["status"] += int(status[0] != 0)
        out["flags"] |= int(o["flags"][0])
        for key, flag in (("first_bad", BAD), ("first_fell", FELL)):
            if out[key] is None and o["flags"][0] & flag:
                out[key] = k
        if o["flags"][0] & BAD:
            break
    plan = gto.targets(P, [gait.stride("trot")], tp, [prof], np.array([ticks * dt]), c, None, sc)[0][:, 0]
    out.update(x=float(q[4, 0]), y=float(q[5, 0]), z=float(q[6, 0]), dx=float(q[4, 0] - plan[0]), dy=float(q[5, 0] - plan[1]),
               dz=float(q[6, 0] - plan[2]))
    out["off"] = math.hypot(out["dx"], out["dy"])
    return out


WALKS = {"kerb_0.10": (lambda: tr.ramp_step(0.3, 0.10), (0.2, 0.0, 0.0)), "stairs_0.08": (lambda: tr.stairs(0.3, 0.2, [0.08] * 3), (0.2, 0.0, 0.0)),
         "yawed_kerb_arc": (lambda: tr.ramp_step(0.35, 0.10, yaw=0.6), (0.3, 0.0, 0.4))}
Z_BAR = 1.6e-3


@pytest.mark.parametrize("case", list(WALKS))
def test_id_walks_over_kerbs_and_stairs_on_the_host_twins(case):
    """Mini Cheetah, ID, dt 5 ms, trot at stride scale 0.5, command 0.2 m/s (the arc: 0.3 m/s and 0.4 rad/s), 800 ticks, FIT: no FELL,
    no BAD, status 0 on every tick, the trunk within 0.03 m of the planned (x, y) -- test_gait_cpu's bar, about ten times the measured
    figures -- and within 1.6 mm of the planned body z.  Measured (x, y and z off the plan): the kerb of 0.10 m 1.3 mm, 2.7 mm,
    -0.13 mm (x 0.7513, plan 0.75); the stairs of 0.08 m 0.13 mm, 0.30 mm, -0.04 mm; the yawed kerb on the arc -1.6 mm, 1.1 mm,
    -0.15 mm, ending at (0.7466, 0.6981).  The largest z distance measured is 0.154 mm, so 5 mm would be thirty times it: the bar is
    ten times the measured value, 1.6 mm."""
    make, cmd = WALKS[case]
    r = host_walk(make(), cmd)
    print("GAIT-TERRAIN host walk %s: x %.4f y %.4f z %.4f dx %+.5f dy %+.5f dz %+.6f flags %d status %d" %
          (case, r["x"], r["y"], r["z"], r["dx"], r["dy"], r["dz"], r["flags"], r["status"]))
    assert not r["flags"] & (FELL | BAD) and r["status"] == 0
    assert r["off"] < 0.03 and abs(r["dz"]) < Z_BAR


def test_id_does_not_walk_over_the_kerb_with_the_plain_gait_and_followed_targets():
    """The same kerb of 0.10 m through the path without this law -- plain gait, then the follow law with FIT: BAD before tick 800
    (measured: tick 241)."""
    r = host_walk(tr.ramp_step(0.3, 0.10), (0.2, 0.0, 0.0), plain_follow="fit")
    print("GAIT-TERRAIN host walk, kerb 0.10, plain gait + follow fit:", r)
    assert r["first_bad"] is not None and r["first_bad"] < 800


def test_what_the_law_does_not_reach_is_printed_not_asserted():
    """Recorded limits (the controllers are frozen): ID walking backwards over a kerb behind it, and MPTC at dt 1 ms over a kerb."""
    for label, prof, cmd, kw in (("ID backwards, kerb 0.05 behind", tr.Profile([-0.33, -0.30], [0.05, 0.0]), (-0.2, 0.0, 0.0), {}),
                                 ("ID backwards, kerb 0.10 behind", tr.Profile([-0.33, -0.30], [0.10, 0.0]), (-0.2, 0.0, 0.0), {}),
                                 ("MPTC dt 1 ms, plane", tr.flat(0.0), (0.2, 0.0, 0.0), dict(kind="mptc", dt=1e-3, ticks=2000)),
                                 ("MPTC dt 1 ms, kerb 0.05", tr.ramp_step(0.3, 0.05), (0.2, 0.0, 0.0), dict(kind="mptc", dt=1e-3, ticks=2000))):
        r = host_walk(prof, cmd, **kw)
        print("GAIT-TERRAIN limit %-32s first_bad %s first_fell %s x %.4f y %.4f dz %+.4f status %d" %
              (label, r["first_bad"], r["first_fell"], r["x"], r["y"], r["dz"], r["status"]))
