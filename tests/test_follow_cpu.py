"""Targets that follow the terrain (include/wbc_ground.h, "Following the ground"), no GPU: the host instantiation of
csrc/wbc_ground_follow.hpp (tests/host_follow.py) against the numpy restatement of the header's sentences (tests/follow_oracle.py),
exact relations that need no oracle, unusable feet, bad terrain choices, the argument checks that return before any device is
touched, and the closed loop on the host twins: ID standing on a slope of grade 0.2 with followed targets, and failing with level
ones.

The bar of every comparison with the oracle is 1e-12 (1 + |value|) per entry: the law is a few dozen roundings, amplified by at most
1 / cos(1.2) = 2.8 in the rates.  The measured worst is printed ("FOLLOW ..." lines) and recorded in profiles/r12/follow.md."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import follow_oracle as fo
import host_follow as hf
import plant_edges as pe
import terrain_oracle as to
from quadruped_drake_amd import terrain as tr, workloads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-12
EXACT = 1e-14          # closed forms on a plane: a dozen roundings of numbers of order one
MODES = [("lift", fo.LIFT), ("fit", fo.FIT)]
FOOT_XY = [18 + 9 * c + k for c in range(4) for k in (0, 1)]


def worst(got, want):
    """max over the entries of |got - want| / (1 + |want|)"""
    return float((np.abs(got - want) / (1.0 + np.abs(want))).max())


def _rows_changed(a, b):
    return sorted(int(r) for r in np.nonzero((pe.bits(a) != pe.bits(b)).any(1))[0])


@pytest.mark.parametrize("table", ["four", "sixteen"])
def test_host_twin_matches_the_oracle_on_every_piece_of_every_profile(table):
    profiles = to.four_profiles() if table == "four" else None
    n = 9 * (4 if table == "four" else 16) + 7
    profiles, tid, tsc, t = fo.draw(n, 11, profiles)
    hits = {}
    for i in range(n):
        for c in range(4):
            key = (int(tid[i]), fo.piece_of(profiles[tid[i]], t[18 + 9 * c, i], t[19 + 9 * c, i]))
            hits[key] = hits.get(key, 0) + 1
    need = [(k, j) for k, p in enumerate(profiles) for j, lo, hi in fo.pieces(p) if lo < fo.REACH and hi > -fo.REACH]
    assert all(key in hits for key in need), sorted(set(need) - set(hits))
    assert any(j == -1 for _, j in hits) and any(j == len(profiles[k].s) - 1 for k, j in hits)     # level ground before and after
    if table == "sixteen":                                      # instance 4: every foothold exactly on a knot, in the piece it opens
        assert [fo.piece_of(profiles[4], t[18 + 9 * c, 4], 0.0) for c in range(4)] == [0, 1, 2, 3]
        assert [t[18 + 9 * c, 4] for c in range(4)] == profiles[4].s
    for s in fo.SCALES:
        assert (tsc == s).any(), s
    assert (tsc < 0).any() and (tsc == 0).any() and (tsc == 2.5).any()
    for name, mode in MODES:
        got = hf.run(profiles, t, name, tid, tsc)
        want = fo.follow(profiles, tid, tsc, t, mode)
        assert np.abs(want[10]).max() <= 1.2
        w = worst(got, want)
        print("FOLLOW twin-to-oracle", table, name, "worst %.3g" % w, "max |pitch'| %.3f" % np.abs(want[10]).max())
        assert w < BAR
        assert np.abs(want - t).max() > 1e-2                   # and the law did something
        assert _rows_changed(got, t) == sorted(fo.ZROWS + (fo.ATTITUDE if mode == fo.FIT else []))


# ---- exact relations that need no oracle
def test_zero_scale_and_level_ground_at_zero_return_the_targets_bit_for_bit():
    profiles, tid, tsc, t = fo.draw(64, 12)
    for name, _ in MODES:
        assert pe.same_bits(hf.run(profiles, t, name, tid, np.zeros(64)), t), name
        assert pe.same_bits(hf.run([tr.flat(0.0, yaw=0.7, x0=0.1)], t, name), t), name
        assert pe.same_bits(hf.run(profiles, t, "off", tid, tsc), t)
        assert pe.same_bits(hf.run(None, t, name), t), name
        assert not pe.same_bits(hf.run(profiles, t, name, tid, tsc), t), name


@pytest.mark.parametrize("h0", [0.37, -0.1, 1.0 / 3.0])
def test_raised_level_ground_shifts_exactly_the_five_heights(h0):
    _, _, _, t = fo.draw(64, 13)
    want = t.copy()
    want[[2] + [18 + 9 * c + 2 for c in range(4)]] += h0
    for name, _ in MODES:
        assert pe.same_bits(hf.run([tr.flat(h0, yaw=-1.1, y0=0.2)], t, name), want), name


@pytest.mark.parametrize("grade", [0.2, -0.35, 1.0])
def test_level_standing_targets_on_a_plane_pitch_with_it(grade):
    """psi = 0: rpy' = (0, -atan grade, 0) and the body's height is the plane's under it; at any psi the body's z axis is the
    plane's normal."""
    st = workloads.standing_targets("mini_cheetah", 1)
    for yaw in (0.0, 0.9, -2.5):
        prof = tr.slope(math.atan(grade), start=-5.0, length=10.0, yaw=yaw, x0=0.03, y0=-0.02)
        got = hf.run([prof], st, "fit")[:, 0]
        H, nrm = tr.evaluate(prof, st[0, 0], st[1, 0])
        assert abs(got[2] - (st[2, 0] + float(H))) < EXACT
        zaxis = fo.rpy_matrix(got[9:12])[:, 2]
        assert np.abs(zaxis - nrm).max() < EXACT
        if yaw == 0.0:
            assert np.abs(got[9:12] - [0.0, -math.atan(grade), 0.0]).max() < EXACT
        assert (got[12:18] == 0).all()
        for c in range(4):                                 # the feet on the plane, x and y as given
            Hc = float(tr.evaluate(prof, st[18 + 9 * c, 0], st[19 + 9 * c, 0])[0])
            assert abs(got[18 + 9 * c + 2] - (st[18 + 9 * c + 2, 0] + Hc)) < EXACT
        assert pe.same_bits(got[FOOT_XY], st[FOOT_XY, 0]) and pe.same_bits(got[0:2], st[0:2, 0])


def _rotz_rows(a, t, rows):
    c, s = math.cos(a), math.sin(a)
    out = t.copy()
    for r in rows:
        out[r], out[r + 1] = c * t[r] - s * t[r + 1], s * t[r] + c * t[r + 1]
    return out


def test_rotating_the_profile_and_the_targets_about_z_rotates_the_answer():
    a = 0.83
    profiles, tid, tsc, t = fo.draw(96, 14)
    t[18:54:9, 4] += 0.01                                   # off the knots: which side of one a foot is on must not hang on a rounding
    vec_rows = [0, 3, 6] + [18 + 9 * c + 3 * d for c in range(4) for d in range(3)]       # every (x, y) pair of rows
    t2 = _rotz_rows(a, t, vec_rows)
    t2[11] = t[11] + a
    rot = [p.rotated(a) for p in profiles]
    for name, mode in MODES:
        base = hf.run(profiles, t, name, tid, tsc)
        got = hf.run(rot, t2, name, tid, tsc)
        want = _rotz_rows(a, base, vec_rows)
        turn = got[11] - (base[11] + a)                     # yaw' + a, up to the whole turns atan2 takes off
        want[11] = got[11] - ((turn + math.pi) % (2.0 * math.pi) - math.pi)
        w = worst(got, want)
        print("FOLLOW rotated world", name, "worst %.3g" % w)
        assert w < BAR
        assert worst(got, base) > 1e-3                      # and it is no identity


def test_lift_and_fit_agree_on_every_row_but_the_attitude():
    profiles, tid, tsc, t = fo.draw(96, 15)
    lift, fit = hf.run(profiles, t, "lift", tid, tsc), hf.run(profiles, t, "fit", tid, tsc)
    keep = [r for r in range(54) if r not in fo.ATTITUDE]
    assert pe.same_bits(lift[keep], fit[keep])
    assert pe.same_bits(lift[fo.ATTITUDE], t[fo.ATTITUDE]) and not pe.same_bits(fit[fo.ATTITUDE], t[fo.ATTITUDE])


# ---- feet whose targets hold anything
@pytest.mark.parametrize("dead", [(1,), (0, 3), (0, 1, 2), (0, 1, 2, 3)])
def test_feet_without_a_finite_target_take_no_part(dead):
    """A contact foot's rows may hold anything (include/wbc.h): with NaN (or x or y alone not finite) in the rows of the feet
    `dead`, those rows keep their bits, every other row is finite and is the oracle's answer over the remaining feet, the living
    feet get what they get with all four alive, and the body does not (three, two: another fit; one, none: no slope, the height
    of that foothold or of the ground under the body, the attitude as given)."""
    profiles, tid, tsc, t = fo.draw(80, 16)
    td = t.copy()
    for c in dead:
        td[18 + 9 * c:27 + 9 * c] = np.nan
    td[18 + 9 * dead[0] + 1, ::2] = 0.123                     # x alone not finite is enough
    td[18 + 9 * dead[0], 1::4] = np.inf
    live_rows = [r for r in range(54) if not any(18 + 9 * c <= r < 27 + 9 * c for c in dead)]
    dead_rows = [r for r in range(54) if r not in live_rows]
    for name, mode in MODES:
        got = hf.run(profiles, td, name, tid, tsc)
        assert pe.same_bits(got[dead_rows], td[dead_rows]), name
        assert np.isfinite(got[live_rows]).all(), name
        want = fo.follow(profiles, tid, tsc, td, mode)
        assert worst(got[live_rows], want[live_rows]) < BAR, name
        full = hf.run(profiles, t, name, tid, tsc)
        body = [2, 5, 8] + (fo.ATTITUDE if mode == fo.FIT else [])
        if len(dead) >= 3:                                  # one usable foot or none: no slope, the attitude stands
            assert pe.same_bits(got[fo.ATTITUDE], td[fo.ATTITUDE]), name
            one = [c for c in range(4) if c not in dead]
            Hm = [fo.surface(profiles[tid[i]], tsc[i], *(td[18 + 9 * one[0]:20 + 9 * one[0], i] if one else td[0:2, i]))[1] for i in range(80)]
            assert np.abs(got[2] - (td[2] + Hm)).max() < BAR and pe.same_bits(got[[5, 8]], td[[5, 8]])
        else:
            assert worst(got[body], full[body]) > 1e-4, name   # the fit over fewer feet is another fit
        others = [18 + 9 * c + k for c in range(4) if c not in dead for k in range(9)]
        assert pe.same_bits(got[others], full[others]), name   # a living foot does not see the dead ones


def test_bad_terrain_choice_leaves_the_instance_alone():
    n = 48
    profiles, tid, tsc, t = fo.draw(n, 17)
    tid2, tsc2 = tid.copy(), tsc.copy()
    tid2[3] = 16; tid2[17] = 255; tsc2[9] = np.nan; tsc2[30] = -np.inf; tsc2[47] = np.inf
    bad = np.zeros(n, bool); bad[[3, 17, 9, 30, 47]] = True
    for name, mode in MODES:
        clean = hf.run(profiles, t, name, tid, tsc)
        got = hf.run(profiles, t, name, tid2, tsc2)
        assert pe.same_bits(got[:, bad], t[:, bad]) and not pe.same_bits(clean[:, bad], t[:, bad])
        assert pe.same_bits(got[:, ~bad], clean[:, ~bad])
        assert pe.same_bits(fo.follow(profiles, tid2, tsc2, t, mode)[:, bad], t[:, bad])
    # padding columns n .. ld are not the batch's
    wide = pe.wide(t, n + 5, np.nan)
    got = hf.run(profiles, wide, "fit", np.r_[tid, [0] * 5], np.r_[tsc, [1.0] * 5], n=n)
    assert pe.padding_kept(got, n, np.nan) and pe.same_bits(got[:, :n], hf.run(profiles, t, "fit", tid, tsc))


# ---- what returns before any device is touched
def test_abi_follow_misuse_without_device():
    from quadruped_drake_amd import plant
    L = plant._L()
    err = lambda: L.wbc_last_error().decode()
    buf = np.zeros((54, 4))
    p = C.c_void_p(buf.ctypes.data)
    fake = C.c_void_p(8)                                   # never dereferenced: every case below is refused on its arguments alone
    assert L.wbc_ground_follow_targets(None, None, 4, 4, 2, p) < 0 and "null ground handle" in err()
    assert L.wbc_ground_follow_targets(None, None, 0, 0, 2, None) < 0 and "null ground handle" in err()
    assert L.wbc_ground_set_follow(None, 1) < 0 and "null ground handle" in err()
    assert L.wbc_ground_follow_kernel_info(None, None, None, None, None) < 0 and "null ground handle" in err()
    assert L.wbc_ground_follow_targets(fake, None, -1, 4, 2, p) < 0 and "n out of range" in err()
    assert L.wbc_ground_follow_targets(fake, None, 4, 3, 2, p) < 0 and "ld must be >= n" in err()
    assert L.wbc_ground_follow_targets(fake, None, 0, -1, 2, p) < 0 and "ld must be >= n" in err()
    assert L.wbc_ground_follow_targets(fake, None, 4, 4, 2, None) < 0 and "targets are required" in err()
    for mode in (-1, 3, 77):
        assert L.wbc_ground_follow_targets(fake, None, 4, 4, mode, p) < 0 and "mode" in err()
        assert L.wbc_ground_set_follow(fake, mode) < 0 and "mode" in err()
    assert (buf == 0).all()
    for bad in ("up", "FIT", ""):
        with pytest.raises(ValueError):
            plant._follow_mode(bad)
    assert [plant._follow_mode(m) for m in ("off", "lift", "fit", 2)] == [0, 1, 2, 2]
    hdr = open(os.path.join(ROOT, "include", "wbc_ground.h")).read()
    for name, value in (("OFF", 0), ("LIFT", 1), ("FIT", 2)):
        assert "#define WBC_FOLLOW_%s %d\n" % (name, value) in hdr and plant.FOLLOW_MODES[name.lower()] == value
    assert (fo.OFF, fo.LIFT, fo.FIT) == (0, 1, 2) and hf.MODES == plant.FOLLOW_MODES


def test_simulate_follow_arguments_and_pyramid_mu():
    from quadruped_drake_amd import simulate
    assert simulate.parse([]).follow == "off"
    assert simulate.parse(["--plant", "ground", "--terrain", "slope:0.2"]).follow == "off"
    for mode in ("off", "lift", "fit"):
        assert simulate.parse(["--plant", "ground", "--terrain", "slope:0.2", "--follow", mode]).follow == mode
    for argv in (["--follow", "fit"], ["--plant", "ground", "--follow", "lift"], ["--plant", "rigid", "--follow", "fit"],
                 ["--plant", "ground", "--terrain", "slope:0.2", "--follow", "tilt"]):
        with pytest.raises(SystemExit):
            simulate.parse(argv)
    assert tr.pyramid_mu(1.0, 0.0) == pytest.approx(1.0, abs=1e-15)
    for mu_p, grade in ((1.0, 0.2), (0.7, -0.2), (0.5, 0.3), (0.4, 0.4), (0.3, 1.0)):
        want = (mu_p - abs(grade)) / (1.0 + mu_p * abs(grade))          # tan of a difference
        assert tr.pyramid_mu(mu_p, grade) == pytest.approx(want, abs=1e-15)
        assert tr.pyramid_mu(mu_p, grade) == tr.pyramid_mu(mu_p, -grade)
    assert tr.pyramid_mu(0.4, 0.4) == pytest.approx(0.0, abs=1e-16) and tr.pyramid_mu(0.3, 1.0) < 0 < tr.pyramid_mu(0.7, 0.2)
    assert "<= 0" in tr.pyramid_mu.__doc__


# ---- the closed loop on the host twins
def host_stand(mode, ticks=100, dt=5e-3, grade=0.2, model="mini_cheetah"):
    """ID with standing targets on terrain_oracle.slope_stance(model, grade), every tick: follow (host_follow) -> tick (host_tick)
    -> ground step on the slope (host_terrain).  -> dict(status: ticks with a non-zero status, flags: OR of the plant's flags,
    first_bad: the first tick that raised BAD or None, height: final trunk height above the ground under it, pitch: final pitch)"""
    import host_terrain as ht
    import host_tick as hk
    t, q, v, prof = to.slope_stance(model, grade)
    st = workloads.standing_targets(model, 1)
    mask = np.array([0b1111], np.uint8)
    out = dict(status=0, flags=0, first_bad=None)
    for k in range(ticks):
        tg = hf.run([prof], st, mode)
        tau, _, status, _ = hk.run("id", t["flat"], q, v, tg, mask, act_perm=t.get("act_perm"))
        o = ht.run(t["flat"], q, v, tau, act_perm=t.get("act_perm"), dt=dt, profiles=[prof])
        q, v = o["q"], o["v"]
        out["status"] += int(status[0] != 0)
        out["flags"] |= int(o["flags"][0])
        if out["first_bad"] is None and o["flags"][0] & to.BAD:
            out["first_bad"] = k
    w, x, y, z = q[0:4, 0] / np.linalg.norm(q[0:4, 0])
    out["height"] = float(q[6, 0] - tr.evaluate(prof, q[4, 0], q[5, 0])[0])
    out["pitch"] = math.asin(2.0 * (w * y - z * x))
    return out


def test_id_stands_on_a_slope_with_followed_targets_and_not_with_level_ones():
    """Mini Cheetah, ID, dt 5 ms, slope of grade 0.2, standing targets, 100 ticks.  FIT: no plant flag, no non-zero status, the
    trunk 0.3 m above the ground under it and pitched by -atan 0.2, both within 1e-3 (measured: 4.5e-5 and 4.6e-5 off).  Level
    targets: BAD before tick 100 (measured: tick 49)."""
    r = host_stand("fit")
    print("FOLLOW host stand, fit: height %.6f pitch %.6f (target %.6f)" % (r["height"], r["pitch"], -math.atan(0.2)), r)
    assert r["flags"] == 0 and r["status"] == 0
    assert abs(r["height"] - 0.3) < 1e-3 and abs(r["pitch"] + math.atan(0.2)) < 1e-3
    r = host_stand("off")
    print("FOLLOW host stand, level targets:", r)
    assert r["first_bad"] is not None and r["first_bad"] < 100
