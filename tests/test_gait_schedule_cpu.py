"""The gait planner's command schedules (include/wbc_gait_schedule.h), no GPU: the host instantiation of the SCHEDULE
law of csrc/wbc_gait.hpp (tests/host_gait_schedule.py) against the numpy restatement of the header (tests/gait_schedule_oracle.py) on
the plane and on a terrain, the exact relations with the plain law, continuity across a switch and a blend's ends, the argument
checks that return before any device is touched, the binding table against the header, the twin under the sanitizers as a
stand-alone program, and the closed loop on the host twins: ID turning, slowing to a stop and reversing.

The bars of the comparison with the oracle are measured here as in tests/test_gait_cpu.py, per row group: 100 x the largest
difference between the oracle in double and in extended precision on the same inputs ("GAIT-SCHEDULE ..." lines print them)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import follow_oracle as fo
import gait_oracle as go
import gait_schedule_oracle as gso
import gait_terrain_oracle as gto
import host_gait as hg
import host_gait_schedule as hgs
import host_gait_terrain as hgt
import plant_edges as pe
import test_gait_cpu as tgc
import test_gait_terrain_cpu as tgt
from quadruped_drake_amd import gait, terrain as tr

ROOT = tgc.ROOT
NEAR = 1e-9
BLENDS = (0.0, 0.1, 0.5)
SWITCHES = (0, 1, 3, 7)


def sample_batch(shift, wait_time):
    """Every third sample of test_gait_cpu.sample_batch's grid (a time every 21.9 ms over 0 .. 20 s, off every boundary of every
    stride at every scale for the reason given there), preceded by its 24 samples with tau < 0; commands (omega = 0, of both signs, and
    2e-5 and 1e-3 rad/s, on either side of the sinc threshold), scales and starts dealt round as there."""
    t, cmd, sc, st = tgc.sample_batch(shift, wait_time)
    keep = np.r_[np.arange(24), np.arange(24, t.size, 3)]
    return t[keep].copy(), cmd[:, keep].copy(), sc[keep].copy(), st[:, keep].copy()


def schedules(n, blend, shift=0):
    """(nswitch [n], when [7, n], cmds [21, n]): instance i has m = 0, 1, 3 or 7 switches, the first at Theta = 1.0137 + 0.37 (i mod 5)
    and each later one blend + 0.9113 + 0.21 ((i + j) mod 3) after the one before -- all seven within the 20 s of samples, none on a
    round number, where a mid-stance lies -- and commands dealt from test_gait_cpu.COMMANDS: omega = 0, +-2, +-2e-5 (|omega theta / 2|
    below 1e-4 on its whole segment) and 1e-3 (which crosses 1e-4 on it).  Rows from m on hold NaN: they are not read."""
    i = np.arange(n) + shift
    m = np.array(SWITCHES)[i % 4].astype(np.uint8)
    when = np.full((7, n), np.nan)
    cmds = np.full((21, n), np.nan)
    th = 1.0137 + 0.37 * (i % 5)
    for j in range(7):
        used = j < m
        when[j, used] = th[used]
        cmds[3 * j:3 * j + 3, used] = np.array(tgc.COMMANDS)[(i + 2 * j + 1) % len(tgc.COMMANDS)].T[:, used]
        th = th + blend + 0.9113 + 0.21 * ((i + j) % 3)
    return m, when, cmds


@pytest.mark.parametrize("ground", ["plane", "terrain"])
@pytest.mark.parametrize("name", list(gait.STRIDES))
def test_host_twin_matches_the_oracle_on_every_stride(name, ground):
    """All ten strides, m = 0, 1, 3 and 7 dealt over the instances, beta = 0, 0.1 and 0.5, on the plane and on follow_oracle's sixteen
    profiles (body fit, lift, fit by blend).  A sample is left out only where a pose evaluation lies within 1e-9 of a Theta_j or of a
    window's end or (terrain) a foothold within 1e-9 of a decision of the terrain law -- at most 1 %, asserted on the oracle alone;
    masks are compared on every sample."""
    P = hg.params(wait_time=0.25)
    S = [gait.stride(name)]
    for k, blend in enumerate(BLENDS):
        t, cmd, sc, st = sample_batch(k, P["wait_time"])
        n = t.size
        assert float(go.boundary_distance(S[0][0], t, P["wait_time"], sc)[24:].min()) >= 1e-9
        m, when, cmds = schedules(n, blend, k)
        kw = {}
        if ground == "terrain":
            profiles, ids, scales = tgt.sixteen()
            kw = dict(profiles=profiles, terrain_id=ids(n), terrain_scale=scales(n), tp=gto.tparams(body=("fit", "lift", "fit")[k], max_grade=tgt.MAX_GRADE))
        got, gmask = hgs.run([name], t, cmd, m, when, cmds, blend, None, sc, st, p=P, **kw)
        info = {}
        want, wmask = gso.targets(P, S, t, cmd, m, when, cmds, blend, None, sc, st, **kw)
        wide, lmask = gso.targets(P, S, t, cmd, m, when, cmds, blend, None, sc, st, dtype=np.longdouble, info=info, **kw)
        keep = (info["near"] >= NEAR) & (info["terrain_near"] >= NEAR)
        print("GAIT-SCHEDULE twin-to-oracle %-12s %-7s beta %.1f left out %d of %d" % (name, ground, blend, int((~keep).sum()), n))
        assert (~keep).sum() <= 0.01 * n
        assert (gmask == wmask).all() and (wmask == lmask).all() and (gmask[:24] == 0xF).all() and np.isfinite(got).all()
        groups = tgc.GROUPS if ground == "plane" else tgt.GROUPS
        for group, rows in groups:
            bar = 100.0 * float(np.abs(want[rows][:, keep] - wide[rows][:, keep]).max())
            worst = float(np.abs(got[rows][:, keep] - wide[rows][:, keep]).max())
            print("GAIT-SCHEDULE twin-to-oracle %-12s %-7s beta %.1f %-14s worst %.3g bar %.3g" % (name, ground, blend, group, worst, bar))
            if bar == 0:                                                              # the lift body's attitude rates: zeros on both sides
                assert worst == 0 and ground == "terrain" and group.startswith("attitude r")
            else:
                assert worst < bar, (name, ground, blend, group, worst, bar)
        # and the schedule did something: the instances with switches end elsewhere than under their first command
        plain = hg.run([name], t, cmd, None, sc, st, p=P)[0]
        late = (m > 0) & (t > 6.0)
        assert np.abs(got[0:2, late] - plain[0:2, late]).max() > 0.5


# ---- exact relations
def _plain(name, t, cmd, sc, st, P, ground):
    if ground == "plane":
        return hg.run([name], t, cmd, None, sc, st, p=P)
    profiles, ids, scales = tgt.sixteen()
    return hgt.run([name], profiles, t, cmd, None, sc, st, ids(t.size), scales(t.size), tp=gto.tparams(max_grade=tgt.MAX_GRADE), p=P)


def _scheduled(name, t, cmd, sc, st, P, ground, m, when, cmds, blend):
    kw = {}
    if ground == "terrain":
        profiles, ids, scales = tgt.sixteen()
        kw = dict(profiles=profiles, terrain_id=ids(t.size), terrain_scale=scales(t.size), tp=gto.tparams(max_grade=tgt.MAX_GRADE))
    return hgs.run([name], t, cmd, m, when, cmds, blend, None, sc, st, p=P, **kw)


@pytest.mark.parametrize("ground", ["plane", "terrain"])
def test_no_switch_and_the_time_before_the_first_switch_give_the_plain_twin_s_bits(ground):
    """m = 0: the plain twin's bits on every sample.  One switch at Theta_1 = 15: the plain twin's bits while all three pose
    evaluations lie before it -- surely for t <= 10 s, the longest stride here being 2 s x scale 2 -- and another answer after it."""
    P = hg.params(wait_time=0.25)
    for name in ("trot", "walk", "gallop"):
        t, cmd, sc, st = sample_batch(1, P["wait_time"])
        n = t.size
        plain, pmask = _plain(name, t, cmd, sc, st, P, ground)
        junk = np.full((7, n), np.nan), np.full((21, n), np.nan)
        got, gmask = _scheduled(name, t, cmd, sc, st, P, ground, np.zeros(n, np.uint8), junk[0], junk[1], 0.5)
        assert pe.same_bits(got, plain) and (gmask == pmask).all()
        when, cmds = np.full((7, n), np.nan), np.full((21, n), np.nan)
        when[0], cmds[0:3] = 15.0, np.array([[0.3], [0.2], [-0.7]])
        got, gmask = _scheduled(name, t, cmd, sc, st, P, ground, np.ones(n, np.uint8), when, cmds, 0.5)
        early, late = t <= 10.0, t > 16.5
        assert early.sum() > 400 and late.sum() > 100 and (gmask == pmask).all()
        assert pe.same_bits(got[:, early], plain[:, early]) and np.abs(got[0:2, late] - plain[0:2, late]).min() > 1e-3


def test_a_switch_to_the_same_command_without_a_blend_changes_no_row_by_more_than_the_bar():
    """Three switches to the command the instance already walks, beta = 0: S_j = E_j and the arc goes on, to rounding.  The bar per row
    group is the oracle's, 100 x its double's distance from its extended twin on these inputs."""
    P = hg.params(wait_time=0.25)
    for name in ("trot", "pace"):
        t, cmd, sc, st = sample_batch(2, P["wait_time"])
        n = t.size
        m, when, _ = schedules(n, 0.0)
        m[:] = 3
        when = np.tile(np.array([1.0137, 4.3, 9.77, 0, 0, 0, 0])[:, None], (1, n))
        cmds = np.tile(cmd, (7, 1))
        got, gmask = hgs.run([name], t, cmd, m, when, cmds, 0.0, None, sc, st, p=P)
        plain, pmask = hg.run([name], t, cmd, None, sc, st, p=P)
        want = gso.targets(P, [gait.stride(name)], t, cmd, m, when, cmds, 0.0, None, sc, st)[0]
        wide = gso.targets(P, [gait.stride(name)], t, cmd, m, when, cmds, 0.0, None, sc, st, dtype=np.longdouble)[0]
        assert (gmask == pmask).all() and not pe.same_bits(got, plain)
        for group, rows in tgc.GROUPS:
            bar = 100.0 * float(np.abs(want[rows] - wide[rows]).max())
            worst = float(np.abs(got[rows] - plain[rows]).max())
            print("GAIT-SCHEDULE same command %-5s %-13s worst %.3g bar %.3g" % (name, group, worst, bar))
            assert worst < bar


# ---- continuity
def test_central_differences_reproduce_the_rates_across_a_switch_and_a_blend_s_ends():
    """Trot at scale 1, ramp 0.5 s: (0.5, 0.1, 0.4) -> (0.2, -0.1, -0.6) at t = 2.1 s (Theta 1.85, in mid-swing of LF and RH), beta 0.5,
    so the blend ends at t = 2.6 s (mid-swing of RF and LH); a second switch at 3.2 s.  61 times 2 us apart around each of the two
    junctions, central differences of step h = 1e-5 s, all of which straddle the junction: pd and pdd of the body and of every foot
    against the differences of p and pd.  P is C2 there, so what a difference leaves is its truncation, h^2 / 6 times a bounded third
    derivative, and the twin's rounding on top: the twin is held to ten times what the extended-precision oracle's own difference
    leaves.  Measured (profiles/r15/gait_schedule.md): the oracle leaves 4.83e-9 (pd) and 5.14e-5 (pdd), and so does the twin; without
    the blend (beta = 0) the velocity jumps and the same difference leaves 0.46."""
    P = hg.params()
    S = ["trot"]
    h = 1e-5
    t = np.concatenate([x + (np.arange(-30, 31) + 0.37) * 2e-6 for x in (2.1, 2.6)])
    n = t.size
    cmd = np.tile([[0.5], [0.1], [0.4]], (1, n))
    m = np.full(n, 2, np.uint8)
    when, cmds = np.zeros((7, n)), np.zeros((21, n))
    when[0], when[1] = gait.path_parameter(P["ramp_time"], 2.1), gait.path_parameter(P["ramp_time"], 3.2)
    cmds[0:3], cmds[3:6] = np.array([[0.2], [-0.1], [-0.6]]), np.array([[0.0], [0.3], [0.0]])
    assert when[0, 0] == 1.85
    wide = lambda x, b: gso.targets(P, [gait.stride("trot")], x, cmd[:, :x.size], m[:x.size], when[:, :x.size], cmds[:, :x.size], b,
                                    dtype=np.longdouble)[0]
    twin = lambda x, b: hgs.run(S, x, cmd, m, when, cmds, b, p=P)[0]
    left = {}
    for label, f in (("oracle", wide), ("twin", twin)):
        lo, hi = t - h, t + h
        span = (hi.astype(np.longdouble) - lo.astype(np.longdouble)) if label == "oracle" else hi - lo
        mid, a, b = f(t, 0.5), f(lo, 0.5), f(hi, 0.5)
        for order, (src, dst) in enumerate(((tgc.POS, tgc.VEL), (tgc.VEL, tgc.ACC))):
            worst = float(np.abs((b[src] - a[src]) / span - mid[dst]).max())
            left[label, order] = worst
            print("GAIT-SCHEDULE central difference %s %s: leaves %.3g" % (label, ("pd", "pdd")[order], worst))
    for order in (0, 1):
        assert 0 < left["oracle", order] < (1e-6, 1e-4)[order]            # h^2 / 6 x 1e4 and x 1e6: the swing's third and fourth derivative
        assert left["twin", order] < 10.0 * left["oracle", order]
    # the same difference sees the jump of a switch without a blend
    jump = float(np.abs((wide(t[:61] + h, 0.0)[tgc.POS] - wide(t[:61] - h, 0.0)[tgc.POS]) / (2 * h) - wide(t[:61], 0.0)[tgc.VEL]).max())
    print("GAIT-SCHEDULE central difference across a switch with beta = 0: leaves %.3g" % jump)
    assert jump > 0.1


# ---- malformed instances
def test_an_invalid_schedule_gets_nan_rows_and_a_full_mask_and_its_neighbours_nothing():
    P = hg.params()
    rng = np.random.default_rng(11)
    cases = [("m", 8), ("m", 255), ("when0", -1e-3), ("when0", math.nan), ("when2", math.inf), ("order", None), ("tight", None),
             ("cmd", math.nan), ("cmd", -math.inf)]
    n = 3 * len(cases) + 2
    t = rng.uniform(0.0, 12.0, n)
    cmd = np.stack([rng.uniform(-1, 1, n), rng.uniform(-0.5, 0.5, n), rng.uniform(-2, 2, n)])
    m, when, cmds = schedules(n, 0.5)
    m[:] = 3
    when, cmds = np.nan_to_num(when, nan=0.0), np.nan_to_num(cmds, nan=0.0)
    when[0], when[1], when[2] = 1.0, 2.5, 4.25
    cmds[0:9] = rng.uniform(-1, 1, (9, n))
    dm, dw, dc = m.copy(), when.copy(), cmds.copy()
    bad = np.zeros(n, bool)
    for k, (case, value) in enumerate(cases):
        i = 3 * k + 1
        bad[i] = True
        if case == "m":
            dm[i] = value
        elif case.startswith("when"):
            dw[int(case[-1]), i] = value
        elif case == "order":
            dw[1, i], dw[2, i] = dw[2, i], dw[1, i]
        elif case == "tight":
            dw[2, i] = dw[1, i] + 0.5 - 1e-9          # Theta_3 < Theta_2 + beta
        else:
            dc[4, i] = value
    ct, cm = hgs.run(["trot"], t, cmd, m, when, cmds, 0.5, p=P)
    dt_, dmk = hgs.run(["trot"], t, cmd, dm, dw, dc, 0.5, p=P)
    ot, om = gso.targets(P, [gait.stride("trot")], t, cmd, dm, dw, dc, 0.5)
    assert np.isfinite(ct).all() and np.isnan(dt_[:, bad]).all() and (dmk[bad] == 0xF).all()
    assert pe.same_bits(dt_[:, ~bad], ct[:, ~bad]) and (dmk[~bad] == cm[~bad]).all()
    assert np.array_equal(np.isnan(ot), np.isnan(dt_)) and (om == dmk).all()
    # Theta_3 = Theta_2 + beta exactly is valid
    dw2 = when.copy()
    dw2[2] = dw2[1] + 0.5
    assert np.isfinite(hgs.run(["trot"], t, cmd, m, dw2, cmds, 0.5, p=P)[0]).all()
    assert hgs.run(["trot"], t, cmd, m, when, cmds, -0.1, p=P, rc=True) == -5 and hgs.run(["trot"], t, cmd, m, when, cmds, math.nan, p=P, rc=True) == -5


# ---- what returns before any device is touched, and the binding
def test_abi_gait_schedule_misuse_without_device():
    from quadruped_drake_amd import _lib
    L = _lib.lib()
    err = lambda: L.wbc_last_error().decode()
    P = hg.params()
    cp = gait.c_params(P["stance"], P["height"], P["swing_height"], P["ramp_time"], P["wait_time"])
    h = C.c_void_p()
    assert L.wbc_gait_create(C.byref(cp), gait.c_strides(["trot"]), 1, 0, C.byref(h)) == 0
    ns, wh, cm = np.zeros(4, np.uint8), np.zeros((7, 4)), np.zeros((21, 4))
    p = lambda a: C.c_void_p(a.ctypes.data)
    f = L.wbc_gait_set_schedule
    assert f(None, None, 4, 4, 0.5, p(ns), p(wh), p(cm)) < 0 and "null gait handle" in err()
    for args in ((None, p(wh), p(cm)), (p(ns), None, p(cm)), (p(ns), p(wh), None)):
        assert f(h, None, 4, 4, 0.5, *args) < 0 and "are required" in err()
    for blend in (-0.1, math.nan, math.inf, -math.inf):
        assert f(h, None, 4, 4, blend, p(ns), p(wh), p(cm)) < 0 and "blend" in err()
    for n, ld, what in ((0, 4, "n out of range"), (-1, 4, "n out of range"), ((1 << 23) + 1, 1 << 24, "n out of range"), (4, 3, "ld must be >= n"),
                        (4, (1 << 23) + 1, "WBC_MAX_LD")):
        assert f(h, None, n, ld, 0.5, p(ns), p(wh), p(cm)) < 0 and what in err(), (n, ld, err())
    assert f(h, None, 4, 4, 0.5, p(ns), p(wh), p(cm)) < 0 and "wbc_gait_set_commands" in err()
    assert L.wbc_gait_clear_schedule(None) < 0 and "null gait handle" in err()
    assert L.wbc_gait_clear_schedule(h) == 0                                    # nothing set: nothing to clear
    assert L.wbc_gait_schedule_kernel_info(None, 0, None, None, None, None) < 0 and "null gait handle" in err()
    assert L.wbc_gait_destroy(h) == 0
    # the Python layer's own checks (numpy only)
    nsw, when, cmds = gait.schedule_arrays([1.5, 2.5], [(0.4, 0, 0.5), (0.2, 0, 0)], 3, 0.5)
    assert (nsw == 2).all() and nsw.dtype == np.uint8 and when.shape == (7, 3) and cmds.shape == (21, 3)
    assert (when[0] == 1.25).all() and (when[1] == 2.25).all() and np.isinf(when[2:]).all() and (cmds[0:6, 1] == [0.4, 0, 0.5, 0.2, 0, 0]).all()
    nsw, when, cmds = gait.schedule_arrays([[1.5, 0.5], [2.5, np.inf]], np.zeros((2, 3, 2)), 2, 0.5)
    assert list(nsw) == [2, 1] and when[0, 1] == 0.25
    assert gait.path_parameter(0.5, 0.25) == 0.5 * (2.5 / 16 - 3 / 32 + 1 / 64) and gait.path_parameter(0.0, 1.5) == 1.5
    for times, cm_ in (([0.4], [(0, 0, 0)]), ([1.0] * 8, [(0, 0, 0)] * 8), ([1.0], [(0, 0)]), ([[np.inf, 1.0], [2.0, 2.0]], np.zeros((2, 3, 2))), ([math.nan], [(0, 0, 0)])):
        with pytest.raises(ValueError):
            gait.schedule_arrays(times, cm_, 2, 0.5)
    g = object.__new__(gait.GaitPlanner)
    g._n = g._h = None
    with pytest.raises(ValueError, match="set_commands"):
        g.set_schedule([1.0], [(0, 0, 0)])


def test_the_twin_runs_clean_under_the_sanitizers_as_a_stand_alone_program(tmp_path):
    """tools/host_gait_schedule_check.cpp + tools/host_gait.cpp built with -fsanitize=address,undefined (no recovery) and run: every m,
    an invalid schedule, both blends, the plane and a terrain, arrays exactly as long as the batch."""
    exe = tmp_path / "check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                    os.path.join(ROOT, "tools", "host_gait_schedule_check.cpp"), os.path.join(ROOT, "tools", "host_gait.cpp")],
                   check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "0 rows out of place" in r.stdout and not r.stderr


def test_simulate_cmd_schedule_arguments():
    from quadruped_drake_amd import simulate
    base = ["--planner", "gait", "--plant", "ground"]
    a = simulate.parse(base + ["--cmd-schedule", "1.5:0.4,0,0.5;2.5:0.2,0,0;3.2:0,0,0"])
    assert a.cmd_schedule == [(1.5, (0.4, 0.0, 0.5)), (2.5, (0.2, 0.0, 0.0)), (3.2, (0.0, 0.0, 0.0))] and a.cmd_blend == 0.5
    assert simulate.parse(base).cmd_schedule is None
    assert simulate.parse(base + ["--cmd-schedule", "0.5:0,0,0", "--cmd-blend", "0"]).cmd_blend == 0.0
    for argv in (base + ["--cmd-schedule", "1.5:0.4,0"], base + ["--cmd-schedule", "0.4:0,0,0"], base + ["--cmd-schedule", "1.5:0,0,0;1.9:0,0,0"],
                 base + ["--cmd-schedule", "1.5:0,0,0", "--cmd-blend", "-1"], base + ["--cmd-schedule", ";".join(["%d:0,0,0" % k for k in range(1, 9)])],
                 base + ["--cmd-schedule", "x"], ["--cmd-schedule", "1.5:0,0,0"]):
        with pytest.raises(SystemExit):
            simulate.parse(argv)
    assert "--cmd-schedule" in simulate.__doc__


# ---- the closed loop on the host twins
FELL, BAD = tgc.FELL, tgc.BAD
TURN = ((0.2, 0.0, 0.0), [1.5, 2.5, 3.2], [(0.4, 0.0, 0.5), (0.2, 0.0, 0.0), (0.0, 0.0, 0.0)])
REVERSE = ((0.2, 0.0, 0.0), [1.5], [(-0.2, 0.0, 0.0)])
WALKS = {"turn_slow_stop": (TURN, None), "reverse": (REVERSE, None), "turn_slow_stop_kerb": (TURN, lambda: tr.ramp_step(0.3, 0.10))}
BLEND = 0.5


def host_walk(case, blend=BLEND, ticks=800, dt=5e-3, scale=0.5, model="mini_cheetah", accumulate=False, trace=None):
    """test_gait_cpu.host_walk's loop under a schedule: gait under the schedule (host_gait_schedule; on a terrain its FIT law) -> tick
    (host_tick, ID) -> ground step (host_ground / host_terrain), from workloads.nominal_state.  case: ((c_0, times [s], commands), a
    terrain.Profile maker or None).  The gait is asked at k dt, or (accumulate) at the clock of wbc_ground_rollout, which adds dt to the
    time tick by tick: after 800 ticks of 5 ms that clock reads 3.999999999999937, and where k dt is a boundary of the stride the two
    fall on different sides of it.  trace (a list, optional) <- (q, flags) after every tick.  -> dict(status, flags, x, y, z, dx, dy, off: the trunk's final distance from the planned body
    position, plan: the planned body position)"""
    import host_ground as hgr
    import host_terrain as ht
    import host_tick as hk
    from quadruped_drake_amd import workloads
    from quadruped_drake_amd.controller import load_model
    (c0, times, cs), make = case
    prof = make() if make else None
    t = load_model(model)
    q, v = workloads.nominal_state(model, 1)
    P = hg.params(model)
    m, when, cmds = gait.schedule_arrays(times, cs, 1, P["ramp_time"])
    when, cmds = np.where(np.isinf(when), 0.0, when), cmds
    c = np.array(c0, dtype=np.float64)[:, None]
    sc = np.array([scale])
    kw = {} if prof is None else dict(profiles=[prof], tp=gto.tparams(body="fit"))
    out = dict(status=0, flags=0)
    now = 0.0
    for k in range(ticks):
        tg, mask = hgs.run(["trot"], np.array([now if accumulate else k * dt]), c, m, when, cmds, blend, None, sc, None, p=P, **kw)
        now = now + dt
        tau, _, status, _ = hk.run("id", t["flat"], q, v, tg, mask, act_perm=t.get("act_perm"))
        if prof is None:
            o = hgr.run(t["flat"], q, v, tau, act_perm=t.get("act_perm"), dt=dt)
        else:
            o = ht.run(t["flat"], q, v, tau, act_perm=t.get("act_perm"), dt=dt, profiles=[prof])
        q, v = o["q"], o["v"]
        out["status"] += int(status[0] != 0)
        out["flags"] |= int(o["flags"][0])
        if trace is not None:
            trace.append((q[:, 0].copy(), int(o["flags"][0])))
        if o["flags"][0] & BAD:
            break
    plan = gso.targets(P, [gait.stride("trot")], np.array([ticks * dt]), c, m, when, cmds, blend, None, sc, **kw)[0][:, 0]
    out.update(x=float(q[4, 0]), y=float(q[5, 0]), z=float(q[6, 0]), dx=float(q[4, 0] - plan[0]), dy=float(q[5, 0] - plan[1]), plan=plan[0:3])
    out["off"] = math.hypot(out["dx"], out["dy"])
    return out


@pytest.mark.parametrize("case", list(WALKS))
def test_id_turns_slows_to_a_stop_and_reverses_on_the_host_twins(case):
    """Mini Cheetah, ID, dt 5 ms, trot at stride scale 0.5, 800 ticks on the compliant ground, beta = 0.5, commands that
    tests/test_gait_cpu.py walks as constants: (0.2, 0, 0) -> (0.4, 0, 0.5) at 1.5 s -> (0.2, 0, 0) at 2.5 s -> (0, 0, 0) at 3.2 s; (0.2, 0, 0)
    -> (-0.2, 0, 0) at 1.5 s; and the first again over the kerb ramp_step(0.3, 0.10) with the terrain gait in FIT.  No FELL, no BAD,
    status 0 on every tick, the final trunk within 0.03 m of the plan in x-y (test_gait_cpu's bar).  Measured
    (profiles/r15/gait_schedule.md), x and y off the plan: -0.29 mm and +3.91 mm; +2.28 mm and +5.71 mm; -0.46 mm and +4.58 mm.  Every
    transition holds at beta = 0.5: no case needed a longer blend."""
    r = host_walk(WALKS[case])
    print("GAIT-SCHEDULE host walk %s: x %.4f y %.4f z %.4f plan (%.4f, %.4f, %.4f) dx %+.5f dy %+.5f flags %d status %d" %
          (case, r["x"], r["y"], r["z"], r["plan"][0], r["plan"][1], r["plan"][2], r["dx"], r["dy"], r["flags"], r["status"]))
    assert not r["flags"] & (FELL | BAD) and r["status"] == 0
    assert r["off"] < 0.03
