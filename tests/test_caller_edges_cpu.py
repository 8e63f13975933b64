"""The host side of the caller edge tests (tests/caller_edges.py; the device side is tests/test_caller_edges_gpu.py): wbc::traj_index
compiled for the host (tools/libhost_tick.so: host_traj_index, the source the lookup kernel and the persistent rollout share) against
numpy's argmin on every table x query x hint, and the numpy oracles of the other batches against restatements of their own laws, so that
a failure on the device is not a slip of the oracle.  Each test prints its figures on a CALLER-EDGE line; profiles/r18/caller_edges.md
records them."""
import ctypes as C
import math
import struct

import numpy as np
import pytest

import caller_edges as ce
import host_tick as ht
from oracle import traj_oracle as to
from test_pd import gold


def _perms():
    _, order, act, _, _ = gold("pd_perm")
    return {"identity": (list(range(12)), list(range(12))), "pd_perm": (order, act)}


@pytest.mark.parametrize("name", list(ce.tables()))
def test_host_index_is_numpy_argmin_for_every_time_and_hint(name):
    """host_traj_index == the oracle's index on every query of the table, the three waits and every hint of caller_edges.hints: the
    answer does not depend on the hint, a NaN time included, and is numpy's where the subtraction rounds (+inf, 1e17, 2^53)."""
    L = ht.lib()
    rng = np.random.default_rng(18)
    calls, wrong, by_kind = 0, [], {}
    for wait in ce.WAITS:
        ts, t, idx, _, _ = ce.lookup_case(name, wait)
        K = ts.size
        tsc = np.ascontiguousarray(ts) if K else np.zeros(1)
        p = tsc.ctypes.data_as(C.POINTER(C.c_double))
        hs = ce.hints(K, rng)
        for x, want in zip(t.tolist(), idx.tolist()):
            for h in hs:
                got = L.host_traj_index(p, K, wait, x, h)
                calls += 1
                if got != want:
                    wrong.append((wait, x, h, got, want))
                    kind = "nan" if x != x else "inf" if math.isinf(x) else "huge" if abs(x) >= 2.0 ** 53 else "other"
                    by_kind[kind] = by_kind.get(kind, 0) + 1
    print("CALLER-EDGE host index %-12s K %4d: %6d calls, %d differ from numpy %s" % (name, ts.size, calls, len(wrong), by_kind or ""))
    assert not wrong, wrong[:8]


def test_the_issue_table_on_the_host():
    """ts = 0.25 arange(8), wait 0: numpy answers 0, 0, 6 and 0 for t = inf, 1e17, 2^53 and NaN -- with every hint."""
    L = ht.lib()
    ts = 0.25 * np.arange(8)
    p = ts.ctypes.data_as(C.POINTER(C.c_double))
    got = {x: sorted({L.host_traj_index(p, 8, 0.0, x, h) for h in range(-2, 10)}) for x in (math.inf, 1e17, 2.0 ** 53, math.nan)}
    print("CALLER-EDGE host index issue table: inf %s 1e17 %s 2^53 %s nan %s" % tuple(got[x] for x in list(got)))
    with np.errstate(invalid="ignore"):
        want = [[int(np.abs(ts - x).argmin())] for x in got]
    assert want == [[0], [0], [6], [0]] and list(got.values()) == want


def test_lookup_oracle_is_the_written_law():
    """numpy's argmin on the small tables equals the law as include/wbc.h words it, in plain Python floats: the first index whose rounded
    distance is a NaN, else the first index of the smallest rounded distance; t < wait (false for a NaN) -> standing."""
    n = 0
    for name, wait in ce.lookup_cases():
        ts, t, idx, out, m = ce.lookup_case(name, wait)
        if ts.size > 64:
            continue
        tg, mk, st = ce.table_rows(ts.size)
        for x, got in zip(t.tolist(), idx.tolist()):
            if x < wait or ts.size == 0:
                want = -1
            else:
                tq = x - wait
                d = [abs(s - tq) if not (math.isinf(s) and s == tq) else math.nan for s in ts.tolist()]     # (inf - inf)
                nans = [j for j, y in enumerate(d) if y != y]
                want = nans[0] if nans else d.index(min(d))
            assert got == want, (name, wait, x, got, want)
            n += 1
        sel = idx >= 0
        assert np.array_equal(out[:, sel], tg[idx[sel]].T) and np.array_equal(m[sel], mk[idx[sel]])
        assert (out[:, ~sel] == st[:, None]).all() and (m[~sel] == ce.STANDING_MASK).all()
    print("CALLER-EDGE lookup oracle against the written law: %d queries, 0 differ" % n)
    assert n > 1500


def test_wire_oracles_on_the_edge_words():
    """Unpack: every word of STATE_WORDS reaches every field; the decoded doubles are the float32 values (denormals kept, NaN as NaN).
    Pack: struct.pack raises exactly on PACK_OVER; the rule for them is +-inf; the halfway points round to even."""
    raw, good = ce.state_messages(257)
    assert sorted(np.flatnonzero(~good).tolist()) == [0, 63, 64, 256]
    q, v = ce.decoded_states(raw, good)
    x = np.concatenate([q, v])
    with np.errstate(invalid="ignore"):                              # (widening the signalling NaN raises the flag)
        want = ce.STATE_WORDS.view(np.float32).astype(np.float64)
    for r in range(37):
        col = x[r, good]
        for w in want:
            assert (np.isnan(col).any() if w != w else ((col == w) & (np.signbit(col) == np.signbit(w))).any()), (r, w)
    with pytest.raises(ValueError, match="Decode error"):
        to.robot_state_decode(raw[:204])
    for y in ce.PACK_OVER:
        with pytest.raises(OverflowError):
            struct.pack(">f", y)
        assert ce.pack_word(y) == struct.pack(">f", math.copysign(math.inf, y))
    for y in ce.PACK_IN_RANGE:
        struct.pack(">f", y)
    f = lambda y: struct.unpack(">f", ce.pack_word(y))[0]
    assert f(ce.LAST_IN) == ce.FLT_MAX and f(3.40282356779733e38) == ce.FLT_MAX and f(-ce.LAST_IN) == -ce.FLT_MAX
    assert f(1.0 + 2.0 ** -24) == 1.0 and f(np.nextafter(1.0 + 2.0 ** -24, 2.0)) == 1.0 + 2.0 ** -23 and f(1.0 + 3 * 2.0 ** -24) == 1.0 + 2.0 ** -22
    assert f(2.0 ** -150) == 0.0 and f(np.nextafter(2.0 ** -150, 1.0)) == 2.0 ** -149 and f(3 * 2.0 ** -150) == 2.0 ** -148
    assert 0.0 < f(1e-40) < 2.0 ** -126 and np.signbit(f(-(2.0 ** -150)))
    for order, act in _perms().values():
        tau = ce.control_torques(65)
        words, nan = ce.control_messages(tau, order, act)          # (asserts traj_oracle.robot_control_message inside)
        assert (words[:, 2:39] == 0).all() and nan.sum() > 0
    print("CALLER-EDGE wire oracles: %d state words in 37 fields, %d pack values of which %d past FLT_MAX" % (ce.STATE_WORDS.size, ce.PACK_VALUES.size, ce.PACK_OVER.size))


@pytest.mark.parametrize("gains", list(ce.PD_GAINS))
def test_pd_oracle_is_np_clip_of_its_unclipped_value(gains):
    """pd_control_law == np.clip(unclipped law) bit for bit; the rows do what their names say: NaN exactly on the NaN and inf - inf rows
    (never on others: NaN base rows do not matter), +-u_max on and beyond the bound, u itself one ulp inside, np.clip's signed zeros."""
    g = ce.PD_GAINS[gains]
    for label, (order, act) in _perms().items():
        q, v, which, names = ce.pd_batch(65, gains, order, act)
        u = ce.pd_oracle(q, v, gains, order, act)
        with np.errstate(invalid="ignore", over="ignore"):
            raw = to.pd_control_law(q, v, q_nom=g["q_nom"], order=order, act_joint=act, kp=g["kp"], kd=g["kd"], u_max=np.inf)
            assert np.clip(raw, -g["u_max"], g["u_max"]).tobytes() == u.tobytes()
        nm = np.array(names)[which]
        want_nan = np.isin(nm, ["inf-inf", "-inf+inf", "nan q", "nan v", "nan both"])
        assert np.array_equal(np.isnan(u), want_nan) and (set(names) == set(nm.ravel().tolist()))
        if gains == "zero_box":
            for name, z in (("u=+0", 0.0), ("u=-0", -0.0), ("u=5", 0.0), ("u=-5", -0.0)):
                assert (u[nm == name] == 0).all() and (np.signbit(u[nm == name]) == np.signbit(z)).all(), name
            assert np.clip(np.array([0.0, -0.0, 5.0, -5.0]), -0.0, 0.0).tobytes() == np.array([0.0, -0.0, 0.0, -0.0]).tobytes()
        else:
            um = g["u_max"]
            for name, x in (("u=+max", um), ("u=-max", -um), ("u=+max+ulp", um), ("u=-max-ulp", -um), ("u=+max-ulp", np.nextafter(um, 0)),
                            ("u=-max+ulp", -np.nextafter(um, 0)), ("kp*qe=+inf", -um), ("kp*qe=-inf", um), ("q=+inf", -um), ("q=-inf", um), ("v=+inf", -um)):
                assert (u[nm == name] == x).all(), name
            assert (raw[nm == "u=+max+ulp"] == np.nextafter(um, np.inf)).all() and np.isinf(raw[nm == "kp*qe=+inf"]).all()
            assert (np.abs(u[nm == "inside"]) < um).all()
        print("CALLER-EDGE pd oracle %s %s: %d entries, %d NaN, %d on the bound" % (gains, label, u.size, np.isnan(u).sum(), (np.abs(u) == g["u_max"]).sum()))


@pytest.mark.parametrize("dt", [5e-3, 0.0])
def test_integrate_oracle_at_the_branches_of_the_quaternion_step(dt):
    """to.integrate against its np.longdouble restatement per kind of caller_edges.integrate_batch: 1e-14 holds everywhere but on the
    large angles, whose rates (|w| = 4e5 < 2^19) are themselves rounded to 2^-34 = 5.8e-11 and whose angle of 1e3 rad carries that
    rounding into the quaternion; zero and underflowing rates are the identity rotation; dt = 0 changes nothing but the norm of the
    quaternion."""
    n = 257
    q, v, vd, kind = ce.integrate_batch(n, dt)
    q1, v1 = to.integrate(q, v, vd, dt)
    q80, v80 = ce.integrate_ld(q, v, vd, dt)
    gap = np.maximum(np.abs(q1 - q80).max(0), np.abs(v1 - v80).max(0)).astype(np.float64)
    per = {nm: float(gap[kind == k].max()) for k, nm in enumerate(ce.INTEGRATE_KINDS)}
    print("CALLER-EDGE integrate oracle64 - oracle80, dt %g: %s" % (dt, " ".join("%s %.3g" % kv for kv in per.items())))
    assert all(x < 1e-15 for nm, x in per.items() if nm != "large_angle") and per["large_angle"] < 2.0 ** -34
    assert np.isfinite(q1).all() and np.allclose(np.linalg.norm(q1[:4], axis=0), 1.0, atol=1e-15)
    still = (kind == 1) | (kind == 2) | (dt == 0.0)
    unit = q[:4] / np.sqrt((q[:4] * q[:4]).sum(0))
    assert np.abs(q1[:4, still] - unit[:, still]).max() < 1e-15
    if dt == 0.0:
        assert np.array_equal(v1, v) and np.array_equal(q1[4:], q[4:])
    else:
        assert np.abs(q1[:4, kind == 3] - unit[:, kind == 3]).max() > 0.1           # the large angles really turn
