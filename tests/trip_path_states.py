"""Sixteen 4-contact stands, each pushed so that a DIFFERENT friction row is the first one its active set adds (tests/test_trip_path_*.py).

Friction row h = 4 * leg + r lives on lane h of the robot's 16-lane row; the active set fetches the picked row's image from that lane through the
lane crossbar (csrc/wbc_hex.hpp: hex_gi, `bcast16d`).  A batch whose first picks are rows 0 ... 15 therefore reads from every source lane of that fetch.

Robot h stands in the nominal pose (simulate.py:171-176, planners/simple.py:39-85) and is asked for a body acceleration along +-x or +-y: the feet must
push sideways, beyond the friction cone.  Which foot gives way first is the one with the least load, and that is steered with angular accelerations
about the roll and pitch axes (they shift the load between left / right and front / hind feet).  PUSH[h] = (axis, linear acceleration [m/s^2], roll
acceleration, pitch acceleration [rad/s^2]) was found by a grid search on the host instantiation of the kernel header; first_picks() below is that
check, and tests/test_trip_path_states_cpu.py runs it for both friction-only laws."""
import ctypes as C

import numpy as np

PUSH = [
    (0, +4.0, -150.0, 0.0), (0, -8.0, -150.0, 150.0), (1, +4.0, 150.0, 50.0), (1, -4.0, -400.0, 50.0),
    (0, +4.0, 50.0, 0.0), (0, -8.0, 150.0, 150.0), (1, +4.0, 400.0, 50.0), (1, -8.0, -400.0, 50.0),
    (0, +4.0, -150.0, -50.0), (0, -4.0, -150.0, 0.0), (1, +4.0, 150.0, -50.0), (1, -4.0, -400.0, -50.0),
    (0, +4.0, 150.0, -50.0), (0, -4.0, 50.0, 0.0), (1, +4.0, 400.0, 0.0), (1, -8.0, -400.0, -50.0),
]


def make_states():
    """q[19, 16], v[18, 16], targets[54, 16], mask[16]: robot h is meant to add friction row h first."""
    from quadruped_drake_amd import workloads
    n = len(PUSH)
    q, v = workloads.nominal_state("mini_cheetah", n)
    tg = workloads.standing_targets("mini_cheetah", n)
    for h, (axis, acc, roll, pitch) in enumerate(PUSH):
        tg[6 + axis, h] = acc       # pdd_body
        tg[15, h] = roll            # rpydd_body
        tg[16, h] = pitch
    return q, v, tg, np.full(n, 0xF, np.uint8)


def first_picks(kind, q, v, tg, mask):
    """The row each robot's active set adds first, RECORDED by the host instantiation of hex_gi itself (tools/host_tick.cpp: host_gi_adds -- the ids of the rows
    in the order of the adds, whatever the pick rule, the apex rule and the key packing of the day make of the state).  Returns (rows, margins, adds): the
    margin is the relative distance of the winner's key to the runner-up's, from hex_gi's inputs (host_gi_dump) under today's rule restated here -- MPTC the
    greatest dual gain s^2 / |D|^2 among the violated rows, ID the most violated row -- and says only how far the recorded pick is from a tie (the pick keys
    drop their low 24 mantissa bits: far above 2^-28 no rounding difference between host and device changes it); the restated winner must BE the recorded one."""
    import host_tick as ht
    from oracle import oracle_py as orc
    n = q.shape[1]
    L = ht.lib()
    buf = np.zeros((n, 16, 16))
    L.host_gi_dump(buf.ctypes.data_as(C.c_void_p))
    adds = np.zeros((n, 32), np.int32)
    L.host_gi_adds(adds.ctypes.data_as(C.c_void_p))
    try:
        out = ht.run(kind, orc.load_model_json("mini_cheetah")["flat"], q, v, tg, mask, hexv=True)
    finally:
        L.host_gi_dump(None)
        L.host_gi_adds(None)
    assert (out[2] == 0).all()
    assert (adds[:, 0] >= 1).all(), adds[:, 0]            # every robot added a row
    rows, margins = [], []
    for i in range(n):
        Jr, z, mu_n, inv_s = buf[i, :, :12], buf[i, :, 13].copy(), buf[i, :, 14], buf[i, :, 15]
        z[3] = 0.0                                   # lane (0, 3) owns no variable
        tol = 1e-13 * (1.0 + np.abs(z).max())
        keys = np.full(16, np.inf)
        for h in range(16):
            leg, sb = h >> 2, h & 3
            if inv_s[h] == 0.0:                      # not a contact leg
                continue
            sg = inv_s[h] if sb & 1 else -inv_s[h]   # n_h = sg e_(leg, sb >> 1) + mu_n e_(leg, 2)
            a, b = 4 * leg + (sb >> 1), 4 * leg + 2
            s = sg * z[a] + mu_n[h] * z[b]
            D = sg * Jr[a] + mu_n[h] * Jr[b]
            if s < -tol:
                keys[h] = -(s * s) / (D @ D) if kind == "mptc" else s
        order = np.argsort(keys)
        assert np.isfinite(keys[order[0]]), "robot %d violates no friction row" % i
        assert int(order[0]) == adds[i, 1], (i, int(order[0]), adds[i, :4])
        rows.append(int(adds[i, 1]))
        margins.append(float((keys[order[1]] - keys[order[0]]) / abs(keys[order[0]])) if np.isfinite(keys[order[1]]) else np.inf)
    return rows, margins, adds
