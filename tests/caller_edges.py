"""Edge batches of the kernels that feed and drain the tick (csrc/wbc_traj.hip, wbc_integrate / the rollout's clock in wbc_kernels.hip,
wbc::traj_index of wbc_traj_dev.hpp), defined once so that tests/test_caller_edges_cpu.py and tests/test_caller_edges_gpu.py run
identical inputs: lookup tables and query times at the ties and roundings of numpy's argmin, float32 words and doubles at the edges of
the wire format, PD rows on and next to the clip, angular rates at the branches of the quaternion step, and the batch sizes at the
tails of the 64- and 256-thread blocks.  References: oracle/traj_oracle.py (numpy, struct).  Test infrastructure only: no GPU, no
fixtures of its own; arrays with ld > n come from plant_edges.wide."""
import functools
import math
import struct

import numpy as np

from oracle import traj_oracle as to

NS = (1, 63, 64, 65, 255, 256, 257)        # the tails of the 64-thread (lookup, integrate) and 256-thread (unpack, pack, PD) blocks
PAD = 5                                    # ld = n + PAD
WAITS = (0.0, 0.5, -0.25)
HUGE = (2.0 ** 53, 1e17, 1e300)
STANDING_MASK = 0xC3


# ---- lookup: tables whose sample k carries its own index (row r of sample k is 64 k + r, exactly), standing rows -1 - r
def tables():
    """name -> timestamps.  Binary-exact values wherever a tie is meant to be a tie."""
    return {
        "empty": np.zeros(0),
        "one": np.array([0.75]),
        "two": np.array([0.25, 1.0]),
        "towr_1ms": np.arange(5001) * 1e-3,
        "all_equal": np.full(7, 1.5),
        "dup_start": np.array([0.0, 0.0, 0.0, 0.25, 0.5, 0.75, 1.0]),
        "dup_middle": np.array([0.0, 0.25, 0.5, 0.5, 0.5, 0.5, 0.75, 1.0]),
        "dup_end": np.array([0.0, 0.25, 0.5, 0.75, 0.75, 0.75]),
        "quarters": 0.25 * np.arange(8),
        "geometric": 2.0 ** np.arange(-20, 12),
        "negative": 0.25 * np.arange(-12.0, 0.0),
        "offset_2p30": 2.0 ** 30 + 2.0 ** -24 * np.arange(40),         # spacing below the ulp (2^-22): the sum rounds to runs of equal timestamps
        "last_inf": np.array([0.0, 0.25, 0.5, 0.75, 1.0, np.inf]),
        "last_two_inf": np.array([0.0, 0.25, 0.5, np.inf, np.inf]),
        "first_ninf": np.array([-np.inf, 0.0, 0.25, 0.5, 0.75]),
    }


def table_rows(K):
    """(targets [K, 54], masks [K], standing [54]) of a table of K samples"""
    tg = 64.0 * np.arange(K)[:, None] + np.arange(54.0)[None, :]
    return tg, ((37 * np.arange(K) + 11) & 0xFF).astype(np.uint8), -1.0 - np.arange(54.0)


def queries(ts, wait):
    """Every sample time, every midpoint and its two neighbours in double, before the first and after the last sample, the wait and
    its neighbours, NaN, +-inf and the huge finite times -- as query times t (the law looks up t - wait)."""
    near = lambda x: [x, np.nextafter(x, -np.inf), np.nextafter(x, np.inf)]
    with np.errstate(invalid="ignore", over="ignore"):
        q = [ts + wait]
        if ts.size > 1:
            q += near(0.5 * (ts[:-1] + ts[1:]) + wait)
        if ts.size:
            q.append(np.array([ts[0] + wait - 1.0, ts[0] + wait - 2.0 ** -10, ts[-1] + wait + 2.0 ** -10, ts[-1] + wait + 1.0]))
        q.append(np.array(near(wait) + [np.nan, np.inf, -np.inf] + list(HUGE)))
        return np.concatenate(q)


def oracle_index(ts, wait, t):
    """traj_oracle.lookup on the indexed table -> sample index per query (-1: the standing targets), and its rows and masks"""
    tg, mk, st = table_rows(ts.size)
    with np.errstate(invalid="ignore", over="ignore"):
        out, m = to.lookup(t, ts, tg, mk, st, STANDING_MASK, wait)
    idx = np.where(out[0] < 0, -1, out[0] / 64.0).astype(np.int64)
    assert np.array_equal(np.where(idx < 0, st[5], 64.0 * idx + 5.0), out[5])
    return idx, out, m


@functools.lru_cache(maxsize=None)
def lookup_case(name, wait):
    """(ts, t, index, rows [54, n], masks [n]) of one table and wait: computed once, shared by every test, never written to"""
    ts = tables()[name]
    t = queries(ts, wait)
    idx, out, m = oracle_index(ts, wait, t)
    for a in (ts, t, idx, out, m):
        a.setflags(write=False)
    return ts, t, idx, out, m


def lookup_cases():
    return [(name, wait) for name in tables() for wait in WAITS]


def hints(K, rng):
    if K <= 64:
        return list(range(-2, K + 2))
    return [-5, 0, K // 2, K - 1, K + 7] + [int(x) for x in rng.integers(0, K, 8)]


# ---- wire format
def _f32(word):
    return struct.unpack(">f", struct.pack(">I", word))[0]


# float32 words of a state message: +-0, the smallest and the largest denormal of either sign, +-FLT_MAX, +-inf, a quiet and a
# signalling NaN, and three ordinary values
STATE_WORDS = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000,
                        0xFF800000, 0x7FC00000, 0x7F800001, 0x3FC00000, 0xBB343958, 0x00800000], np.uint32)
BAD_BYTE = {0: 0, 63: 7, 64: 3}            # column -> the fingerprint byte that is wrong there (column n - 1: byte 4)


def bad_columns(n):
    return {c: b for c, b in list(BAD_BYTE.items()) + [(n - 1, 4)] if 0 <= c < n}


def state_messages(n):
    """n messages of 204 bytes: field r of message i holds STATE_WORDS[(i + r) mod 15], so every word visits every one of the 37 fields
    within fifteen messages; the twelve torque words (not decoded on the device) hold a NaN.  Messages at bad_columns(n) carry a wrong
    fingerprint, each in another byte.  -> (bytes, good [n] bool)"""
    i, r = np.arange(n)[:, None], np.arange(37)[None, :]
    words = STATE_WORDS[(i + r) % STATE_WORDS.size]
    good = np.ones(n, bool)
    out = []
    for k in range(n):
        fp = bytearray(to.RS_FINGERPRINT)
        if k in bad_columns(n):
            fp[bad_columns(n)[k]] ^= 0x40
            good[k] = False
        out.append(bytes(fp) + struct.pack(">37I", *[int(w) for w in words[k]]) + struct.pack(">12I", *([0x7FC01234] * 12)))
    return b"".join(out), good


def decoded_states(raw, good):
    """traj_oracle.robot_state_decode of the good messages -> q [19, n], v [18, n] (columns of rejected messages: NaN, never compared)"""
    n = good.size
    q, v = np.full((19, n), np.nan), np.full((18, n), np.nan)
    for k in np.flatnonzero(good):
        q[:, k], v[:, k], _ = to.robot_state_decode(raw[204 * k:204 * k + 204])
    return q, v


FLT_MAX = _f32(0x7F7FFFFF)
OVER_HALF = float.fromhex("0x1.ffffffp127")                    # halfway between FLT_MAX and 2^128: round-to-even goes up, out of float32
LAST_IN = float(np.nextafter(OVER_HALF, 0.0))                 # the largest double that rounds to FLT_MAX
_near = lambda x: [float(np.nextafter(x, -np.inf)), x, float(np.nextafter(x, np.inf))]
# doubles of a control message that struct.pack('>f') encodes: float32 halfway points and both neighbours, doubles that round to float32
# denormals, the denormal halfway point 2^-150 (to even: 0) and its neighbours, the largest double that still rounds to FLT_MAX, +-inf
# and NaN, and their negatives
_IN = (_near(1.0 + 2.0 ** -24) + _near(1.0 + 3 * 2.0 ** -24) + [1e-40, 1.1754942e-38, 2.0 ** -149, 2.0 ** -126] + _near(2.0 ** -150)
       + _near(3 * 2.0 ** -150) + [3.40282356779733e38, LAST_IN, FLT_MAX, 0.0, 1.0 + 2.0 ** -23, 12.375, np.inf])
PACK_IN_RANGE = np.array(_IN + [-x for x in _IN] + [np.nan])
# ... and the doubles past FLT_MAX, where struct.pack raises and the device writes +-inf (include/wbc_extras.h)
_OVER = [OVER_HALF, float(np.nextafter(OVER_HALF, np.inf)), 2.0 ** 128, 1e39, 1e300, 1.7976931348623157e308]
PACK_OVER = np.array(_OVER + [-x for x in _OVER])
PACK_VALUES = np.concatenate([PACK_IN_RANGE, PACK_OVER])


def pack_word(x):
    """The four bytes of one torque: struct.pack('>f'), and +-inf where that raises"""
    try:
        return struct.pack(">f", x)
    except OverflowError:
        return struct.pack(">f", math.copysign(math.inf, x))


def control_torques(n, values=PACK_VALUES):
    """tau [12, n]: actuator k of robot i holds values[(i + 5 k) mod len]: every value on every actuator within len robots"""
    i, k = np.arange(n)[None, :], np.arange(12)[:, None]
    return values[(i + 5 * k) % values.size]


def control_messages(tau, order, act):
    """-> (words [n, 51] uint32 as read big-endian from the expected messages, nan [n, 51] bool): traj_oracle.robot_control_message's
    layout (msg.tau[order[act[k]]] = u[k], q and v zero) with pack_word per torque; where no torque of a robot is past FLT_MAX the
    bytes ARE traj_oracle.robot_control_message's (asserted here), NaN torques aside, whose payload nobody pins."""
    n = tau.shape[1]
    words = np.zeros((n, 51), np.uint32)
    for i in range(n):
        t = np.zeros(12)
        for k in range(12):
            t[order[act[k]]] = tau[k, i]
        msg = to.RS_FINGERPRINT + struct.pack(">37f", *([0.0] * 37)) + b"".join(pack_word(x) for x in t)
        if (np.abs(t[np.isfinite(t)]) < OVER_HALF).all():           # (struct.pack encodes +-inf and NaN)
            assert same_messages(msg, to.robot_control_message(tau[:, i], order, act))
        words[i] = np.frombuffer(msg, dtype=">u4")
    nan = ((words & 0x7F800000) == 0x7F800000) & ((words & 0x007FFFFF) != 0)
    nan[:, :39] = False
    return words, nan


def same_messages(a, b):
    """Equal bytes, NaN words compared as "is a NaN" only"""
    wa, wb = np.frombuffer(a, dtype=">u4"), np.frombuffer(b, dtype=">u4")
    isnan = lambda w: ((w & 0x7F800000) == 0x7F800000) & ((w & 0x007FFFFF) != 0)
    return wa.shape == wb.shape and np.array_equal(isnan(wa), isnan(wb)) and np.array_equal(wa[~isnan(wa)], wb[~isnan(wb)])


# ---- PD
PD_GAINS = {"default": dict(kp=30.0, kd=1.5, u_max=150.0, q_nom=None),
            "other": dict(kp=41.5, kd=0.75, u_max=33.0,
                          q_nom=np.array([1.0, 0.0, 0.0, 0.0, 0.1, -0.2, 0.4] + [0.125, -0.6875, 1.3125, -0.0625, -0.9375, 1.75] * 2)),
            "zero_box": dict(kp=30.0, kd=1.5, u_max=0.0, q_nom=None)}
_DEFAULT_NOM = np.array([1.0, 0, 0, 0, 0, 0, 0.3] + [0.0, -0.8, 1.6] * 4)


def _rate_for(u, kd):
    """A joint rate v with -(0.0) - kd v == u exactly (angle error zero), found among the neighbours of -u / kd"""
    v = -u / kd
    for cand in [v] + [x for k in range(1, 9) for x in (_step(v, k), _step(v, -k))]:
        if -0.0 - kd * cand == u:
            return cand
    raise AssertionError((u, kd))


def _step(x, k):
    for _ in range(abs(k)):
        x = float(np.nextafter(x, np.inf if k > 0 else -np.inf))
    return x


def pd_rows(kp, kd, u_max, zero_box=False):
    """[(name, angle error as (kind, value), rate)]: what one actuator's joint sees.  kind "err": q = q_nom + value needs no exactness;
    "abs": q = value."""
    if zero_box:     # u = -(kp 0) - kd v = -0.0 - kd v: +0.0 needs kd v = -0.0
        return [("u=+0", ("err", 0.0), -0.0), ("u=-0", ("err", 0.0), 0.0), ("u=5", ("err", 0.0), _rate_for(5.0, kd)), ("u=-5", ("err", 0.0), _rate_for(-5.0, kd))]
    up, dn = float(np.nextafter(u_max, np.inf)), float(np.nextafter(u_max, 0.0))
    rows = [(nm, ("err", 0.0), _rate_for(u, kd)) for nm, u in (("u=+max", u_max), ("u=-max", -u_max), ("u=+max+ulp", up), ("u=+max-ulp", dn),
                                                              ("u=-max-ulp", -up), ("u=-max+ulp", -dn))]
    rows += [("kp*qe=+inf", ("abs", 1e308), 0.5), ("kp*qe=-inf", ("abs", -1e308), 0.5), ("q=+inf", ("abs", np.inf), -0.25), ("q=-inf", ("abs", -np.inf), 1.0),
             ("inf-inf", ("abs", 1e308), -np.inf), ("-inf+inf", ("abs", -np.inf), np.inf), ("v=+inf", ("err", 0.1), np.inf),
             ("nan q", ("abs", np.nan), 0.3), ("nan v", ("err", -0.2), np.nan), ("nan both", ("abs", np.nan), np.nan),
             ("inside", ("err", 0.3), 1.7), ("inside-", ("err", -0.41), -2.9), ("clipped", ("err", -9.0), -3.0), ("zero", ("err", 0.0), 0.0)]
    return rows


def pd_batch(n, gains, order, act):
    """q [19, n], v [18, n] in the plant's numbering: actuator k of robot i sees row (i + k) mod len(rows) of pd_rows, so that every row
    visits every actuator; the seven base rows of q and the six of v hold NaN on every third robot (they must not matter).
    -> (q, v, names [12, n])"""
    g = PD_GAINS[gains]
    rows = pd_rows(g["kp"], g["kd"], g["u_max"], zero_box=(gains == "zero_box"))
    qn = _DEFAULT_NOM if g["q_nom"] is None else g["q_nom"]
    rng = np.random.default_rng(n)
    q, v = rng.normal(size=(19, n)), rng.normal(size=(18, n))
    q[:7, ::3] = np.nan
    v[:6, ::3] = np.nan
    which = np.zeros((12, n), np.int64)
    for k in range(12):
        j = order[act[k]]
        for i in range(n):
            nm, (kind, x), rate = rows[(i + k) % len(rows)]
            q[7 + j, i] = qn[7 + j] + x if kind == "err" else x
            v[6 + j, i] = rate
            which[k, i] = (i + k) % len(rows)
    return q, v, which, [r[0] for r in rows]


def pd_oracle(q, v, gains, order, act):
    g = PD_GAINS[gains]
    with np.errstate(invalid="ignore", over="ignore"):
        return to.pd_control_law(q, v, q_nom=g["q_nom"], order=order, act_joint=act, kp=g["kp"], kd=g["kd"], u_max=g["u_max"])


# ---- integrate
INTEGRATE_KINDS = ("ordinary", "zero_rate", "tiny_rate", "large_angle", "nonunit_quat")


def integrate_batch(n, dt, seed=0):
    """q, v, vd and kind [n] (index into INTEGRATE_KINDS, robot i: i mod 5).  The angular rate after the velocity update is: exactly zero;
    1e-170 in norm (w.w underflows: the identity rotation); |w| dt / 2 near 1e3 (dt = 0: |w| = 4e5 all the same); the quaternion of the
    last kind is 3.7 times a unit one."""
    from quadruped_drake_amd import workloads
    rng = np.random.default_rng(100 + seed)
    b = workloads.make_batch(3, n=max(n, 8), seed=seed)
    q, v = b["q"][:, :n].copy(), b["v"][:, :n].copy()
    vd = rng.normal(0.0, 5.0, (18, n))
    kind = np.arange(n) % len(INTEGRATE_KINDS)
    d = rng.normal(size=(3, n))
    d /= np.linalg.norm(d, axis=0)
    z, t, l = kind == 1, kind == 2, kind == 3
    v[0:3, z] = 0.0; vd[0:3, z] = 0.0
    v[0:3, t] = 1e-170 * d[:, t]; vd[0:3, t] = 0.0
    v[0:3, l] = (2e3 / (dt if dt > 0 else 5e-3)) * d[:, l] * rng.uniform(0.9, 1.1, l.sum())
    q[0:4, kind == 4] *= 3.7
    return q, v, vd, kind


def integrate_ld(q, v, vd, dt):
    """traj_oracle.integrate restated in np.longdouble (inputs are the same doubles) -> (q+, v+) as longdouble"""
    L = np.longdouble
    q = np.array(q, L); dt = L(dt)
    v = np.array(v, L) + dt * np.asarray(vd, L)
    w = v[0:3]
    wn = np.sqrt((w * w).sum(0))
    ang = L(0.5) * wn * dt
    sc = np.where(wn > 0, np.sin(ang) / np.where(wn > 0, wn, L(1)), L(0))
    dw = np.where(wn > 0, np.cos(ang), L(1)); dx, dy, dz = sc * w[0], sc * w[1], sc * w[2]
    w1, x1, y1, z1 = q[0].copy(), q[1].copy(), q[2].copy(), q[3].copy()
    qq = np.stack([dw * w1 - dx * x1 - dy * y1 - dz * z1, dw * x1 + dx * w1 + dy * z1 - dz * y1,
                   dw * y1 - dx * z1 + dy * w1 + dz * x1, dw * z1 + dx * y1 - dy * x1 + dz * w1])
    q[0:4] = qq / np.sqrt((qq * qq).sum(0))
    q[4:7] += dt * v[3:6]
    q[7:] += dt * v[6:]
    return q, v
