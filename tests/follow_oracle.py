"""Plain numpy restatement of the follow law (include/wbc_ground.h, "Following the ground") -- test infrastructure.

Written from the header's sentences, one instance at a time, with numpy's own rotations and means.  The terrain is read through
quadruped_drake_amd.terrain.evaluate (height and normal by the header's definition), not through the packed table of
csrc/wbc_ground.hpp, and nothing of csrc/ is shared."""
import math

import numpy as np

from quadruped_drake_amd import terrain as tr

OFF, LIFT, FIT = 0, 1, 2
ZROWS = [2, 5, 8] + [18 + 9 * c + 3 * d + 2 for c in range(4) for d in range(3)]     # the 15 z rows of LIFT
ATTITUDE = list(range(9, 18))


def surface(profile, scale, x, y):
    """-> (s, H, g) under the world point (x, y): g is read off the normal, n = (-g cos psi, -g sin psi, 1) / sqrt(1 + g^2)."""
    c, sn = math.cos(profile.yaw), math.sin(profile.yaw)
    s = (x - profile.x0) * c + (y - profile.y0) * sn
    H, n = tr.evaluate(profile, x, y, scale)
    n = np.asarray(n, float)
    g = -(n[0] * c + n[1] * sn) / n[2]
    return s, float(H), float(g)


def _rot(axis, angle):
    axis = np.asarray(axis, float)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * K @ K


def rpy_matrix(rpy):
    return _rot([0, 0, 1], rpy[2]) @ _rot([0, 1, 0], rpy[1]) @ _rot([1, 0, 0], rpy[0])


def rpy_from_matrix(R):
    return np.array([math.atan2(R[2, 1], R[2, 2]), math.atan2(-R[2, 0], math.hypot(R[0, 0], R[1, 0])), math.atan2(R[1, 0], R[0, 0])])


def rate_matrix(rpy):
    """E: rates of (roll, pitch, yaw) -> angular velocity in the world."""
    sp, cp, sy, cy = math.sin(rpy[1]), math.cos(rpy[1]), math.sin(rpy[2]), math.cos(rpy[2])
    return np.array([[cp * cy, -sy, 0.0], [cp * sy, cy, 0.0], [-sp, 0.0, 1.0]])


def fit(profile, scale, t):
    """-> (usable feet, s_m, H_m, b) of one instance's 54 rows."""
    usable = [c for c in range(4) if np.isfinite(t[18 + 9 * c]) and np.isfinite(t[18 + 9 * c + 1])]
    if not usable:
        s, H, _ = surface(profile, scale, t[0], t[1])
        return usable, s, H, 0.0
    sH = np.array([surface(profile, scale, t[18 + 9 * c], t[18 + 9 * c + 1])[:2] for c in usable])
    sm, Hm = sH.mean(0)
    den = float(((sH[:, 0] - sm) ** 2).sum())
    b = 0.0 if len(usable) < 2 or den < 1e-12 else float(((sH[:, 0] - sm) * (sH[:, 1] - Hm)).sum()) / den
    return usable, sm, Hm, b


def follow_one(profile, scale, t, mode):
    """One instance's 54 rows -> the followed rows (a copy)."""
    t = np.array(t, float)
    if mode == OFF or profile is None or not np.isfinite(scale):
        return t
    out = t.copy()
    c, sn = math.cos(profile.yaw), math.sin(profile.yaw)
    along = lambda u: u[0] * c + u[1] * sn
    usable, sm, Hm, b = fit(profile, scale, t)
    for k in usable:
        r = 18 + 9 * k
        _, H, g = surface(profile, scale, t[r], t[r + 1])
        out[r + 2] = t[r + 2] + H
        out[r + 5] = t[r + 5] + g * along(t[r + 3:r + 5])
        out[r + 8] = t[r + 8] + g * along(t[r + 6:r + 8])
    sb = surface(profile, scale, t[0], t[1])[0]
    out[2] = t[2] + (Hm + b * (sb - sm))
    out[5] = t[5] + b * along(t[3:5])
    out[8] = t[8] + b * along(t[6:8])
    if mode == FIT and b != 0.0:
        Rf = _rot([-sn, c, 0.0], -math.atan(b))
        rpy = rpy_from_matrix(Rf @ rpy_matrix(t[9:12]))
        if abs(math.cos(rpy[1])) >= 1e-9:
            M = np.linalg.solve(rate_matrix(rpy), Rf @ rate_matrix(t[9:12]))
            out[9:12], out[12:15], out[15:18] = rpy, M @ t[12:15], M @ t[15:18]
    return out


def pitch_after_fit(profile, scale, t):
    """pitch' of one instance under FIT (its own pitch where the attitude stands)."""
    return float(follow_one(profile, scale, t, FIT)[10])


# ---- test states
KNOTTED = dict(s=[-0.25, 0.0, 0.125, 0.5], h=[0.0, 0.05, 0.02, 0.1])   # yaw = 0, origin 0: s(x, y) is x, bit for bit
SCALES = (1.0, 0.0, -0.7, 2.5)
REACH = 0.4                            # [m] of s about a profile's origin within which draw() plants feet (test_terrain_cpu._segments)


def sixteen_profiles():
    """terrain_oracle.four_profiles() and twelve more: KNOTTED, a ridge, a full table of eight knots, a single raised knot,
    slopes down and across, and rotated copies -- every direction, origin and knot count."""
    import terrain_oracle as to
    p = to.four_profiles()
    p += [tr.Profile(KNOTTED["s"], KNOTTED["h"]), tr.ridge(-0.15, 0.3, 0.1, 0.12, yaw=1.0, x0=0.02),
          tr.Profile(np.linspace(-0.35, 0.35, 8), [0.0, 0.03, 0.01, 0.06, 0.06, 0.02, 0.08, 0.05], yaw=-2.4, y0=-0.03),
          tr.flat(-0.11, yaw=0.3), tr.slope(math.atan(-0.3), start=-0.2, yaw=math.pi / 2), tr.slope(0.25, start=-3.0, yaw=3.0, x0=0.1)]
    p += [q.rotated(a) for q, a in zip(p[1:7], (0.7, -1.9, 2.6, 1.3, -0.4, 3.1))]
    assert len(p) == 16
    return p


def pieces(profile):
    """The pieces of a profile as (index, lower edge, upper edge) with index -1 the level ground before the knots, nk - 1 the level
    ground after them (tests/test_terrain_cpu._segments)."""
    edges = [-math.inf] + list(profile.s) + [math.inf]
    return [(j - 1, edges[j], edges[j + 1]) for j in range(len(edges) - 1)]


def piece_of(profile, x, y):
    s = (x - profile.x0) * math.cos(profile.yaw) + (y - profile.y0) * math.sin(profile.yaw)
    return int(np.searchsorted(np.array(profile.s), s, side="right")) - 1


def draw(n, seed, profiles=None):
    """-> (profiles, terrain_id [n], terrain_scale [n], targets [54, n]).  Instance i stands on profile i mod 16 (4 without the
    twelve) at one of SCALES in turn (then random in [-1, 2.5]); its four footholds lie on four consecutive pieces of its profile,
    the first piece moving on with i, within 0.45 m of the profile's origin, so that a batch of 9 x 16 instances puts a foot on
    every piece of every profile; every other row is random, roll and pitch within 0.6.  Instances 4 (profile KNOTTED) has its
    footholds exactly ON knots.  A scale whose FIT would pitch the trunk beyond 1.2 is halved until it does not."""
    profiles = sixteen_profiles() if profiles is None else profiles
    rng = np.random.default_rng(seed)
    tid = (np.arange(n) % len(profiles)).astype(np.uint8)
    tsc = np.array([SCALES[(i // len(profiles) + i) % 4] if i < 8 * len(profiles) else rng.uniform(-1.0, 2.5) for i in range(n)])
    t = rng.uniform(-0.5, 0.5, (54, n))
    t[9:11] = rng.uniform(-0.6, 0.6, (2, n))
    t[11] = rng.uniform(-math.pi, math.pi, n)
    for i in range(n):
        p = profiles[tid[i]]
        pc = [x for x in pieces(p) if x[1] < REACH and x[2] > -REACH]
        c, sn = math.cos(p.yaw), math.sin(p.yaw)
        for f in range(4):
            _, lo, hi = pc[(i // len(profiles) + f) % len(pc)]
            lo, hi = max(lo, -REACH - 0.05), min(hi, REACH + 0.05)
            s = rng.uniform(lo + 0.05 * (hi - lo), hi - 0.05 * (hi - lo))
            w = rng.uniform(-0.3, 0.3)
            t[18 + 9 * f, i] = p.x0 + s * c - w * sn
            t[18 + 9 * f + 1, i] = p.y0 + s * sn + w * c
        t[0:2, i] = t[18:54:9, i].mean(), t[19:54:9, i].mean()
        t[0:2, i] += rng.uniform(-0.05, 0.05, 2)
    if n > 4 and len(profiles) == 16:
        t[18:54:9, 4] = [-0.25, 0.0, 0.125, 0.5]          # exactly on KNOTTED's four knots
    for i in range(n):
        for _ in range(8):
            if abs(pitch_after_fit(profiles[tid[i]], tsc[i], t[:, i])) <= 1.2:
                break
            tsc[i] *= 0.5
    return profiles, tid, tsc, t


def slope_start(model, grade=0.2, scales=(1.0, 0.5, 0.0, -1.0), depth=1e-3):
    """-> (table, q [19, n], v [18, n], profile, terrain_scale [n]): one robot per scale in the reference's stance, each square on
    its own slope of grade `grade` x scale rising along +x (the attitude of terrain.stance_pose), its trunk origin over the world's
    origin, where the standing targets want it, and its lowest foot `depth` into the slope (terrain_oracle.slope_stance, per scale)."""
    import ground_oracle as go
    import terrain_oracle as to
    prof = tr.slope(math.atan(grade), start=-5.0, length=10.0)
    t, q, v = go.drop_state(model, n=len(scales))
    for i, sc in enumerate(scales):
        q[0:4, i] = tr.stance_pose(prof, 0.0, 0.0, 0.0, sc)[0]
        q[4:7, i] = 0.0
        q[6, i] -= to._clearance(t, q[:, i], prof, sc).min() + depth
    return t, q, v, prof, np.array(scales, float)


def trunk_height_and_pitch(q, profile, scales):
    """Per instance: height of the trunk origin above the ground under it, and the pitch of Rz Ry Rx read from the quaternion."""
    w, x, y, z = q[0:4] / np.linalg.norm(q[0:4], axis=0)
    H = np.array([float(tr.evaluate(profile, q[4, i], q[5, i], scales[i])[0]) for i in range(q.shape[1])])
    return q[6] - H, np.arcsin(2.0 * (w * y - z * x))


def follow(profiles, terrain_id, terrain_scale, targets, mode, n=None):
    """SoA targets [54, ld] -> the followed copy; instances n .. ld are padding and stay."""
    out = np.array(targets, float)
    n = out.shape[1] if n is None else n
    for i in range(n):
        k = 0 if terrain_id is None else int(terrain_id[i])
        sc = 1.0 if terrain_scale is None else float(terrain_scale[i])
        with np.errstate(all="ignore"):
            out[:, i] = follow_one(profiles[k] if k < len(profiles) else None, sc, out[:, i], mode)
    return out
