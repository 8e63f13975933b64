"""The gait planner's terrain law restated in numpy from the sentences at the head of include/wbc_gait_terrain.h (tests
only; shares no code with csrc/wbc_gait.hpp and knows nothing of its packed tables).  What that header takes from wbc_gait.h -- the
clock, the runs, theta, the body's arc -- is gait_oracle.py's restatement of it.  Every function takes `dtype`: np.float64, or
np.longdouble for the extended-precision answer the CPU tests measure their bars with."""
import numpy as np

import gait_oracle as go

LIFT, FIT = 0, 1
DEFAULTS = dict(body="fit", max_grade=0.5, edge_margin=0.03, apex_max=0.25)


def tparams(**kw):
    """dict(body, max_grade, edge_margin, apex_max): GaitPlanner.set_terrain's defaults, overridden by kw"""
    bad = set(kw) - set(DEFAULTS)
    assert not bad, bad
    return dict(DEFAULTS, **kw)


def knots(profile, dtype):
    return np.array(profile.s, dtype), np.array(profile.h, dtype)


def coordinate(profile, x, y, dtype=np.float64):
    """s of the world points (x, y) along the profile"""
    yaw = dtype(profile.yaw)
    return (x - dtype(profile.x0)) * np.cos(yaw) + (y - dtype(profile.y0)) * np.sin(yaw)


def height(profile, scale, s, dtype=np.float64):
    """scale h(s): half-open pieces [s_k, s_k+1), constant before the first and from the last knot on"""
    sk, hk = knots(profile, dtype)
    s = np.asarray(s, dtype)
    j = np.searchsorted(sk, s, side="right")                       # knots at or below s
    h = np.where(j == 0, hk[0], hk[np.clip(j - 1, 0, sk.size - 1)])
    if sk.size > 1:
        a = np.clip(j - 1, 0, sk.size - 2)
        inside = (j > 0) & (j < sk.size)
        h = h + np.where(inside, (hk[a + 1] - hk[a]) / (sk[a + 1] - sk[a]) * (s - sk[a]), dtype(0))
    return scale * h


def forbidden(profile, scale, max_grade, edge_margin, dtype=np.float64):
    """[(steep [n], lower, upper)] per piece: whether it is steep at each instance's scale, and its open interval with the margin"""
    sk, hk = knots(profile, dtype)
    out = []
    for j in range(sk.size - 1):
        slope = (hk[j + 1] - hk[j]) / (sk[j + 1] - sk[j])
        out.append((np.abs(scale * slope) > dtype(max_grade), sk[j] - dtype(edge_margin), sk[j + 1] + dtype(edge_margin)))
    return out


def place(profile, scale, tp, F, fixed, dtype=np.float64):
    """The flat law's footholds F [2, n] put on the terrain -> (F' [2, n], s [n], z [n], near [n]); fixed [n]: start-pose footholds,
    which are not moved.  near: how close the foothold came to a decision -- its s to a knot, to an end of a forbidden interval that
    was still in question, or to the tie between the two ends."""
    yaw = dtype(profile.yaw)
    d = np.array([np.cos(yaw), np.sin(yaw)])
    sF = coordinate(profile, F[0], F[1], dtype)
    sk, _ = knots(profile, dtype)
    near = np.min(np.abs(sF[None, :] - sk[:, None]), axis=0)
    e = sF.copy()
    found = fixed.copy()
    for steep, lo, hi in forbidden(profile, scale, tp["max_grade"], tp["edge_margin"], dtype):
        open_question = steep & ~found
        hit = open_question & (sF > lo) & (sF < hi)
        upper = (hi - sF) <= (sF - lo)
        near = np.where(open_question, np.minimum(near, np.minimum(np.abs(sF - lo), np.abs(sF - hi))), near)
        near = np.where(hit, np.minimum(near, np.abs((hi - sF) - (sF - lo))), near)
        e = np.where(hit, np.where(upper, hi, lo), e)
        found = found | hit
    moved = F + (e - sF) * d[:, None]
    return moved, e, height(profile, scale, e, dtype), near


def apex(profile, scale, tp, swing_height, sA, zA, sB, zB, dtype=np.float64):
    sk, hk = knots(profile, dtype)
    lo, hi = np.minimum(sA, sB), np.maximum(sA, sB)
    m = np.zeros(sA.shape, dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in range(sk.size):
            between = (sk[k] > lo) & (sk[k] < hi)
            lam = (sk[k] - sA) / np.where(between, sB - sA, dtype(1))
            ek = scale * hk[k] - (zA + lam * (zB - zA))
            m = np.where(between, np.maximum(m, ek / np.where(between, 4 * lam * (1 - lam), dtype(1))), m)
    return np.minimum(dtype(tp["apex_max"]), dtype(swing_height) + m)


def targets(params, strides, tp, profiles, time, cmd, gait_id=None, stride_scale=None, start=None, terrain_id=None, terrain_scale=None,
            dtype=np.float64, info=None):
    """-> (targets [54, n], mask [n]).  params, strides and the per-instance arrays: gait_oracle.targets; tp: tparams(); profiles: a
    list of terrain.Profile; terrain_id [n], terrain_scale [n].  info (a dict, optional) <- near [n]: the closest any foothold in use
    came to a decision; fixed [4, n]: whether the foothold of the run each foot is in (a stance run's own, a swing's B) is a start-pose
    one; s [2, 4, n], z [2, 4, n]: the footholds A and B of each foot along the profile (a stance run's own, twice); apex [4, n]."""
    time = np.asarray(time, np.float64)
    n = time.shape[0]
    cmd = np.asarray(cmd, np.float64)
    gid = np.zeros(n, int) if gait_id is None else np.asarray(gait_id).astype(int)
    sc = np.ones(n) if stride_scale is None else np.asarray(stride_scale, np.float64)
    st0 = np.zeros((3, n)) if start is None else np.asarray(start, np.float64)
    tid = np.zeros(n, int) if terrain_id is None else np.asarray(terrain_id).astype(int)
    tsc = np.ones(n) if terrain_scale is None else np.asarray(terrain_scale, np.float64)
    with np.errstate(invalid="ignore"):
        bad = (gid >= len(strides)) | ~(sc > 0) | ~np.isfinite(sc) | ~np.isfinite(time) | ~np.isfinite(cmd).all(0) | ~np.isfinite(st0).all(0)
        bad |= (tid >= len(profiles)) | ~np.isfinite(tsc)
    out = np.full((54, n), np.nan, dtype)
    mask = np.full(n, 0xF, np.uint8)
    near_all = np.full(n, np.inf, dtype)
    fixed_all = np.zeros((4, n), bool)
    s_all, z_all, apex_all = np.full((2, 4, n), np.nan, dtype), np.full((2, 4, n), np.nan, dtype), np.full((4, n), np.nan, dtype)
    stance = np.asarray(params["stance"], np.float64).astype(dtype)
    Hb, hs, ramp, wait = (params[k] for k in ("height", "swing_height", "ramp_time", "wait_time"))
    xt, yt = stance[:, 0] - stance[:, 0].mean(), stance[:, 1] - stance[:, 1].mean()
    fit = tp["body"] in ("fit", FIT)
    for g, (durations, masks) in enumerate(strides):
        for pi, prof in enumerate(profiles):
            sel = np.nonzero(~bad & (gid == g) & (tid == pi))[0]
            sel = sel[~go.unresolved(durations, masks, time[sel] - np.float64(wait), sc[sel])]      # wbc_gait.h's unresolved clock
            if sel.size == 0:
                continue
            m_ = sel.size
            t = time[sel].astype(dtype)
            c, w, s, st = cmd[:2, sel].astype(dtype), cmd[2, sel].astype(dtype), sc[sel].astype(dtype), st0[:, sel].astype(dtype)
            scale = tsc[sel].astype(dtype)
            tau = t - dtype(wait)
            pre = tau < 0
            tc = np.where(pre, dtype(0), tau)
            B = go.boundaries(durations)
            k, kT, r, phase = go.clock(durations, tc, s, dtype)
            at = lambda i: kT + s * dtype(go.boundary(B, i))
            o = np.zeros((54, m_), dtype)
            # ---- body, as on the plane
            th, thd, thdd = go.theta(ramp, tc, dtype)
            th, thd, thdd = (np.where(pre, dtype(0), x) for x in (th, thd, thdd))
            p, psi = go.pose(th, c, w, st, dtype)
            vel = go._rot(psi, c[0], c[1])
            o[0:2] = p
            o[3:5] = thd * vel
            o[6:8] = thdd * vel + thd**2 * w * np.stack([-vel[1], vel[0]])
            o[11] = psi; o[14] = w * thd; o[17] = w * thdd
            zero = np.zeros(m_, dtype)
            never = np.ones(m_, bool)

            def foothold(f, a, b):
                """of the stance run [a, b) of foot f, a None: the run without a beginning -> (xy, s, z, near, fixed)"""
                if a is None:
                    thm, fixed = zero, never
                else:
                    fixed = pre | (a <= 0)
                    thm = np.where(fixed, dtype(0), go.theta(ramp, np.maximum((a + b) / 2, dtype(0)), dtype)[0])
                pm, psim = go.pose(thm, c, w, st, dtype)
                F = pm + go._rot(psim, stance[f, 0], stance[f, 1])
                return place(prof, scale, tp, F, fixed, dtype) + (fixed,)

            known = {}

            def foothold_of(f, lo, hi):
                """foothold() of the stance run between boundaries lo and hi; a stride's phases share their runs: each is computed once"""
                if (f, lo, hi) not in known:
                    known[(f, lo, hi)] = foothold(f, None if lo is None else at(lo), None if lo is None else at(hi))
                return known[(f, lo, hi)]

            G = np.zeros((4, 3, m_), dtype)                  # the ground height under each foot and its two rates
            near = np.full(m_, np.inf, dtype)
            fixed_now = np.zeros((4, m_), bool)
            sAB, zAB, ap = np.zeros((2, 4, m_), dtype), np.zeros((2, 4, m_), dtype), np.zeros((4, m_), dtype)
            mk = np.zeros(m_, np.uint8)
            cases = [(j, ~pre & (phase == j), masks[j]) for j in range(len(durations))] + [(None, pre, 0xF)]
            for j, inj, mj in cases:
                mk[inj] = mj
                for f in range(4):
                    contact, lo, hi, plo, nhi = (1, None, None, None, None) if j is None else go.runs(masks, f, j)
                    val = np.zeros((9, m_), dtype)
                    gf = np.zeros((3, m_), dtype)
                    if contact:
                        F, sF, zF, nr, fx = foothold_of(f, lo, hi)
                        val[0:2] = F; val[2] = zF
                        gf[0] = zF
                        sa, sb, za, zb, a_ = sF, sF, zF, zF, zero + dtype(hs)
                    else:
                        a, b = at(lo), at(hi)
                        A, sa, za, n1, _ = foothold_of(f, plo, lo)
                        Bf, sb, zb, n2, fx = foothold_of(f, hi, nhi)
                        nr = np.minimum(n1, n2)
                        D = b - a
                        u = (tau - a) / D
                        sg = 10 * u**3 - 15 * u**4 + 6 * u**5
                        sgd = 30 * u**2 - 60 * u**3 + 30 * u**4                 # sigma' D and sigma'' D^2: divided last, as wbc_gait.h's rows are
                        sgdd = 60 * u - 180 * u**2 + 120 * u**3
                        a_ = apex(prof, scale, tp, hs, sa, za, sb, zb, dtype)
                        bu = a_ * 64 * u**3 * (1 - u)**3                     # the apex times b(u) and its rates, in wbc_gait.h's order
                        bud = a_ * 64 * (3 * u**2 * (1 - u)**3 - 3 * u**3 * (1 - u)**2) / D
                        budd = a_ * 64 * (6 * u * (1 - u)**3 - 18 * u**2 * (1 - u)**2 + 6 * u**3 * (1 - u)) / D**2
                        gf[0], gf[1], gf[2] = za + (zb - za) * sg, (zb - za) * sgd / D, (zb - za) * sgdd / D**2
                        val[0:2] = A + (Bf - A) * sg
                        val[3:5] = (Bf - A) * sgd / D
                        val[6:8] = (Bf - A) * sgdd / D**2
                        val[2], val[5], val[8] = gf[0] + bu, gf[1] + bud, gf[2] + budd
                    rows = slice(18 + 9 * f, 27 + 9 * f)
                    o[rows, :] = np.where(inj, val, o[rows, :])
                    G[f] = np.where(inj, gf, G[f])
                    near = np.where(inj, np.minimum(near, nr), near)
                    fixed_now[f] = np.where(inj, fx, fixed_now[f])
                    sAB[0, f], sAB[1, f] = np.where(inj, sa, sAB[0, f]), np.where(inj, sb, sAB[1, f])
                    zAB[0, f], zAB[1, f] = np.where(inj, za, zAB[0, f]), np.where(inj, zb, zAB[1, f])
                    ap[f] = np.where(inj, a_, ap[f])
            # ---- the body follows the feet
            pairs = lambda a: (a[0] + a[1]) + (a[2] + a[3])          # the header's order of every sum over the feet
            mean = pairs(G) / 4
            o[2], o[5], o[8] = dtype(Hb) + mean[0], mean[1], mean[2]
            if fit:
                for row, lever, sign in ((10, xt, -1), (9, yt, +1)):
                    P, Pd, Pdd = (pairs(lever[:, None] * G[:, d_]) / pairs(lever**2) for d_ in range(3))
                    o[row] = sign * np.arctan(P)
                    o[row + 3] = sign * Pd / (1 + P**2)
                    o[row + 6] = sign * (Pdd * (1 + P**2) - 2 * P * Pd**2) / (1 + P**2)**2
            out[:, sel] = o
            mask[sel] = mk
            near_all[sel], fixed_all[:, sel] = near, fixed_now
            s_all[:, :, sel], z_all[:, :, sel], apex_all[:, sel] = sAB, zAB, ap
    if info is not None:
        info.update(near=near_all, fixed=fixed_all, s=s_all, z=z_all, apex=apex_all)
    return out, mask
