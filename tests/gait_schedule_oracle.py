"""The gait planner's command schedules restated in numpy from the sentences at the head of
include/wbc_gait_schedule.h (tests only; shares no code with csrc/wbc_gait.hpp and knows nothing of its buffer of
resolved switches).  That header changes one thing, the body's pose function P(theta); what it leaves as it is -- the clock, the
runs, the swings, the terrain law -- is gait_oracle.py's and gait_terrain_oracle.py's restatement, evaluated with their `pose`
replaced by P.  Every function takes `dtype`: np.float64, or np.longdouble for the extended-precision answer the tests measure their
bars with."""
import contextlib

import numpy as np

import gait_oracle as go
import gait_terrain_oracle as gto

MAX_SWITCHES = 7
_arc = go.pose                                   # the arc of one command from one start: wbc_gait.h's body pose
BODY_ROWS = [0, 1, 3, 4, 6, 7, 11, 14, 17]      # what the chain rule on P gives; the other body rows are the flat or the terrain law's


def valid(nswitch, when, cmds, blend):
    """[n] bool: every number finite, Theta_1 >= 0, Theta_j+1 >= Theta_j + beta, m <= 7 (rows from m on are not looked at)"""
    m = np.asarray(nswitch).astype(int)
    ok = m <= MAX_SWITCHES
    least = np.zeros(m.shape)
    with np.errstate(invalid="ignore"):
        for j in range(MAX_SWITCHES):
            used = j < m
            fin = np.isfinite(when[j]) & np.isfinite(cmds[3 * j:3 * j + 3]).all(0)
            ok &= ~used | (fin & (when[j] >= least))
            least = np.where(used, when[j] + blend, least)
    return ok


def _quintic(q0, V0, A0, q1, V1, A1, u):
    """q, dq/du, d2q/du2 of the quintic through value, V and A at u = 0 and u = 1"""
    D, DV, DA = q1 - q0 - V0 - A0 / 2, V1 - V0 - A0, A1 - A0
    k3, k4, k5 = 10 * D - 4 * DV + DA / 2, -15 * D + 7 * DV - DA, 6 * D - 3 * DV + DA / 2
    return (q0 + V0 * u + A0 * u**2 / 2 + k3 * u**3 + k4 * u**4 + k5 * u**5,
            V0 + A0 * u + 3 * k3 * u**2 + 4 * k4 * u**3 + 5 * k5 * u**4,
            A0 + 6 * k3 * u + 12 * k4 * u**2 + 20 * k5 * u**3)


class Schedule:
    """The schedules of n valid instances: cmd [3, n] = c_0, start [3, n] = S_0, nswitch [n], when [7, n], cmds [21, n], blend."""

    def __init__(self, cmd, start, nswitch, when, cmds, blend, dtype=np.float64):
        self.dtype = dtype
        self.c0 = np.asarray(cmd, np.float64).astype(dtype)
        self.s0 = np.asarray(start, np.float64).astype(dtype)
        self.m = np.asarray(nswitch).astype(int)
        self.when = np.asarray(when, np.float64).astype(dtype)
        self.cmds = np.asarray(cmds, np.float64).astype(dtype)
        self.beta = dtype(blend)
        self.near = np.full(self.m.shape, np.inf)           # the closest any evaluation came to a Theta_j or to a window's end

    def pose(self, th):
        """P(th) -> (p [2, n], psi [n], P' [3, n], P'' [3, n]), the derivatives in theta"""
        dt, beta = self.dtype, self.beta
        th = np.asarray(th, dt)
        cx, cy, w = self.c0[0].copy(), self.c0[1].copy(), self.c0[2].copy()           # the segment before the switch: its command,
        sx, sy, sp = self.s0[0].copy(), self.s0[1].copy(), self.s0[2].copy()           # its start
        org = np.zeros(th.shape, dt)                                                    # and the theta its arc starts at
        p, psi = _arc(th, np.stack([cx, cy]), w, np.stack([sx, sy, sp]), dt)
        v = go._rot(psi, cx, cy)
        d1 = np.stack([v[0], v[1], w + 0 * th])
        d2 = np.stack([-w * v[1], w * v[0], 0 * th])
        x, y = p[0], p[1]
        for j in range(MAX_SWITCHES):
            used = j < self.m
            if not used.any():                                                           # no instance has a switch j: nothing below selects
                break
            Th = np.where(used, self.when[j], dt(0))
            cj = [np.where(used, self.cmds[3 * j + d], dt(0)) for d in range(3)]
            pE, psiE = _arc(Th - org, np.stack([cx, cy]), w, np.stack([sx, sy, sp]), dt)
            psiS = psiE + beta * (w + cj[2]) / 2
            vE, vS = go._rot(psiE, cx, cy), go._rot(psiS, cj[0], cj[1])
            pS = pE + (beta / 2) * (vE + vS)
            with np.errstate(invalid="ignore"):
                gap = np.minimum(np.abs(th - Th), np.abs(th - (Th + beta)))
            self.near = np.where(used, np.minimum(self.near, gap.astype(np.float64)), self.near)
            blend = used & (th >= Th) & (th < Th + beta)
            arc = used & (th >= Th + beta)
            # the arc of c_j from S_j
            pa, psia = _arc(np.where(arc, th - Th - beta, dt(0)), np.stack(cj[:2]), cj[2], np.stack([pS[0], pS[1], psiS]), dt)
            va = go._rot(psia, cj[0], cj[1])
            # the blend: value, V = beta q', A = beta^2 q'' at both ends
            u = np.where(blend, (th - Th) / np.where(beta > 0, beta, dt(1)), dt(0))
            qx = _quintic(pE[0], beta * vE[0], beta**2 * (-w * vE[1]), pS[0], beta * vS[0], beta**2 * (-cj[2] * vS[1]), u)
            qy = _quintic(pE[1], beta * vE[1], beta**2 * (w * vE[0]), pS[1], beta * vS[1], beta**2 * (cj[2] * vS[0]), u)
            qp = _quintic(psiE, beta * w, dt(0), psiS, beta * cj[2], dt(0), u)
            b1, b2 = (beta if beta > 0 else dt(1)), (beta**2 if beta > 0 else dt(1))
            x = np.where(blend, qx[0], np.where(arc, pa[0], x))
            y = np.where(blend, qy[0], np.where(arc, pa[1], y))
            psi = np.where(blend, qp[0], np.where(arc, psia, psi))
            d1 = np.where(blend, np.stack([qx[1], qy[1], qp[1]]) / b1, np.where(arc, np.stack([va[0], va[1], cj[2]]), d1))
            d2 = np.where(blend, np.stack([qx[2], qy[2], qp[2]]) / b2, np.where(arc, np.stack([-cj[2] * va[1], cj[2] * va[0], 0 * th]), d2))
            cx, cy, w = (np.where(used, a, b) for a, b in zip(cj, (cx, cy, w)))
            sx, sy, sp = (np.where(used, a, b) for a, b in zip((pS[0], pS[1], psiS), (sx, sy, sp)))
            org = np.where(used, Th + beta, org)
        return np.stack([x, y]), psi, d1, d2


@contextlib.contextmanager
def _pose_is(schedule):
    """gait_oracle.pose <- P of `schedule`, for the instances the schedule holds, in their order"""
    old = go.pose

    def pose(th, c, w, start, dtype=np.float64):
        assert dtype is schedule.dtype and np.shape(th) == schedule.m.shape
        p, psi, _, _ = schedule.pose(th)
        return p, psi

    go.pose = pose
    try:
        yield
    finally:
        go.pose = old


def targets(params, strides, time, cmd, nswitch, when, cmds, blend, gait_id=None, stride_scale=None, start=None, tp=None, profiles=None,
            terrain_id=None, terrain_scale=None, dtype=np.float64, info=None):
    """-> (targets [54, n], mask [n]).  params, strides and the per-instance arrays: gait_oracle.targets; nswitch [n], when [7, n],
    cmds [21, n], blend: wbc_gait_set_schedule's; profiles (a list of terrain.Profile, None: the plane), tp, terrain_id,
    terrain_scale: gait_terrain_oracle.targets'.  info (a dict, optional) <- near [n]: the closest a pose evaluation of the instance
    -- of its body, or of a foothold of any of its stride's runs, in use at this time or not -- came to a Theta_j or to the end of a
    blend window, in path-parameter units; terrain_near [n]: gait_terrain_oracle.targets' `near` (inf on the plane)."""
    time = np.asarray(time, np.float64)
    n = time.shape[0]
    cmd = np.asarray(cmd, np.float64)
    gid = np.zeros(n, int) if gait_id is None else np.asarray(gait_id).astype(int)
    sc = np.ones(n) if stride_scale is None else np.asarray(stride_scale, np.float64)
    st0 = np.zeros((3, n)) if start is None else np.asarray(start, np.float64)
    tid = np.zeros(n, int) if terrain_id is None else np.asarray(terrain_id).astype(int)
    tsc = np.ones(n) if terrain_scale is None else np.asarray(terrain_scale, np.float64)
    when, cmds = np.asarray(when, np.float64), np.asarray(cmds, np.float64)
    with np.errstate(invalid="ignore"):
        bad = (gid >= len(strides)) | ~(sc > 0) | ~np.isfinite(sc) | ~np.isfinite(time) | ~np.isfinite(cmd).all(0) | ~np.isfinite(st0).all(0)
        if profiles is not None:
            bad |= (tid >= len(profiles)) | ~np.isfinite(tsc)
        bad |= ~valid(nswitch, when, cmds, blend)
    out = np.full((54, n), np.nan, dtype)
    mask = np.full(n, 0xF, np.uint8)
    near, tnear = np.full(n, np.inf), np.full(n, np.inf)
    ramp, wait = params["ramp_time"], params["wait_time"]
    for g in range(len(strides)):
        for pi in range(1 if profiles is None else len(profiles)):
            sel = np.nonzero(~bad & (gid == g) & ((tid == pi) | (profiles is None)))[0]
            sel = sel[~go.unresolved(strides[g][0], strides[g][1], time[sel] - np.float64(wait), sc[sel])]      # wbc_gait.h's unresolved clock
            if sel.size == 0:
                continue
            S = Schedule(cmd[:, sel], st0[:, sel], np.asarray(nswitch)[sel], when[:, sel], cmds[:, sel], blend, dtype)
            with _pose_is(S):
                if profiles is None:
                    o, mk = go.targets(params, [strides[g]], time[sel], cmd[:, sel], None, sc[sel], st0[:, sel], dtype=dtype)
                else:
                    ti = {}
                    o, mk = gto.targets(params, [strides[g]], tp, [profiles[pi]], time[sel], cmd[:, sel], None, sc[sel], st0[:, sel], None,
                                        tsc[sel], dtype=dtype, info=ti)
                    tnear[sel] = np.asarray(ti["near"], np.float64)
            # the body rows by the chain rule on P
            tau = time[sel].astype(dtype) - dtype(wait)
            pre = tau < 0
            th, thd, thdd = go.theta(ramp, np.where(pre, dtype(0), tau), dtype)
            th, thd, thdd = (np.where(pre, dtype(0), a) for a in (th, thd, thdd))
            p, psi, d1, d2 = S.pose(th)
            o[0:2] = p
            o[3:5] = thd * d1[0:2]
            o[6:8] = thdd * d1[0:2] + thd**2 * d2[0:2]
            o[11], o[14], o[17] = psi, thd * d1[2], thdd * d1[2] + thd**2 * d2[2]
            out[:, sel], mask[sel], near[sel] = o, mk, S.near
    if info is not None:
        info.update(near=near, terrain_near=tnear)
    return out, mask
