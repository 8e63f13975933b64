"""The gait planner's foot-placement feedback restated in numpy from the sentences at the head of
include/wbc_gait_feedback.h (tests only; shares no code with csrc/ and takes its clock from gait_oracle).  The state is
carried from call to call in a State; every function takes `dtype`: np.float64, or np.longdouble for the extended-precision answer
the CPU tests measure their bars with."""
import numpy as np

import gait_oracle as go

NEAR = 1e-9


def defaults(height):
    """wbc_gait_feedback_params_default"""
    return dict(k_v=float(np.sqrt(height / 9.81)), k_p=0.0, d_max=0.10, u_hold=0.5)


class State:
    """cur, frm, to [4, 2, n] (foot, x / y, instance) and the previous mask [n], as wbc_gait_set_feedback leaves them"""

    def __init__(self, n, dtype=np.float64):
        self.cur, self.frm, self.to = (np.zeros((4, 2, n), dtype) for _ in range(3))
        self.prev = np.full(n, 0xF, np.uint8)

    def copy(self):
        s = State.__new__(State)
        s.cur, s.frm, s.to, s.prev = self.cur.copy(), self.frm.copy(), self.to.copy(), self.prev.copy()
        return s

    def packed(self):
        """[6, 4 n] in the device's layout: rows cur_x, cur_y, from_x, from_y, to_x, to_y, foot f of instance i at 4 i + f"""
        n = self.prev.size
        return np.stack([a[:, k, :].T.reshape(4 * n) for a in (self.cur, self.frm, self.to) for k in range(2)])


def offset(par, q, v, tg, dtype=np.float64):
    """-> (d [2, n], |d_raw| [n]) from the measured q [19, n], v [18, n] and the targets' body rows"""
    kv, kp, dmax = dtype(par["k_v"]), dtype(par["k_p"]), dtype(par["d_max"])
    e_p = np.asarray(q[4:6], dtype) - tg[0:2]
    e_v = np.asarray(v[3:5], dtype) - tg[3:5]
    raw = kv * e_v + kp * e_p
    m = np.sqrt(raw[0] * raw[0] + raw[1] * raw[1])
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.minimum(dtype(1), dmax / m)
        d = np.where(m == 0, dtype(0), raw * g)
    return d, m


def step(par, params, strides, time, q, v, tg, mask, state, gait_id=None, stride_scale=None, dtype=np.float64):
    """One call of the pass on the targets tg [54, n] (dtype) and mask [n] that the gait's oracle wrote at time [n].  Advances `state`
    in place.  -> (rows [54, n], offsets [8, n], decisions [n, 9] ints: the clamp binding, per foot `to` taken, per foot the contact bit;
    near [n]: |u - u_hold| < NEAR on a foot in the air, or ||d_raw| - d_max| < NEAR; skipped [n])."""
    time = np.asarray(time, np.float64)
    n = time.size
    gid = np.zeros(n, int) if gait_id is None else np.asarray(gait_id).astype(int)
    sc = np.ones(n) if stride_scale is None else np.asarray(stride_scale, np.float64)
    tg = np.asarray(tg, dtype)
    out, offs = tg.copy(), np.full((8, n), np.nan, dtype)
    d, m = offset(par, q, v, tg, dtype)
    with np.errstate(invalid="ignore"):
        skipped = ~(np.isfinite(np.asarray(q[4:6], np.float64)).all(0) & np.isfinite(np.asarray(v[3:5], np.float64)).all(0) &
                    np.isfinite(tg.astype(np.float64)).all(0) & np.isfinite(time))
    decisions = np.zeros((n, 9), int)
    near = np.zeros(n, bool)
    with np.errstate(invalid="ignore"):
        decisions[:, 0] = m > dtype(par["d_max"])
        near |= np.abs(m - dtype(par["d_max"])) < NEAR
    mask = np.asarray(mask, np.uint8)
    uh = dtype(par["u_hold"])
    for g, (durations, masks) in enumerate(strides):
        sel = np.nonzero(~skipped & (gid == g))[0]
        if sel.size == 0:
            continue
        s = sc[sel].astype(dtype)
        tau = time[sel].astype(dtype) - dtype(params["wait_time"])
        B = go.boundaries(durations)
        k, kT, r, phase = go.clock(durations, np.where(tau < 0, dtype(0), tau), s, dtype)
        for f in range(4):
            down = ((mask[sel] >> f) & 1).astype(bool)
            was = ((state.prev[sel] >> f) & 1).astype(bool)
            D, u = np.full(sel.size, np.nan, dtype), np.full(sel.size, np.nan, dtype)
            for j in range(len(durations)):
                contact, lo, hi, _, _ = go.runs(masks, f, j)
                if lo is None:
                    continue
                a, b = kT + s * dtype(go.boundary(B, lo)), kT + s * dtype(go.boundary(B, hi))
                inj = phase == j
                D = np.where(inj, b - a, D)
                u = np.where(inj, (tau - a) / (b - a), u)
            with np.errstate(invalid="ignore"):
                take = ~down & (was | (u <= uh))
                near[sel] |= ~down & (np.abs(u - uh) < NEAR)
            lift, land = ~down & was, down & ~was
            cur, frm, to = state.cur[f][:, sel], state.frm[f][:, sel], state.to[f][:, sel]
            frm = np.where(lift, cur, frm)
            to = np.where(take, d[:, sel], to)
            cur = np.where(land, to, cur)
            sg = 10 * u**3 - 15 * u**4 + 6 * u**5
            sgd = 30 * u**2 * (1 - u)**2
            sgdd = 60 * u * (1 - u) * (1 - 2 * u)
            with np.errstate(invalid="ignore"):
                p = np.where(down, cur, frm + (to - frm) * sg)
                pd = np.where(down, dtype(0), (to - frm) * sgd / D)
                pdd = np.where(down, dtype(0), (to - frm) * sgdd / D**2)
            r0 = 18 + 9 * f
            out[r0:r0 + 2, sel] = tg[r0:r0 + 2, sel] + p
            out[r0 + 3:r0 + 5, sel] = tg[r0 + 3:r0 + 5, sel] + pd
            out[r0 + 6:r0 + 8, sel] = tg[r0 + 6:r0 + 8, sel] + pdd
            offs[2 * f:2 * f + 2, sel] = p
            state.cur[f][:, sel], state.frm[f][:, sel], state.to[f][:, sel] = cur, frm, to
            decisions[sel, 1 + f] = take
            decisions[sel, 5 + f] = down
        state.prev[sel] = mask[sel]
    return out, offs, decisions, near, skipped
