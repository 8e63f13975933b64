"""The gait planner's law restated in numpy from the sentences at the head of include/wbc_gait.h (tests only; shares no code with
csrc/wbc_gait.hpp and knows nothing of its packed table).  Every function takes `dtype`: np.float64, or np.longdouble for the
extended-precision answer the CPU tests measure their bars with.  The stride's boundaries B_j are summed in double in either case:
that is the law's definition, not a rounding of it."""
import numpy as np

SINC_SMALL = 1e-4


def boundaries(durations):
    """B_0 .. B_n in double, summed in the header's order"""
    B = [0.0]
    for d in durations:
        B.append(B[-1] + float(d))
    return B


def boundary(B, i):
    """the time of boundary i (any integer) relative to the stride's start: B_(i mod n) + floor(i / n) B_n, in double"""
    n = len(B) - 1
    return B[i % n] + float(i // n) * B[n]


def runs(masks, foot, j):
    """The run of `foot` around phase j of a stride with contact masks `masks`, as boundary indices: (contact, lo, hi, plo, nhi) --
    the run is [lo, hi); for a swing run the stance run before it is [plo, lo) and the one after it [hi, nhi).  A foot in contact in
    every phase: (1, None, None, None, None)."""
    n = len(masks)
    bit = lambda i: (masks[i % n] >> foot) & 1
    if all(bit(i) for i in range(n)):
        return 1, None, None, None, None
    lo = j
    while bit(lo - 1) == bit(j):
        lo -= 1
    hi = j + 1
    while bit(hi) == bit(j):
        hi += 1
    if bit(j):
        return 1, lo, hi, None, None
    plo = lo - 1
    while bit(plo - 1):
        plo -= 1
    nhi = hi + 1
    while bit(nhi):
        nhi += 1
    return 0, lo, hi, plo, nhi


def theta(ramp, t, dtype=np.float64):
    """theta, theta', theta'' at t >= 0"""
    t = np.asarray(t, dtype)
    ramp = dtype(ramp)
    if ramp > 0:
        x = t / ramp
        inside = t < ramp
        th = np.where(inside, ramp * (dtype(2.5) * x**4 - 3 * x**5 + x**6), t - ramp / 2)
        thd = np.where(inside, 10 * x**3 - 15 * x**4 + 6 * x**5, dtype(1))
        thdd = np.where(inside, 30 * x**2 * (1 - x)**2 / ramp, dtype(0))
        return th, thd, thdd
    return t.copy(), np.ones_like(t), np.zeros_like(t)


def pose(th, c, w, start, dtype=np.float64):
    """-> (p_xy [2, n], psi [n]) at path parameter th [n]; c [2, n], w [n], start [3, n]"""
    a = w * th / 2
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(np.abs(a) < dtype(SINC_SMALL), 1 - a * a / 6, np.sin(a) / np.where(a == 0, dtype(1), a))
    m = start[2] + a
    cm, sm = np.cos(m), np.sin(m)
    p = np.stack([start[0] + th * sinc * (cm * c[0] - sm * c[1]), start[1] + th * sinc * (sm * c[0] + cm * c[1])])
    return p, start[2] + w * th


def _rot(psi, x, y):
    c, s = np.cos(psi), np.sin(psi)
    return np.stack([c * x - s * y, s * x + c * y])


def clock(durations, tau, s, dtype=np.float64):
    """-> (k, kT, r, phase) of tau [n] at stride scale s [n], by the header's operations"""
    B = boundaries(durations)
    T = s * dtype(B[-1])
    k = np.floor(tau / T)
    k = np.where(k * T > tau, k - 1, k)
    k = np.where((k + 1) * T <= tau, k + 1, k)
    kT = k * T
    r = tau - kT
    phase = np.zeros(tau.shape, int)
    for j in range(1, len(durations)):
        phase += r >= s * dtype(B[j])
    return k, kT, r, phase


def unresolved(durations, masks, tau, s):
    """[n] bool, the header's "clock that does not resolve in double" -- always evaluated in double, whatever precision the rows are
    computed in: T = s B_n zero or not finite; or, for tau >= 0, k T not finite, or a foot that has a run whose run [a, b) of the phase
    in progress (a = k T + s B_lo, b = k T + s B_hi) does not have b - a positive and finite."""
    tau, s = np.asarray(tau, np.float64), np.asarray(s, np.float64)
    B = boundaries(durations)
    with np.errstate(all="ignore"):
        T = s * B[-1]
        lost = ~(T > 0) | ~np.isfinite(T)
        k, kT, _, phase = clock(durations, np.where(tau < 0, 0.0, tau), s)
        walking = ~(tau < 0)
        lost |= walking & ~np.isfinite(kT)
        for j in range(len(durations)):
            for f in range(4):
                _, lo, hi, _, _ = runs(masks, f, j)
                if lo is not None:
                    D = (kT + s * boundary(B, hi)) - (kT + s * boundary(B, lo))
                    lost |= walking & (phase == j) & (~(D > 0) | ~np.isfinite(D))
    return lost


def boundary_distance(durations, time, wait_time, s):
    """min over the stride's boundaries of |r - s B_j| per sample, in extended precision (r itself near 0 or T counts too)"""
    ld = np.longdouble
    tau = np.asarray(time, ld) - ld(wait_time)
    s = np.asarray(s, ld)
    B = boundaries(durations)
    T = s * ld(B[-1])
    r = tau - np.floor(tau / T) * T
    return np.min([np.abs(r - s * ld(b)) for b in B], axis=0)


def targets(params, strides, time, cmd, gait_id=None, stride_scale=None, start=None, dtype=np.float64):
    """-> (targets [54, n], mask [n]).  params: dict(stance [4, 2], height, swing_height, ramp_time, wait_time); strides: a list of
    (durations, masks); time [n], cmd [3, n], gait_id [n], stride_scale [n], start [3, n] as wbc_gait_set_commands takes them."""
    time = np.asarray(time, np.float64)
    n = time.shape[0]
    cmd = np.asarray(cmd, np.float64)
    gid = np.zeros(n, int) if gait_id is None else np.asarray(gait_id).astype(int)
    sc = np.ones(n) if stride_scale is None else np.asarray(stride_scale, np.float64)
    st0 = np.zeros((3, n)) if start is None else np.asarray(start, np.float64)
    with np.errstate(invalid="ignore"):
        bad = (gid >= len(strides)) | ~(sc > 0) | ~np.isfinite(sc) | ~np.isfinite(time) | ~np.isfinite(cmd).all(0) | ~np.isfinite(st0).all(0)
    out = np.full((54, n), np.nan, dtype)
    mask = np.full(n, 0xF, np.uint8)
    stance = np.asarray(params["stance"], np.float64)
    H, hs, ramp, wait = (params[k] for k in ("height", "swing_height", "ramp_time", "wait_time"))
    for g, (durations, masks) in enumerate(strides):
        sel = np.nonzero(~bad & (gid == g))[0]
        sel = sel[~unresolved(durations, masks, time[sel] - np.float64(wait), sc[sel])]      # malformed too: NaN rows, mask 0xF
        if sel.size == 0:
            continue
        t = time[sel].astype(dtype)
        c, w, s, st = cmd[:2, sel].astype(dtype), cmd[2, sel].astype(dtype), sc[sel].astype(dtype), st0[:, sel].astype(dtype)
        tau = t - dtype(wait)
        pre = tau < 0
        tc = np.where(pre, dtype(0), tau)
        B = boundaries(durations)
        k, kT, r, phase = clock(durations, tc, s, dtype)
        at = lambda i: kT + s * dtype(boundary(B, i))
        o = np.zeros((54, sel.size), dtype)
        # ---- body
        th, thd, thdd = theta(ramp, tc, dtype)
        th, thd, thdd = (np.where(pre, dtype(0), x) for x in (th, thd, thdd))
        p, psi = pose(th, c, w, st, dtype)
        vel = _rot(psi, c[0], c[1])
        o[0:2] = p; o[2] = dtype(H)
        o[3:5] = thd * vel
        o[6:8] = thdd * vel + thd**2 * w * np.stack([-vel[1], vel[0]])
        o[11] = psi; o[14] = w * thd; o[17] = w * thdd
        # ---- feet
        zero = np.zeros(sel.size, dtype)

        def foothold(f, a, b):
            """of the stance run [a, b) of foot f (arrays), a None: the run without beginning"""
            if a is None:
                thm = zero
            else:
                thm = np.where(a <= 0, dtype(0), theta(ramp, np.maximum((a + b) / 2, dtype(0)), dtype)[0])
            pm, psim = pose(thm, c, w, st, dtype)
            return pm + _rot(psim, dtype(stance[f, 0]), dtype(stance[f, 1]))

        known = {}

        def foothold_of(f, lo, hi):
            """foothold() of the stance run between boundaries lo and hi; a stride's phases share their runs, so each is computed once"""
            if (f, lo, hi) not in known:
                known[(f, lo, hi)] = foothold(f, None if lo is None else at(lo), None if lo is None else at(hi))
            return known[(f, lo, hi)]

        m = np.zeros(sel.size, np.uint8)
        for j in range(len(durations)):
            inj = ~pre & (phase == j)
            m[inj] = masks[j]
            for f in range(4):
                contact, lo, hi, plo, nhi = runs(masks, f, j)
                rows = slice(18 + 9 * f, 27 + 9 * f)
                val = np.zeros((9, sel.size), dtype)
                if contact:
                    val[0:2] = foothold_of(f, lo, hi)
                else:
                    a, b = at(lo), at(hi)
                    A, Bf = foothold_of(f, plo, lo), foothold_of(f, hi, nhi)
                    D = b - a
                    u = (tau - a) / D
                    val[0:2] = A + (Bf - A) * (10 * u**3 - 15 * u**4 + 6 * u**5)
                    val[3:5] = (Bf - A) * (30 * u**2 - 60 * u**3 + 30 * u**4) / D
                    val[6:8] = (Bf - A) * (60 * u - 180 * u**2 + 120 * u**3) / D**2
                    val[2] = dtype(hs) * 64 * u**3 * (1 - u)**3
                    val[5] = dtype(hs) * 64 * (3 * u**2 * (1 - u)**3 - 3 * u**3 * (1 - u)**2) / D
                    val[8] = dtype(hs) * 64 * (6 * u * (1 - u)**3 - 18 * u**2 * (1 - u)**2 + 6 * u**3 * (1 - u)) / D**2
                o[rows, :] = np.where(inj, val, o[rows, :])
        m[pre] = 0xF
        for f in range(4):                       # tau < 0: the start stance
            val = np.zeros((9, sel.size), dtype)
            val[0:2] = foothold_of(f, None, None)
            o[18 + 9 * f:27 + 9 * f, :] = np.where(pre, val, o[18 + 9 * f:27 + 9 * f, :])
        out[:, sel] = o
        mask[sel] = m
    return out, mask
