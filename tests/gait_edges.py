"""The edge batches of the gait planner's tests (tests/test_gait_edges_cpu.py on the host twins, tests/test_gait_edges_gpu.py on the
device): inputs that sit ON the decisions of the law of include/wbc_gait.h, where the other gait tests draw their samples again --
times that are a boundary of the stride as the header forms it (a product, a product, a sum) and their two neighbours in double, the
first instants of the clock, the end of the ramp, the two branches of sinc, and legal instances whose clock does not resolve in double.
Pure numpy (the oracles are numpy too): no device, no ctypes.  Every batch is seeded, read-only, and no multiple of 16 instances long,
so that the last wavefront of a launch is a tail.  Test infrastructure only."""
import functools

import numpy as np

import follow_oracle as fo
import gait_oracle as go
import gait_schedule_oracle as gso
import gait_terrain_oracle as gto

SCALES = (0.5, 0.77, 1.0, 1.3, 2.0, 0.3141592653589793)
STRIDE_NUMBERS = (0, 1, 2, 3, 7, 50, 1000, 123457)
CMD = (0.3, 0.1, 0.4)
NEAR = 1e-9                     # the clearance of tests/test_gait_terrain_cpu.py and tests/test_gait_schedule_cpu.py
MAX_GRADE = 0.45                # tests/test_gait_terrain_cpu.py: no piece of the sixteen profiles is steep by a rounding
BLEND = 2.0 ** -6               # the schedule cases' blend [path parameter]
EIGHT = ((0.15, 0.1, 0.15, 0.1, 0.15, 0.1, 0.15, 0.1), (14, 15, 13, 15, 11, 15, 7, 15))   # the eight-phase stride of the sixteen


def params(ramp_time=0.5, wait_time=0.0):
    """host_gait.params("mini_cheetah", ...) without its ctypes: the same numbers (asserted in tests/test_gait_edges_cpu.py)"""
    from quadruped_drake_amd import workloads
    st = np.array(workloads.STAND_FEET["mini_cheetah"], dtype=np.float64)[:, :2]
    return dict(stance=st, height=float(workloads.NOMINAL_HEIGHT["mini_cheetah"]), swing_height=0.05, ramp_time=float(ramp_time),
                wait_time=float(wait_time))


def _finish(batch):
    """the batch made no multiple of 16 long (its first three samples once more at the end) and read-only"""
    n = batch["time"].shape[0]
    if n % 16 == 0:
        for k, a in batch.items():
            if isinstance(a, np.ndarray):
                batch[k] = np.concatenate([a, a[..., :3]], axis=-1)
    for a in batch.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    assert batch["time"].shape[0] % 16 != 0
    return batch


def commands(rng, n):
    """seeded commands and starts: |c| <= 1 m/s per axis, |omega| <= 2 rad/s and zero for every sixth, starts over +-1 m and +-3 rad"""
    cmd = np.stack([rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n), rng.uniform(-2.0, 2.0, n)])
    cmd[2, ::6] = 0.0
    st = np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(-3, 3, n)])
    return cmd, st


def boundaries(strides, wait_time, seed=71):
    """For every stride (durations, masks) of `strides`, scale of SCALES, stride number k of STRIDE_NUMBERS and boundary j < nphase:
    tau0 = fl(fl(k T) + fl(s B_j)) with T = fl(s B_n), and its two neighbours in double; samples with tau < 0 are dropped;
    time = fl(tau + wait_time).  With wait_time = 0 the hits are exact: the kernel's tau is tau0 itself, which is the start a of
    the runs that begin at that boundary.
    -> dict(time, tau [n]: what the batch was built from; gid, sc, k, j, kind (-1, 0, +1: neighbour below, the boundary, above) [n];
    lift [4, n]: the sample is tau0 of a boundary at which that foot's swing run begins; cmd [3, n], st [3, n])"""
    rows = []
    for g, (d, m) in enumerate(strides):
        B = go.boundaries(d)
        n = len(d)
        for s in SCALES:
            T = s * B[-1]
            for k in STRIDE_NUMBERS:
                for j in range(n):
                    tau0 = float(k) * T + s * B[j]
                    lifts = [((m[(j - 1) % n] >> f) & 1) == 1 and ((m[j] >> f) & 1) == 0 for f in range(4)]
                    for kind, tau in ((-1, np.nextafter(tau0, -np.inf)), (0, tau0), (1, np.nextafter(tau0, np.inf))):
                        if tau < 0:
                            continue
                        rows.append((tau + wait_time, tau, g, s, k, j, kind) + tuple(bool(x) and kind == 0 for x in lifts))
    a = np.array(rows, dtype=np.float64).T
    cmd, st = commands(np.random.default_rng(seed), a.shape[1])
    return _finish(dict(time=a[0].copy(), tau=a[1].copy(), gid=a[2].astype(np.uint8), sc=a[3].copy(), k=a[4].astype(np.int64), j=a[5].astype(np.int64),
                        kind=a[6].astype(np.int64), lift=a[7:11].astype(bool), cmd=cmd, st=st))


def clock_start(strides, wait_time, seed=72):
    """The first instants of the clock on `strides` (the caller passes those whose phase 0 lifts a foot or has a swing under way, and
    the trot) at three scales: wait - ulp, wait, wait + ulp, the largest double below wait, and with wait_time = 0 also -0.0, 0.0 and
    5e-324.  -> dict(time, gid, sc, cmd, st, before [n]: time < wait_time, the standing branch)"""
    w = float(wait_time)
    times = [w - np.spacing(w), w, w + np.spacing(w), np.nextafter(w, -np.inf)] + ([-0.0, 0.0, 5e-324] if w == 0.0 else [])
    rows = [(t, g, s) for g in range(len(strides)) for s in (0.5, 0.77, 1.0) for t in times]
    a = np.array(rows, dtype=np.float64).T
    cmd, st = commands(np.random.default_rng(seed), a.shape[1])
    b = _finish(dict(time=a[0].copy(), gid=a[1].astype(np.uint8), sc=a[2].copy(), cmd=cmd, st=st))
    b["before"] = b["time"] < w
    return b


def ramp_end(nstrides, ramp_time, seed=73):
    """wait_time = 0, so time = tau: ramp - ulp, ramp, ramp + ulp and 0 on every one of `nstrides` strides at three scales.  At
    ramp_time = 0 the first is -5e-324 (standing) and gait_theta forms 0 / 0 at tau = 0 before its select."""
    r = float(ramp_time)
    times = [r - np.spacing(r), r, r + np.spacing(r), 0.0]
    rows = [(t, g, s) for g in range(nstrides) for s in (0.5, 1.0, 1.3) for t in times]
    a = np.array(rows, dtype=np.float64).T
    cmd, st = commands(np.random.default_rng(seed), a.shape[1])
    cmd[2] = np.where(cmd[2] == 0.0, 0.7, cmd[2])                 # every instance turns: the ramp's rows all carry omega
    return _finish(dict(time=a[0].copy(), gid=a[1].astype(np.uint8), sc=a[2].copy(), cmd=cmd, st=st))


def sinc_edge(seed=74):
    """ramp_time = wait_time = 0, so the body's path parameter is the time: theta in {0.7, 3, 11} s and the yaw rates whose
    a = fl(fl(omega theta) / 2), as gait_pose forms it, is 1e-4 or one of the four values nearest to it on either side that any omega
    reaches (omega's own spacing times theta / 2 is wider than a's, so not every double near 1e-4 is one), in both signs; and
    omega = 0, 5e-324 and -5e-324.  One stride, scale 1."""
    rows = []
    for th in (0.7, 3.0, 11.0):
        w = 2.0 * go.SINC_SMALL / th
        for _ in range(12):
            w = np.nextafter(w, 0.0)
        reached = {}
        for _ in range(25):                                          # a is monotone in omega: the scan meets every value it can take
            reached.setdefault(0.5 * (w * th), w)
            w = np.nextafter(w, 1.0)
        below = sorted(a for a in reached if a < go.SINC_SMALL)[-4:]
        above = sorted(a for a in reached if a >= go.SINC_SMALL)[:5]          # 1e-4 itself, which every theta here reaches, and four above
        assert len(below) == 4 and len(above) == 5 and above[0] == go.SINC_SMALL
        for a in below + above:
            rows += [(th, reached[a]), (th, -reached[a])]
        rows += [(th, 0.0), (th, 5e-324), (th, -5e-324)]
    a = np.array(rows, dtype=np.float64).T
    cmd, st = commands(np.random.default_rng(seed), a.shape[1])
    cmd[2] = a[1]
    b = _finish(dict(time=a[0].copy(), gid=np.zeros(a.shape[1], np.uint8), sc=np.ones(a.shape[1]), cmd=cmd, st=st))
    half = np.abs(0.5 * (b["cmd"][2] * b["time"]))
    assert (half == go.SINC_SMALL).sum() >= 6 and ((half < go.SINC_SMALL) & (half > 0.99 * go.SINC_SMALL)).sum() >= 24
    return b


# (stride_scale, time): legal instances whose clock does or does not resolve in double (the first six do not on a stride with a swing)
UNRESOLVED = [(5e-324, 1.0), (1e-310, 1.0), (1e-200, 1.0), (1e-17, 1.0), (1.0, 1e300), (1.0, 1.7e308), (1e-9, 1.0), (1e9, 1.0), (1e200, 1.0),
              (1e308, 1.0), (1.0, 1e15)]


def unresolved(nstrides):
    """UNRESOLVED on each of `nstrides` strides, under the command CMD.  -> dict(time, gid, sc, cmd, st)"""
    rows = [(t, g, s) for g in range(nstrides) for s, t in UNRESOLVED]
    a = np.array(rows, dtype=np.float64).T
    n = a.shape[1]
    return _finish(dict(time=a[0].copy(), gid=a[1].astype(np.uint8), sc=a[2].copy(), cmd=np.tile(np.array(CMD)[:, None], (1, n)), st=np.zeros((3, n))))


# ---- the four target kernels' cases on the boundaries batch: inputs and the two oracles, computed once per process
def terrain_kw(gid):
    """every stride walks its own profile of follow_oracle's sixteen; the terrain scales are dealt round"""
    n = gid.shape[0]
    return dict(profiles=fo.sixteen_profiles(), terrain_id=(gid % 16).astype(np.uint8), terrain_scale=np.array(fo.SCALES)[(np.arange(n) // 3) % 4].copy(),
                tp=gto.tparams(body="fit", max_grade=MAX_GRADE))


def _switches(rng, th, sel, ahead=None):
    """For the instances `sel`: two switches before the path parameter th -- Theta_1, Theta_2 >= Theta_1 + BLEND, and every third
    instance inside the second blend window -- where th leaves room for them (th >= 2 BLEND + 0.02) and `ahead` [n] does not ask
    otherwise, else two switches after it; a third switch after th for every other instance.
    -> (m, when [7], cmds [21], room: the two switches lie before th) of those instances"""
    n = sel.size
    t = th[sel]
    room = (t >= 2 * BLEND + 0.02) & (True if ahead is None else ~ahead[sel])
    avail = np.where(room, t - 2 * BLEND, 1.0)
    th1 = avail * rng.uniform(0.1, 0.4, n)
    th2 = th1 + BLEND + (avail - th1) * rng.uniform(0.2, 0.7, n)
    inside = room & (sel % 3 == 0) & (t - 0.75 * BLEND >= th1 + BLEND)
    th2 = np.where(inside, t - BLEND * rng.uniform(0.25, 0.75, n), th2)
    th1 = np.where(room, th1, t + 0.5 + rng.uniform(0.0, 1.0, n))
    th2 = np.where(room, th2, th1 + BLEND + rng.uniform(0.1, 1.0, n))
    third = sel % 2 == 0
    when, cmds = np.full((7, n), np.nan), np.full((21, n), np.nan)
    when[0], when[1] = th1, th2
    when[2, third] = (np.maximum(th2, t) + BLEND + rng.uniform(0.1, 1.0, n))[third]
    for j in range(3):
        c = np.stack([rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n), rng.uniform(-2.0, 2.0, n)])
        c[2, (sel + j) % 5 == 0] = 0.0
        used = np.ones(n, bool) if j < 2 else third
        cmds[3 * j:3 * j + 3, used] = c[:, used]
    return np.where(third, 3, 2).astype(np.uint8), when, cmds, room


def schedule_for(P, b, seed=76):
    """A schedule (m, when, cmds) for the small batch b on the handle P: the odd instances switch twice before their time where it
    leaves room, the even ones keep both switches ahead of them -- their body is then still on the arc of their own command"""
    n = b["time"].shape[0]
    tau = b["time"] - P["wait_time"]
    with np.errstate(all="ignore"):                     # unresolved(): a time of 1e300 s overflows the ramp's powers, which are not used
        th = go.theta(P["ramp_time"], np.where(tau < 0, 0.0, tau))[0]
    return _switches(np.random.default_rng(seed), th, np.arange(n), ahead=np.arange(n) % 2 == 0)[:3]


@functools.lru_cache(maxsize=None)
def case(strides, kernel, wait_time):
    """The boundaries batch of `strides` (a tuple of (durations, masks) with tuples inside) for one of the four target kernels --
    "plain", "terrain", "schedule", "schedule_terrain" -- with both oracles.  The times are the batch's, never redrawn: for the terrain
    kernels commands and starts are drawn again until no foothold lies within NEAR of a decision of the terrain law, for the schedule
    kernels the schedule (and under a terrain the commands and starts too) until no pose evaluation lies within NEAR of a Theta_j or a
    window's end.  -> dict(b: the batch as it was built, P, S, cmd, st, kw: the terrain's arrays or {}, sched: (m, when, cmds) or None,
    room [n] (schedule kernels: the instance has its two switches before its time), redrawn: instances drawn again,
    o64, m64, o80, m80)"""
    b = boundaries(strides, wait_time)
    n = b["time"].shape[0]
    P = params(wait_time=wait_time)
    S = [(list(d), list(m)) for d, m in strides]
    terrain, scheduled = kernel in ("terrain", "schedule_terrain"), kernel in ("schedule", "schedule_terrain")
    rng = np.random.default_rng([75, ("plain", "terrain", "schedule", "schedule_terrain").index(kernel), int(4 * wait_time)])
    cmd, st = b["cmd"].copy(), b["st"].copy()
    kw = terrain_kw(b["gid"]) if terrain else {}
    sched, room = None, None
    if scheduled:
        tau = b["time"] - P["wait_time"]
        th = go.theta(P["ramp_time"], np.where(tau < 0, 0.0, tau))[0]
        m, when, cmds, room = _switches(rng, th, np.arange(n))
        sched = [m, when, cmds]

    def oracle(dtype, info=None):
        if scheduled:
            return gso.targets(P, S, b["time"], cmd, sched[0], sched[1], sched[2], BLEND, b["gid"], b["sc"], st, dtype=dtype, info=info, **kw)
        if terrain:
            return gto.targets(P, S, kw["tp"], kw["profiles"], b["time"], cmd, b["gid"], b["sc"], st, kw["terrain_id"], kw["terrain_scale"],
                               dtype=dtype, info=info)
        return go.targets(P, S, b["time"], cmd, b["gid"], b["sc"], st, dtype=dtype)

    redrawn = 0
    for _ in range(30):
        if kernel == "plain":
            o80, m80 = oracle(np.longdouble)
            break
        info = {}
        o80, m80 = oracle(np.longdouble, info)
        again = np.zeros(n, bool)
        if terrain:
            again |= np.asarray(info["terrain_near" if scheduled else "near"], np.float64) < NEAR
        if scheduled:
            again |= np.asarray(info["near"], np.float64) < NEAR
        if not again.any():
            break
        sel = np.nonzero(again)[0]
        redrawn += sel.size
        if terrain:
            cmd[:, sel], st[:, sel] = commands(rng, sel.size)
        if scheduled:
            sched[0][sel], sched[1][:, sel], sched[2][:, sel], room[sel] = _switches(rng, th, sel)
    else:
        raise AssertionError("the %s case keeps %d instances within %g of a decision" % (kernel, int(again.sum()), NEAR))
    o64, m64 = oracle(np.float64)
    out = dict(b=b, P=P, S=S, cmd=cmd, st=st, kw=kw, sched=None if sched is None else tuple(sched), room=room, redrawn=redrawn,
               o64=o64, m64=m64, o80=o80, m80=m80)
    for a in [cmd, st, o64, m64, o80, m80] + (list(sched) if sched else []) + ([room] if room is not None else []):
        a.setflags(write=False)
    return out


def bars(o64, o80, k, groups):
    """{(group, k): 100 x max |oracle64 - oracle80| over the rows of the group and the samples of stride number k}: the project's bar,
    taken over the samples of the same k only, so that the samples at large times do not loosen the bar of those at small ones"""
    out = {}
    for kk in sorted(set(k.tolist())):
        sel = k == kk
        for name, rows in groups:
            out[(name, kk)] = 100.0 * float(np.abs(o64[rows][:, sel].astype(np.longdouble) - o80[rows][:, sel]).max())
    return out


def worst(got, want, k, groups):
    """{(group, k): max |got - want|}, as bars() groups them"""
    out = {}
    for kk in sorted(set(k.tolist())):
        sel = k == kk
        for name, rows in groups:
            out[(name, kk)] = float(np.abs(got[rows][:, sel] - want[rows][:, sel]).max())
    return out


# ---- the feedback pass on exact lift-offs and an exact u_hold
DYADIC = ((0.25, 0.125, 0.25, 0.125), (0b1001, 0b1111, 0b0110, 0b1111))      # tests/test_gait_cpu.py's: every product and sum of its clock is exact
FEEDBACK = dict(k_v=0.25, k_p=0.5, d_max=5.0 * 2.0 ** -7, u_hold=0.5)         # dyadic gains; d_max = |(3, 4)| 2^-7


def feedback_ties(n=17, ticks=64, seed=77):
    """n instances on DYADIC at the scales 1, 0.5 and 2, ramp_time = wait_time = 0, `ticks` calls at k 2^-5 s: every boundary of every
    instance is a tick, so ticks fall exactly on lift-offs and touch-downs, and the middle of every swing is one too: u == u_hold.
    Instances 0 and 1 stand under a zero command with the trunk on its planned position, so their raw offset is k_v times the
    measured velocity, exactly: (3, 4) 2^-7 -- whose norm IS d_max -- on the ticks where a foot in the air has u == u_hold, and
    (d_max, 0) on every other tick.  If `u <= u_hold` takes, `to` holds (3, 4) 2^-7 from that tick on; if it did not, (d_max, 0).
    Every number of the pass is then exact in double for them.  The others get seeded commands and perturbations.
    -> dict(P, par, dt, times [ticks, n], cmd [3, n], sc [n], dq, dv [ticks, 2, n], exact: [0, 1], hold [ticks, n]: a foot in the air
    has u == u_hold, edge [ticks, n]: the tick is a lift-off or a touch-down)"""
    rng = np.random.default_rng(seed)
    dt = 2.0 ** -5
    sc = np.array([1.0, 0.5, 2.0])[np.arange(n) % 3].copy()
    cmd = np.stack([rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n), rng.uniform(-2.0, 2.0, n)])
    cmd[:, :2] = 0.0
    times = np.repeat((np.arange(ticks) * dt)[:, None], n, axis=1)
    r = np.mod(times, 0.75 * sc[None, :])                                      # exact: all dyadic
    hold = (r == 0.125 * sc) | (r == 0.5 * sc)                                 # the middle of [0, 0.25 s) and of [0.375 s, 0.625 s)
    edge = (r == 0.0) | (r == 0.25 * sc) | (r == 0.375 * sc) | (r == 0.625 * sc)
    dq, dv = 0.05 * rng.uniform(-1, 1, (ticks, 2, n)), 0.3 * rng.uniform(-1, 1, (ticks, 2, n))
    dq[:, :, :2] = 0.0
    par = dict(FEEDBACK)
    for i in range(2):
        dv[:, 0, i] = np.where(hold[:, i], 3.0, 5.0) * 2.0 ** -7 / par["k_v"]
        dv[:, 1, i] = np.where(hold[:, i], 4.0, 0.0) * 2.0 ** -7 / par["k_v"]
    assert hold[:, :2].sum() >= 8 and edge[:, :2].sum() >= 16 and n % 16 != 0
    out = dict(P=params(ramp_time=0.0), par=par, dt=dt, times=times, cmd=cmd, sc=sc, dq=dq, dv=dv, exact=[0, 1], hold=hold, edge=edge)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out
