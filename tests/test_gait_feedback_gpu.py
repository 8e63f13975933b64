"""The gait planner's foot-placement feedback on the device (include/wbc_gait_feedback.h): wbc_gait_feedback_kernel against
the host twin at the smallest shapes at which the quad mapping can go wrong, the law's exact relations, damaged instances in every
slot of a wavefront, one handle through every change of its configuration against fresh handles, the kernels' resources, the rollouts with feedback against the launches made by hand, and a batch of pushed
walks against the host twins.  Measured figures: profiles/r16/gait_feedback.md."""
import ctypes as C
import functools

import numpy as np
import pytest

import gait_feedback_oracle as gfo
import host_gait as hg
import host_gait_feedback as hgf
import plant_edges as pe
import test_gait_feedback_cpu as tfc
from quadruped_drake_amd import _lib, gait, workloads
from test_gait_gpu import COMMANDS5, DEV, MODEL, _ptr, _sync, _t

pytestmark = pytest.mark.gpu

TEN = list(gait.STRIDES)
TICKS = 120
FILL = 7.5
# what the four gait kernels report on the parent commit's build (its wbc_*_kernel_info on an MI355X and its compiler's metadata,
# profiles/r15/gait_schedule.md): (registers, LDS bytes); scratch 0, 64 threads
PARENT = {"plain": (112, 26208), "terrain": (194, 31424), "schedule": (116, 26208), "schedule_terrain": (192, 31424)}


class RawFeedbackGait:
    """A wbc_gait handle with feedback through the C ABI, with arrays of any leading dimension"""

    def __init__(self, strides, P, cap, par, ld, cmd, gid=None, sc=None, schedule=None):
        import torch
        self.L, self.ld = _lib.lib(), ld
        self.h = C.c_void_p()
        cp = gait.c_params(P["stance"], P["height"], P["swing_height"], P["ramp_time"], P["wait_time"])
        _lib.check(self.L.wbc_gait_create(C.byref(cp), gait.c_strides(strides), len(strides), 0, C.byref(self.h)))
        self.keep = [_t(cmd), None if gid is None else _t(gid), None if sc is None else _t(sc)]
        _lib.check(self.L.wbc_gait_set_commands(self.h, _ptr(self.keep[0]), _ptr(self.keep[1]), _ptr(self.keep[2]), None))
        self.stream = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
        if schedule is not None:
            m, when, cmds, blend = schedule
            tm, tw, tc = _t(m), _t(when), _t(cmds)
            _lib.check(self.L.wbc_gait_set_schedule(self.h, self.stream, cap, ld, float(blend), _ptr(tm), _ptr(tw), _ptr(tc)))
        if par is not None:
            self.reset(par, cap)

    def reset(self, par, cap):
        self.cap = cap
        _lib.check(self.L.wbc_gait_set_feedback(self.h, C.byref(hgf.c_feedback(par)), cap))

    def buffers(self, ticks):
        import torch
        return (torch.full((ticks, 54, self.ld), FILL, dtype=torch.float64, device=DEV), torch.full((ticks, self.ld), 0x55, dtype=torch.uint8, device=DEV),
                torch.full((ticks, 8, self.ld), FILL, dtype=torch.float64, device=DEV))

    def plain(self, n, times):
        """wbc_gait_targets at times [ticks, ld] -> (targets [ticks, 54, ld], mask [ticks, ld]), numpy"""
        tm = _t(times)
        tg, mk, _ = self.buffers(times.shape[0])
        for k in range(times.shape[0]):
            _lib.check(self.L.wbc_gait_targets(self.h, self.stream, n, self.ld, _ptr(tm[k]), _ptr(tg[k]), _ptr(mk[k])))
        _sync()
        return tg.cpu().numpy(), mk.cpu().numpy()

    def measured(self, n, times, q, v, offsets=True):
        """wbc_gait_targets_measured tick by tick on times [ticks, ld], q [ticks, 19, ld], v [ticks, 18, ld] -> (targets, mask, offsets)"""
        tm, tq, tv = _t(times), _t(q), _t(v)
        tg, mk, of = self.buffers(times.shape[0])
        for k in range(times.shape[0]):
            _lib.check(self.L.wbc_gait_targets_measured(self.h, self.stream, n, self.ld, _ptr(tm[k]), _ptr(tq[k]), _ptr(tv[k]), _ptr(tg[k]), _ptr(mk[k]),
                                                        _ptr(of[k]) if offsets else None))
        _sync()
        return tg.cpu().numpy(), mk.cpu().numpy(), of.cpu().numpy()

    def state(self, n):
        """-> (state [6, 4 n], prev [n]) read back from the device"""
        st, pv = np.zeros((6, 4 * n)), np.zeros(n, np.uint8)
        fn = self.L.wbc_gait_feedback_state_
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        _lib.check(fn(self.h, n, C.c_void_p(st.ctypes.data), C.c_void_p(pv.ctypes.data)))
        return st, pv

    def close(self):
        self.L.wbc_gait_destroy(self.h)


def _inputs(ld, shift=0):
    """tests/test_gait_feedback_cpu.py's sequence cut to 120 ticks for ld instances at stride scales 0.13 .. 0.17 (a trot's stride is
    then 0.15 s: every foot lifts and lands twice in the 0.3 s), instance i on stride (i + shift) mod 10 of the reference's ten"""
    P, cmd, sc, times, dq, dv = tfc.sequence("device", TICKS, n=ld, scales=(0.13, 0.17))
    gid = ((np.arange(ld) + shift) % 10).astype(np.uint8)
    return P, cmd, sc, times, dq, dv, gid


def _schedule(ld):
    """three switches inside the 0.3 s (theta reaches 0.069 there), a blend of 0.01"""
    m = np.full(ld, 3, np.uint8)
    when = np.zeros((7, ld)); when[0], when[1], when[2] = 0.01, 0.03, 0.05
    cmds = np.zeros((21, ld)); cmds[0], cmds[3], cmds[5], cmds[6] = 0.4, 0.2, 0.5, -0.3
    return m, when, cmds, 0.01


def _measure(tg, dq, dv):
    """q [ticks, 19, ld], v [ticks, 18, ld] from the rows the device's own gait kernel wrote, so that the device's pass and the twin's
    work on the same bits"""
    q, v = zip(*(tfc.measured(np.where(np.isfinite(tg[k]), tg[k], 0.0), dq[k], dv[k]) for k in range(tg.shape[0])))
    return np.stack(q), np.stack(v)


@pytest.mark.parametrize("scheduled", [False, True], ids=["plain", "schedule"])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 33])
def test_feedback_kernel_matches_the_host_twin(n, scheduled):
    """n = 1, 15 (a quad short of a wavefront), 16 (exactly one), 17 (one robot into the next), 33 (into a third), ld = n + 3; all ten
    strides (for n = 1 one after the other), with and without a schedule; 120 ticks.  The twin's pass runs on the rows the device's gait
    kernel wrote.  Rows, offsets and the state read back after the last tick, at the CPU test's bar -- 4 x the oracle's distance between
    double and extended precision on these inputs -- and its near-tie rule, at most 2 % left out.  Measured: the device's pass equals
    the twin's bit for bit in every case (worst 0)."""
    ld = n + 3
    for shift in (range(10) if n < 10 else (0,)):
        P, cmd, sc, times, dq, dv, gid = _inputs(ld, shift)
        g = RawFeedbackGait(TEN, P, n, tfc.PAR, ld, cmd, gid, sc, _schedule(ld) if scheduled else None)
        plain, pmask = g.plain(n, times)
        q, v = _measure(plain, dq, dv)
        got, gmask, goff = g.measured(n, times, q, v)
        gstate, gprev = g.state(n)
        g.close()
        assert (got[:, :, n:] == FILL).all() and (goff[:, :, n:] == FILL).all() and (gmask[:, n:] == 0x55).all()   # the padding columns
        assert (gmask[:, :n] == pmask[:, :n]).all()
        eng = [tfc.Twin(n), tfc.Oracle(n), tfc.Oracle(n, np.longdouble)]
        alive, left = np.ones(n, bool), 0
        bar, worst = {k: 0.0 for k, _ in tfc.GROUPS}, {k: 0.0 for k, _ in tfc.GROUPS}
        for k in range(TICKS):
            a = [np.ascontiguousarray(x[..., :n]) for x in (times[k], q[k], v[k], plain[k], pmask[k], gid, sc)]
            (rt, ot), (rd, od), (rw, ow) = (e.step(tfc.PAR, P, TEN, *a) for e in eng)
            alive &= ~((eng[1].decisions != eng[2].decisions).any(1) | eng[1].near | eng[2].near)
            left += int((~alive).sum())
            if not alive.any():
                continue
            for grp, rows in tfc.GROUPS:
                sets = [(got[k][rows][:, :n], rt[rows], rd[rows], rw[rows])] + ([(goff[k][:, :n], ot, od, ow)] if grp == "positions" else [])
                for dev, twin, o64, o80 in sets:
                    bar[grp] = max(bar[grp], 4 * float(np.abs(o64[:, alive] - o80[:, alive]).max()))
                    worst[grp] = max(worst[grp], float(np.abs(dev[:, alive] - twin[:, alive]).max()))
            body = [r for r in range(54) if r not in sum((rows for _, rows in tfc.GROUPS), [])]
            assert pe.same_bits(got[k][body][:, :n], plain[k][body][:, :n])                  # body rows and z rows: not written
        tstate, tprev = eng[0].packed()
        s80 = eng[2].packed()[0]
        sel = np.repeat(alive, 4)
        if alive.any():
            bar["positions"] = max(bar["positions"], 4 * float(np.abs(eng[1].packed()[0][:, sel] - s80[:, sel]).max()))
            worst["positions"] = max(worst["positions"], float(np.abs(gstate[:, sel] - tstate[:, sel]).max()))
        assert (gprev == tprev).all()
        print("GAIT-FEEDBACK device-to-twin n=%d %s shift %d: left out %d of %d; %s" %
              (n, "schedule" if scheduled else "plain", shift, left, n * TICKS, ", ".join("%s worst %.3g bar %.3g" % (k, worst[k], bar[k]) for k in bar)))
        assert left <= 0.02 * n * TICKS
        for k in bar:
            assert worst[k] <= bar[k] and (bar[k] > 0 or TEN[int(gid[0])] == "stand"), (n, k, worst[k], bar[k])


def test_zero_gains_feedback_set_and_padding_change_no_bit():
    """k_v = k_p = 0: every row == the plain kernel's, the offsets exactly 0.  wbc_gait_targets on a handle with feedback set returns the
    bits of a handle without.  Columns n .. ld of targets and offsets keep what was in them.  And what wbc_gait_targets_measured refuses
    only with a device at hand: a terrain on the handle, n above wbc_gait_set_feedback's, and feedback cleared."""
    from quadruped_drake_amd import terrain as tr
    n, ld = 17, 20
    P, cmd, sc, times, dq, dv, gid = _inputs(ld)
    fresh = RawFeedbackGait(TEN, P, n, None, ld, cmd, gid, sc)
    want, wmask = fresh.plain(n, times)
    fresh.close()
    g = RawFeedbackGait(TEN, P, n, dict(tfc.PAR, k_v=0.0, k_p=0.0), ld, cmd, gid, sc)
    plain, pmask = g.plain(n, times)
    assert pe.same_bits(plain, want) and (pmask == wmask).all()
    q, v = _measure(plain, dq, dv)
    got, gmask, goff = g.measured(n, times, q, v)
    assert (got[:, :, :n] == plain[:, :, :n]).all() and (goff[:, :, :n] == 0).all() and (gmask == pmask).all()
    assert (got[:, :, n:] == FILL).all() and (goff[:, :, n:] == FILL).all()
    g.reset(tfc.PAR, n)
    moved, _, off = g.measured(n, times, q, v)
    assert float(np.abs(off[:, :, :n]).max()) > 0.01 and not pe.same_bits(moved, plain)
    again, amask = g.plain(n, times)
    assert pe.same_bits(again, want) and (amask == wmask).all()                            # wbc_gait_targets: still a function of the time
    # misuse that needs a device to set up
    L, err = g.L, (lambda: g.L.wbc_last_error().decode())
    tm, tq, tv = _t(times[0]), _t(q[0]), _t(v[0])
    tg, mk, of = g.buffers(1)
    call = lambda n_: L.wbc_gait_targets_measured(g.h, g.stream, n_, ld, _ptr(tm), _ptr(tq), _ptr(tv), _ptr(tg[0]), _ptr(mk[0]), _ptr(of[0]))
    assert call(n + 1) < 0 and "larger than the n" in err()
    tp = gait.c_terrain_params()
    arr = tr.c_array([tr.ramp_step(0.3, 0.05)])
    _lib.check(L.wbc_gait_set_terrain(g.h, C.byref(tp), C.cast(arr, C.c_void_p), 1, None, None))
    assert call(n) < 0 and "terrain" in err()
    _lib.check(L.wbc_gait_set_terrain(g.h, None, None, 0, None, None))
    assert call(n) == 0
    _lib.check(L.wbc_gait_clear_feedback(g.h))
    assert call(n) < 0 and "wbc_gait_set_feedback" in err()
    _sync()
    assert (tg[0][:, n:] == FILL).all().item()
    g.close()


def test_one_handle_through_its_life_equals_fresh_handles_step_by_step():
    """n = 5 (two quads, the second partly empty), ld = 8 and then 16, one handle through: commands; a schedule at ld 8; cleared; commands
    and a schedule at ld 16 (the handle's buffer regrows); feedback for 5; wbc_gait_targets_measured over two runs of ticks; feedback
    cleared; feedback for 3 and a run at n = 3; a terrain set and unset; destroy.  After every step its targets, masks, offsets and
    state are bit for bit those of a fresh handle brought directly to that configuration, and what it refuses it refuses in the same
    words: n above the schedule's, n above the feedback's, no feedback, measured targets with a terrain set."""
    from quadruped_drake_amd import terrain as tr
    n = 5
    P, cmd, sc, times, dq, dv, gid = _inputs(16)
    times, dq, dv = times[::5], dq[::5], dv[::5]                                             # 24 ticks over the 0.3 s
    half = times.shape[0] // 2
    cut = lambda a, ld: np.ascontiguousarray(a[..., :ld])

    def fresh(ld, schedule, feedback=None):
        f = RawFeedbackGait(TEN, P, n, None, ld, cut(cmd, ld), gid[:ld], sc[:ld], _schedule(ld) if schedule else None)
        if feedback:
            f.reset(tfc.PAR, feedback)
        return f

    def same(a, b):
        return all(pe.same_bits(x, y) for x, y in zip(a, b))

    def set_schedule(g, ld):
        m, when, cmds, blend = _schedule(ld)
        arrays = [_t(m), _t(when), _t(cmds)]
        _lib.check(g.L.wbc_gait_set_schedule(g.h, g.stream, n, ld, float(blend), *[_ptr(a) for a in arrays]))

    def refused(g, n_, what, measured=True):
        """one call at n_ is refused with `what` in the message and writes nothing"""
        tm, tq, tv = _t(cut(times[0], g.ld)), _t(cut(q[0], g.ld)), _t(cut(v[0], g.ld))
        tg, mk, of = g.buffers(1)
        if measured:
            rc = g.L.wbc_gait_targets_measured(g.h, g.stream, n_, g.ld, _ptr(tm), _ptr(tq), _ptr(tv), _ptr(tg[0]), _ptr(mk[0]), _ptr(of[0]))
        else:
            rc = g.L.wbc_gait_targets(g.h, g.stream, n_, g.ld, _ptr(tm), _ptr(tg[0]), _ptr(mk[0]))
        _sync()
        return rc < 0 and what in g.L.wbc_last_error().decode() and (tg == FILL).all().item() and (mk == 0x55).all().item()

    # 1. commands
    g = fresh(8, False)
    f = fresh(8, False)
    plain8 = f.plain(n, cut(times, 8))
    f.close()
    assert same(g.plain(n, cut(times, 8)), plain8)
    # 2. a schedule at ld 8
    set_schedule(g, 8)
    f = fresh(8, True)
    sched8 = f.plain(n, cut(times, 8))
    f.close()
    assert same(g.plain(n, cut(times, 8)), sched8) and not same(sched8, plain8)
    q, v = _measure(np.concatenate([sched8[0], sched8[0]], axis=2), dq, dv)                   # [ticks, 19 | 18, 16]: any finite trunk will do
    assert refused(g, n + 1, "larger than the n of the handle's wbc_gait_set_schedule", measured=False)
    # 3. cleared
    _lib.check(g.L.wbc_gait_clear_schedule(g.h))
    assert same(g.plain(n, cut(times, 8)), plain8) and same(g.plain(n + 1, cut(times, 8))[0][:, :, :n], plain8[0][:, :, :n])
    # 4. commands and a schedule at ld 16: the buffer regrows
    g.ld = 16
    g.keep = [_t(cmd), _t(gid), _t(sc)]
    _lib.check(g.L.wbc_gait_set_commands(g.h, _ptr(g.keep[0]), _ptr(g.keep[1]), _ptr(g.keep[2]), None))
    set_schedule(g, 16)
    f = fresh(16, True, feedback=n)
    sched16 = f.plain(n, times)
    assert same(g.plain(n, times), sched16) and pe.same_bits(sched16[0][:, :, :n], sched8[0][:, :, :n])
    # 5. feedback for n = 5: wbc_gait_targets is what it was
    g.reset(tfc.PAR, n)
    assert same(g.plain(n, times), sched16)
    # 6. measured targets over two runs of ticks: the state carries over
    moved = []
    for lo, hi in ((0, half), (half, 2 * half)):
        got, want = g.measured(n, times[lo:hi], q[lo:hi], v[lo:hi]), f.measured(n, times[lo:hi], q[lo:hi], v[lo:hi])
        assert same(got, want) and same(g.state(n), f.state(n))
        moved.append(got[0])
    f.close()
    assert not pe.same_bits(np.concatenate(moved), sched16[0][:2 * half])                   # the pass did move footholds
    assert refused(g, n + 1, "larger than the n of the handle's wbc_gait_set_feedback")
    assert refused(g, n + 1, "larger than the n of the handle's wbc_gait_set_schedule", measured=False)
    # 7. feedback cleared
    _lib.check(g.L.wbc_gait_clear_feedback(g.h))
    assert refused(g, n, "wbc_gait_set_feedback has not been called") and same(g.plain(n, times), sched16)
    # 8. feedback for n = 3, a run at n = 3
    g.reset(tfc.PAR, 3)
    f = fresh(16, True, feedback=3)
    assert same(g.measured(3, times[:half], q[:half], v[:half]), f.measured(3, times[:half], q[:half], v[:half])) and same(g.state(3), f.state(3))
    assert refused(g, 4, "larger than the n of the handle's wbc_gait_set_feedback")
    # 9. a terrain set and unset
    tp, arr = gait.c_terrain_params(), tr.c_array([tr.slope(0.1, start=-1.0)])             # a slope under every foot: other rows
    for h in (g, f):
        _lib.check(h.L.wbc_gait_set_terrain(h.h, C.byref(tp), C.cast(arr, C.c_void_p), 1, None, None))
    on = g.plain(n, times)
    assert same(on, f.plain(n, times)) and not same(on, sched16) and refused(g, 3, "the handle has a terrain set")
    for h in (g, f):
        _lib.check(h.L.wbc_gait_set_terrain(h.h, None, None, 0, None, None))
    assert same(g.plain(n, times), sched16)
    assert same(g.measured(3, times[half:], q[half:], v[half:]), f.measured(3, times[half:], q[half:], v[half:])) and same(g.state(3), f.state(3))
    f.close()
    # 10. destroy
    assert g.L.wbc_gait_destroy(g.h) == 0


DAMAGE = [("q4", np.nan), ("q5", np.inf), ("v3", -np.inf), ("v4", np.nan), ("time", np.nan), ("time", np.inf), ("gait_id", 200), ("cmd", np.nan)]


def test_a_damaged_instance_in_every_slot_of_a_wavefront():
    """n = 32, 20 ticks, one run per robot slot of a wavefront: from tick 5 on the robot in that slot has a NaN or an inf in one of its
    measured numbers or its time, or NaN rows from the gait (a gait_id past the table, a NaN command).  Its rows are the gait's, its
    state and previous mask those after tick 4, and the other 31 robots keep the bits of the undamaged run."""
    n = ld = 32
    ticks, at = 20, 5
    P, cmd, sc, times, dq, dv, gid = _inputs(ld)
    times, dq, dv = times[:ticks], dq[:ticks], dv[:ticks]
    g = RawFeedbackGait(TEN, P, n, tfc.PAR, ld, cmd, gid, sc)
    plain, _ = g.plain(n, times)
    q, v = _measure(plain, dq, dv)
    g.measured(n, times[:at], q[:at], v[:at])
    state4, prev4 = g.state(n)
    g.reset(tfc.PAR, n)
    clean, cmask, coff = g.measured(n, times, q, v)
    cstate, cprev = g.state(n)
    g.close()
    for slot in range(16):
        kind, value = DAMAGE[slot % len(DAMAGE)]
        t2, q2, v2, gid2, cmd2 = times.copy(), q.copy(), v.copy(), gid.copy(), cmd.copy()
        if kind == "time":
            t2[at:, slot] = value
        elif kind == "gait_id":
            gid2[slot] = value
        elif kind == "cmd":
            cmd2[1, slot] = value
        else:
            (q2 if kind[0] == "q" else v2)[at:, int(kind[1]), slot] = value
        d = RawFeedbackGait(TEN, P, n, tfc.PAR, ld, cmd, gid, sc)
        first = d.measured(n, t2[:at], q2[:at], v2[:at])
        d.keep[0].copy_(_t(cmd2)); d.keep[1].copy_(_t(gid2))                                # the gait's own inputs are damaged from tick 5 on
        raw, _ = d.plain(n, t2[at:])
        rest = d.measured(n, t2[at:], q2[at:], v2[at:])
        dstate, dprev = d.state(n)
        d.close()
        got, goff = np.concatenate([first[0], rest[0]]), np.concatenate([first[2], rest[2]])
        others = np.arange(n) != slot
        assert pe.same_bits(got[:, :, others], clean[:, :, others]) and pe.same_bits(goff[:, :, others], coff[:, :, others]), (slot, kind)
        assert pe.same_bits(dstate[:, np.repeat(others, 4)], cstate[:, np.repeat(others, 4)]) and (dprev[others] == cprev[others]).all(), (slot, kind)
        assert pe.same_bits(got[at:, :, slot], raw[:, :, slot]) and np.isnan(goff[at:, :, slot]).all(), (slot, kind)
        mine = np.repeat(~others, 4)
        assert pe.same_bits(dstate[:, mine], state4[:, mine]) and dprev[slot] == prev4[slot], (slot, kind)


def test_feedback_kernel_resources_and_the_parents_kernels():
    """0 scratch and 64 threads per block; the VGPR and LDS figures are printed.  The four gait kernels of before report what they
    report on the parent commit (PARENT)."""
    from quadruped_drake_amd import terrain as tr
    p = gait.GaitPlanner(MODEL, device=0)
    info = p.feedback_kernel_info()
    print("GAIT-FEEDBACK kernel", info)
    assert info["scratch_bytes_per_lane"] == 0 and info["block_threads"] == 64
    assert info["lds_bytes"] == 8 * (12 + 16 * 204) and 0 < info["num_regs"] <= 128
    old = {"plain": p.kernel_info(), "terrain": p.terrain_kernel_info(), "schedule": p.schedule_kernel_info(False),
           "schedule_terrain": p.schedule_kernel_info(True)}
    for key, (regs, lds) in PARENT.items():
        print("GAIT-FEEDBACK kernel of before", key, old[key])
        assert old[key] == dict(num_regs=regs, scratch_bytes_per_lane=0, lds_bytes=lds, block_threads=64), key
    p.close()


# ---- the rollouts
def _planner(n, feedback=True, cmd=None, **par):
    p = gait.GaitPlanner(MODEL, strides=("trot",), device=0)
    p.set_commands(_t(COMMANDS5[:, :n] if cmd is None else cmd), stride_scale=_t(np.full(n, 0.5)))
    if feedback:
        p.set_feedback(n, **par)
    return p


def _loops(plant, traj, chunks, dt, q0, v0, wrench=None, counts=False):
    """closed_loop call after call (chunks: ticks per call; wrench: per call an ext_wrench or None) with one fresh ID controller
    -> q, v, the last tick's tau, flags, targets and mask (+ counts [4, n])"""
    import torch
    from quadruped_drake_amd import IDController, closed_loop
    n = q0.shape[1]
    ctrl = IDController(max_batch=n, device=0)
    q, v, tm = _t(q0), _t(v0), _t(np.zeros(n))
    cn = torch.zeros((4, n), dtype=torch.int32, device=DEV) if counts else None
    for j, k in enumerate(chunks):
        kw = {} if wrench is None or wrench[j] is None else dict(ext_wrench=wrench[j])
        out = closed_loop(ctrl, plant, traj, k, dt, q, v, tm, counts=cn, **kw)
    _sync()
    res = [x.cpu().numpy() for x in (q, v, out[0], out[6], out[3], out[4])] + ([cn.cpu().numpy()] if counts else [])
    ctrl.close()
    return res


NAMES = ("q", "v", "tau", "flags", "targets", "mask")


@pytest.mark.parametrize("kind", ["ground", "rigid"])
def test_rollouts_with_feedback_equal_the_launches_made_by_hand(kind):
    """40 ticks, n = 5, as two rollout calls of 20 -- the state crosses the call -- against wbc_gait_targets_measured -> wbc_step -> plant
    step issued one by one on a second handle: bit-identical.  With the feedback cleared the rollout equals that of a handle that
    never had any, and differs from the one with feedback."""
    from quadruped_drake_amd import GroundContactPlant, IDController, RigidContactPlant
    n, dt = 5, 5e-3
    q0, v0 = workloads.nominal_state(MODEL, n)
    v0 = v0.copy(); v0[3] = 0.15; v0[4] = np.linspace(-0.2, 0.2, n)                       # a trunk that drifts: the pass has something to do
    plant = (GroundContactPlant if kind == "ground" else RigidContactPlant)(MODEL, device=0)
    planner = _planner(n)
    got = _loops(plant, planner, (20, 20), dt, q0, v0)
    hand = _planner(n)
    ctrl = IDController(max_batch=n, device=0)
    q, v, tm = _t(q0), _t(v0), _t(np.zeros(n))
    for _ in range(40):
        tg, mk = hand.targets_measured(tm, q, v)
        tau, met, st = ctrl.step(q, v, tg, mk)
        if kind == "ground":
            f, ct, fl = plant.step(q, v, tau, dt, time=tm)
        else:
            vd, f, fl = plant.step(q, v, tau, mk, dt, time=tm)
    _sync()
    for a, b, name in zip(got, (q, v, tau, fl, tg, mk), NAMES):
        assert pe.same_bits(a, b.cpu().numpy()), name
    ctrl.close()
    fresh = _planner(n, feedback=False)
    none = _loops(plant, fresh, (20, 20), dt, q0, v0)
    planner.clear_feedback()
    assert not planner.has_feedback
    for a, b, name in zip(none, _loops(plant, planner, (20, 20), dt, q0, v0), NAMES):
        assert pe.same_bits(a, b), name
    assert not pe.same_bits(none[4], got[4])
    plant.close(); planner.close(); hand.close(); fresh.close()


@functools.lru_cache(maxsize=None)
def _host_sweep():
    par = gfo.defaults(workloads.NOMINAL_HEIGHT[MODEL])
    return tfc.host_walk((0.2, 0.0, 0.0), tfc.GRID, None)["flags"], tfc.host_walk((0.2, 0.0, 0.0), tfc.GRID, par)["flags"], par


def test_a_batch_of_pushed_walks_falls_where_the_host_twins_fall():
    """The CPU sweep's grid of lateral pushes (10 N x sqrt(2)^k, ticks 300 .. 319 of 600) in one batch per variant, one robot per force,
    through three rollout calls (300 ticks, 20 with ext_wrench, 280): FELL or BAD as on the host twins.  Robots within one grid step
    of either variant's threshold are exempt (the loop is not contractive to rounding), at most four of them."""
    from quadruped_drake_amd import GroundContactPlant
    import torch
    off_flags, on_flags, par = _host_sweep()
    grid = np.array(tfc.GRID)
    n, dt = grid.size, 5e-3
    q0, v0 = workloads.nominal_state(MODEL, n)
    w = np.zeros((6, n)); w[4] = grid
    cmd = np.tile(np.array([[0.2], [0.0], [0.0]]), (1, n))
    exempt = np.zeros(n, bool)
    for flags in (off_flags, on_flags):
        k = tfc.GRID.index(tfc.survived(flags)) if tfc.survived(flags) else -1
        exempt[max(k, 0):k + 2] = True                                                  # the last force survived and the first not
    fell = {}
    for key, feedback, host in (("off", False, off_flags), ("on", True, on_flags)):
        plant = GroundContactPlant(MODEL, device=0)
        planner = _planner(n, feedback, cmd, **(par if feedback else {}))
        res = _loops(plant, planner, (300, 20, 280), dt, q0, v0, wrench=(None, _t(w), None), counts=True)
        plant.close(); planner.close()
        fell[key] = (res[6][1] > 0) | (res[6][3] > 0)
        want = (np.asarray(host) & (tfc.FELL | tfc.BAD)) != 0
        print("GAIT-FEEDBACK pushed batch, feedback %s: device %s host %s exempt %s" % (key, fell[key].astype(int), want.astype(int), exempt.astype(int)))
        assert (fell[key][~exempt] == want[~exempt]).all(), key
    assert exempt.sum() <= 4


def test_simulate_gait_feedback_and_push_are_wired_and_reported(capsys):
    """python -m quadruped_drake_amd.simulate --planner gait --plant ground with --gait-feedback and --push: the JSON line names both, the
    push (5 N in +y for 0.1 s) splits the rollout at its two ends, nobody falls and the trunks end within the walks' bar of the plan.
    Measured: 1.04 mm off the plan with the default feedback, 0.44 mm with the push."""
    import json
    from quadruped_drake_amd import simulate
    common = ["--control", "ID", "--n", "4", "--sim-time", "0.4", "--dt", "5e-3", "--log-every", "30", "--planner", "gait", "--plant", "ground"]
    lines = {}
    for key, extra in (("plain", []), ("feedback", ["--gait-feedback"]), ("pushed", ["--gait-feedback", "0.17,0,0.1,0.5", "--push", "0.1:0.2:0,5"])):
        rc = simulate.main(common + extra)
        lines[key] = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        assert rc == 0 and lines[key]["FELL"] == 0 and lines[key]["plant_flags"]["bad"] == 0, key
    assert "gait_feedback" not in lines["plain"] and lines["feedback"]["gait_feedback"] == {} and "push" not in lines["feedback"]
    assert lines["pushed"]["gait_feedback"] == dict(k_v=0.17, k_p=0.0, d_max=0.1, u_hold=0.5) and lines["pushed"]["push"] == [0.1, 0.2, 0.0, 5.0]
    assert lines["feedback"]["plan_offset_worst"] < 0.03 and lines["pushed"]["plan_offset_worst"] < 0.03
