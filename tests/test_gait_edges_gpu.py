"""The gait kernels on the MI355X at the ties of their laws (include/wbc_gait.h): the edge batches of tests/gait_edges.py -- times ON
the stride's boundaries as the header forms them and their neighbours in double, the first instants of the clock, the end of the ramp,
the two branches of sinc, legal instances whose clock does not resolve in double, and the feedback pass on exact lift-offs and an exact
u_hold -- through the C ABI with ld > n and preset padding, against the host twins and the oracles of tests/test_gait_edges_cpu.py.
The header fixes the clock operation by operation, and hipcc contracts by default: a kernel that rounds k T + s B_j in one fused
step answers another mask on the samples that a rounding decides (one in sixteen of the boundaries batch) and lifts a foot off the
ground a rounding early.  Measured figures: profiles/r17/gait_edges.md."""
import numpy as np
import pytest

import gait_edges as ge
import plant_edges as pe
import test_gait_edges_cpu as tec
import test_gait_feedback_cpu as tfc
from test_gait_edges_cpu import KERNELS, S16
from test_gait_feedback_gpu import RawFeedbackGait
from test_gait_gpu import SIXTEEN
from test_gait_schedule_gpu import RawScheduleGait

pytestmark = pytest.mark.gpu
PAD = 5


def device(strides, P, time, cmd, gid, sc, st, kw=None, sched=None, blend=ge.BLEND):
    """The target kernel that a handle with these settings launches, on n = len(time) instances in arrays of ld = n + PAD columns: the
    inputs' padding holds NaN (bytes: 0xA5), the outputs' is RawGait's preset and must come back as it was -> (targets [54, n], mask [n])"""
    n = time.shape[0]
    ld = n + PAD
    w = lambda a: None if a is None else pe.wide(a, ld, fill=np.nan if np.asarray(a).dtype == np.float64 else None)
    g = RawScheduleGait(strides, P)
    if kw:
        g.set_terrain(kw["tp"], kw["profiles"], w(kw["terrain_id"]), w(kw["terrain_scale"]))
    if sched is not None:
        tg, mk = g.scheduled(n, ld, w(time), w(cmd), w(gid), w(sc), w(st), blend, w(np.asarray(sched[0], np.uint8)), w(sched[1]), w(sched[2]))
    else:
        tg, mk = g.targets(n, ld, w(time), w(cmd), w(gid), w(sc), w(st))
    g.close()
    assert (tg[:, n:] == 7.5).all() and (mk[n:] == 0x55).all()
    return tg[:, :n], mk[:n]


@pytest.mark.parametrize("kernel", KERNELS)
def test_exact_boundaries_on_every_target_kernel(kernel):
    """The boundaries batch with wait_time 0 and 0.25 -- 10419 samples on the sixteen strides, none drawn again for its time, none left
    out: device mask == twin mask == oracle64 mask on every sample; rows device-to-twin below 100 x max |oracle64 - oracle80| per row
    group, the maximum taken over the samples of the same stride number only; and on the two plane kernels with wait_time = 0, z and
    z-rate exactly 0.0 for every foot at every sample that is exactly its lift-off."""
    for wait in (0.0, 0.25):
        c = ge.case(S16, kernel, wait)
        b = c["b"]
        assert np.array_equal(b["time"], ge.boundaries(S16, wait)["time"])
        print("GAIT-EDGE boundaries %s wait %.2f: times changed 0 of %d, instances drawn again %d" % (kernel, wait, b["time"].shape[0], c["redrawn"]))
        want, wmask = tec.case_twin(c)
        got, gmask = device(SIXTEEN, c["P"], b["time"], c["cmd"], b["gid"], b["sc"], c["st"], c["kw"], c["sched"])
        decided = c["m64"] != c["m80"]
        print("GAIT-EDGE boundaries %s wait %.2f: device masks differ from the twin's on %d samples, from oracle64's on %d; %d samples (%.1f %%) are "
              "decided by a rounding" % (kernel, wait, (gmask != wmask).sum(), (gmask != c["m64"]).sum(), decided.sum(), 100.0 * decided.mean()))
        zeros = None
        if wait == 0.0 and "terrain" not in kernel:
            zeros = [(got[18 + 9 * f + r, b["lift"][f]] != 0.0).sum() for f in range(4) for r in (2, 5)]
            print("GAIT-EDGE boundaries %s: %d exact lift-offs, z or z-rate not exactly 0 on %d" % (kernel, b["lift"].sum(), sum(zeros)))
        assert (gmask == wmask).all() and (wmask == c["m64"]).all() and np.isfinite(got).all()
        tec.check_rows("boundaries %s wait %.2f device-to-twin" % (kernel, wait), got, want, c, kernel)
        assert zeros is None or (sum(zeros) == 0 and b["lift"].sum() > 1000)


def test_clock_start_ramp_end_and_sinc_edge_on_the_device():
    """clock_start, ramp_end (both handles) and sinc_edge on the plain kernel and on the plane schedule kernel: the masks are the double
    oracle's, every row is finite and within the bar of the twin, the standing rows hold strictly before the wait and phase 0 from
    tau = 0 on.  And at ramp_time = 0 the device answers what a handle with ramp_time = 5e-324 answers, to the bar: the select keeps
    the 0 / 0 of gait_theta out.  (At tau = 0 itself the two laws differ by their definition in theta' alone -- 0 inside a ramp, 1
    without one -- so there the body's velocity rows are compared with the law's own, theta' c, not with the other handle.)"""
    for scheduled in (False, True):
        for label, strides, P, b in tec.small_batches():
            sched = ge.schedule_for(P, b) if scheduled else None
            args = (strides, P, b["time"], b["cmd"], b["gid"], b["sc"], b["st"], None, sched)
            o80, _ = tec.oracle(None, *args, dtype=np.longdouble)
            o64, m64 = tec.oracle(None, *args)
            want, wmask = tec.twin(None, *args)
            got, gmask = device(*args)
            tec.check_small(label + (" schedule" if scheduled else " plain") + " device-to-twin", strides, P, b, got, gmask, want, wmask, o64, m64, o80)
            if label.startswith("ramp_end ramp 0.0"):
                tiny, tmask = device(strides, dict(P, ramp_time=5e-324), *args[2:])
                at0 = b["time"] == 0.0
                rates = [3, 4, 6, 7, 14, 17]                                       # the body rows that carry theta' and theta''
                assert at0.any() and (tmask == gmask).all() and np.isfinite(tiny).all()
                same = np.ones(got.shape, bool)
                same[np.ix_(rates, np.nonzero(at0)[0])] = False
                for name, rows in tec.tgc.GROUPS:
                    bar = 100.0 * float(np.abs(o64[rows] - o80[rows]).max())
                    worst = float(np.abs(np.where(same, got - tiny, 0.0)[rows]).max())
                    print("GAIT-EDGE ramp 0 against ramp 5e-324 %s %-13s worst %.3g bar %.3g" % ("schedule" if scheduled else "plain", name, worst, bar))
                    assert worst < bar or (bar == 0 and worst == 0), (name, worst, bar)
                assert (tiny[np.ix_([3, 4, 14], np.nonzero(at0)[0])] == 0.0).all()                   # theta'(0) = 0 inside a ramp ...
                assert np.abs(got[14, at0]).min() > 0 and (got[14, at0] == o64[14, at0]).all()       # ... and 1 without one: omega itself


@pytest.mark.parametrize("kernel", KERNELS)
def test_unresolved_clocks_are_malformed_not_half_nan(kernel):
    """Each instance of gait_edges.unresolved() -- the eleven (scale, time) pairs on walk, stand and the eight-phase stride -- in robot
    slot (case mod 16) of a wavefront of fifteen clean robots: all 54 rows finite, or all 54 NaN with mask 0xF; which of the two is the
    header's verdict (gait_oracle.unresolved) and the twin's; and every neighbour keeps the bits it has in the batch without it."""
    strides, P, u, lost = tec.unresolved_case()
    cases = u["time"].shape[0]
    n = 16 * cases
    rng = np.random.default_rng(78)
    clean = dict(time=rng.uniform(0.0, 6.0, n), gid=(np.arange(n) % len(strides)).astype(np.uint8), sc=rng.uniform(0.5, 2.0, n))
    clean["cmd"], clean["st"] = ge.commands(rng, n)
    where = np.arange(cases) * 16 + np.arange(cases) % 16
    dirty = {k: a.copy() for k, a in clean.items()}
    for k in dirty:
        dirty[k][..., where] = u[k]
    kw_c, sched_c = tec.unresolved_inputs(kernel, clean, P)
    kw_d, sched_u = tec.unresolved_inputs(kernel, dirty, P)
    sched_d = None
    if sched_c is not None:
        sched_u = ge.schedule_for(P, u)
        sched_d = [a.copy() for a in sched_c]
        for a, b in zip(sched_d, sched_u):
            a[..., where] = b
    run = lambda f, b, kw, sched: f(strides, P, b["time"], b["cmd"], b["gid"], b["sc"], b["st"], kw, sched)
    ct, cm = run(device, clean, kw_c, sched_c)
    dt_, dm = run(device, dirty, kw_d, sched_d)
    twin, tmask = run(lambda *a: tec.twin(kernel, *a), dirty, kw_d, sched_d)
    bad = np.zeros(n, bool)
    bad[where] = True
    nan = np.isnan(dt_[:, where]).sum(0)
    print("GAIT-EDGE unresolved %s on the device: NaN rows per instance %s, masks %s" % (kernel, nan.tolist(), dm[where].tolist()))
    assert np.isfinite(ct).all() and set(nan.tolist()) <= {0, 54}
    assert np.array_equal(nan == 54, lost) and (dm[where][lost] == 0xF).all() and np.isfinite(dt_[:, where][:, ~lost]).all()
    assert np.array_equal(np.isnan(twin), np.isnan(dt_)) and (tmask == dm).all()
    assert pe.same_bits(dt_[:, ~bad], ct[:, ~bad]) and (dm[~bad] == cm[~bad]).all()


def test_feedback_on_exact_lift_offs_and_exact_u_hold():
    """gait_edges.feedback_ties(): the DYADIC stride, dt = 2^-5 s, 64 calls of wbc_gait_targets_measured, n = 17, u_hold = 0.5, dyadic
    gains and d_max; ticks fall exactly on lift-offs and touch-downs and on u == u_hold, and two instances' raw offset has |d_raw| == d_max
    exactly.  The device equals the host twin bit for bit in rows, offsets, state and previous mask, and on the two exact instances it
    equals gait_feedback_oracle.step, nothing left out: `u <= u_hold` takes, and g = min(1, d_max / m) = 1."""
    c = ge.feedback_ties()
    n, ticks = c["sc"].shape[0], c["times"].shape[0]
    ld = n + 3
    w = lambda a: pe.wide(a, ld, fill=np.nan)
    g = RawFeedbackGait([ge.DYADIC], c["P"], n, c["par"], ld, w(c["cmd"]), None, w(c["sc"]))
    plain, pmask = g.plain(n, w(c["times"]))
    q, v = zip(*(tfc.measured(plain[k][:, :n], c["dq"][k], c["dv"][k]) for k in range(ticks)))
    rows, gmask, offs = g.measured(n, w(c["times"]), w(np.stack(q)), w(np.stack(v)))
    state, prev = g.state(n)
    g.close()
    assert (rows[:, :, n:] == 7.5).all() and (offs[:, :, n:] == 7.5).all() and (gmask[:, n:] == 0x55).all() and (gmask[:, :n] == pmask[:, :n]).all()
    cut = lambda a: [np.ascontiguousarray(x[..., :n]) for x in a]
    tec.feedback_ties_check(c, cut(rows), cut(offs), state, prev, cut(plain), cut(pmask), q, v)
