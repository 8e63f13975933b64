"""The gait planner at the ties of its law (include/wbc_gait.h), no GPU: the edge batches of tests/gait_edges.py through the host
instantiations of csrc/wbc_gait.hpp (tests/host_gait.py, host_gait_terrain.py, host_gait_schedule.py) against the numpy oracles in
double and in extended precision.  Nothing is drawn again for lying on a decision, and no sample is left out.  The header fixes the
clock operation by operation, so on the boundaries batch the mask of the double oracle is the answer, to the bit, and the
extended-precision oracle's differs wherever a rounding decides: the batch must keep at least 3 % of such samples, or it checks
nothing that the other gait tests do not.  Legal instances whose clock does not resolve in double are malformed as a whole.
tests/test_gait_edges_gpu.py runs the same batches on the device; measured figures: profiles/r17/gait_edges.md."""
import numpy as np
import pytest

import gait_edges as ge
import gait_oracle as go
import gait_schedule_oracle as gso
import gait_terrain_oracle as gto
import host_gait as hg
import host_gait_schedule as hgs
import host_gait_terrain as hgt
import test_gait_cpu as tgc
import test_gait_terrain_cpu as tgt
from quadruped_drake_amd import gait
from test_gait_gpu import SIXTEEN

KERNELS = ["plain", "terrain", "schedule", "schedule_terrain"]
S16 = tuple((tuple(d), tuple(m)) for d, m in (gait.stride(s) for s in SIXTEEN))


def groups(kernel):
    return tgt.GROUPS if "terrain" in kernel else tgc.GROUPS


def twin(kernel, strides, P, time, cmd, gid, sc, st, kw=None, sched=None, blend=ge.BLEND):
    """the host instantiation of the target kernel `kernel` -> (targets [54, n], mask [n])"""
    if sched is not None:
        return hgs.run(strides, time, cmd, sched[0], sched[1], sched[2], blend, gid, sc, st, p=P, **(kw or {}))
    if kw:
        return hgt.run(strides, kw["profiles"], time, cmd, gid, sc, st, kw["terrain_id"], kw["terrain_scale"], tp=kw["tp"], p=P)
    return hg.run(strides, time, cmd, gid, sc, st, p=P)


def oracle(kernel, strides, P, time, cmd, gid, sc, st, kw=None, sched=None, blend=ge.BLEND, dtype=np.float64, info=None):
    """the numpy oracle of the target kernel `kernel` -> (targets [54, n], mask [n])"""
    S = [gait.stride(s) for s in strides]
    if sched is not None:
        return gso.targets(P, S, time, cmd, sched[0], sched[1], sched[2], blend, gid, sc, st, dtype=dtype, info=info, **(kw or {}))
    if kw:
        return gto.targets(P, S, kw["tp"], kw["profiles"], time, cmd, gid, sc, st, kw["terrain_id"], kw["terrain_scale"], dtype=dtype, info=info)
    return go.targets(P, S, time, cmd, gid, sc, st, dtype=dtype)


def case_twin(c):
    b = c["b"]
    return twin(None, SIXTEEN, c["P"], b["time"], c["cmd"], b["gid"], b["sc"], c["st"], c["kw"], c["sched"])


def check_rows(label, got, want, c, kernel):
    """got against want below gait_edges.bars(): per row group and per stride number; prints the worst ratio per group"""
    b = c["b"]
    bar, wst = ge.bars(c["o64"], c["o80"], b["k"], groups(kernel)), ge.worst(got, want, b["k"], groups(kernel))
    for name, _ in groups(kernel):
        keys = [key for key in bar if key[0] == name]
        top = max(keys, key=lambda key: wst[key] / bar[key] if bar[key] > 0 else (0.0 if wst[key] == 0 else np.inf))
        print("GAIT-EDGE %s %-14s worst %.3g against its bar %.3g (k = %d); bars %.3g .. %.3g" %
              (label, name, wst[top], bar[top], top[1], min(bar[key] for key in keys), max(bar[key] for key in keys)))
    for key in bar:
        assert wst[key] < bar[key] or (bar[key] == 0 and wst[key] == 0), (label, key, wst[key], bar[key])


def test_the_edge_handles_are_the_planners():
    for ramp, wait in ((0.5, 0.0), (0.0, 0.25)):
        a, b = ge.params(ramp, wait), hg.params(ramp_time=ramp, wait_time=wait)
        assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert ge.EIGHT == SIXTEEN[12] and ge.MAX_GRADE == tgt.MAX_GRADE and ge.NEAR == tgt.NEAR


@pytest.mark.parametrize("wait", [0.0, 0.25])
@pytest.mark.parametrize("kernel", KERNELS)
def test_exact_boundaries_on_every_host_twin(kernel, wait):
    """The boundaries batch, every sample: twin mask == oracle64 mask; rows twin to oracle64 below the bars; the times are the batch's
    (only commands, starts and schedules were drawn again for the clearances of the terrain and the schedule laws).  On the plain
    twin: at least 3 % of the samples are decided by the header's rounding rule (the two oracles' masks differ there); and with
    wait_time = 0 the batch's tau is the kernel's and every exact lift-off has z and z-rate exactly 0."""
    c = ge.case(S16, kernel, wait)
    b = c["b"]
    n = b["time"].shape[0]
    assert n % 16 != 0 and n > 10000 and sorted(set(b["gid"])) == list(range(16))
    assert np.array_equal(b["time"], ge.boundaries(S16, wait)["time"]) and (b["time"] - wait >= 0).all()
    got, gmask = case_twin(c)
    decided = c["m64"] != c["m80"]
    print("GAIT-EDGE boundaries %s wait %.2f: %d samples, %d decided by a rounding (%.1f %%), %d instances drawn again, times changed 0" %
          (kernel, wait, n, decided.sum(), 100.0 * decided.mean(), c["redrawn"]))
    assert (gmask == c["m64"]).all() and np.isfinite(got).all() and np.isfinite(c["o64"]).all()
    if kernel == "plain":
        assert decided.mean() >= 0.03
    if c["room"] is not None:
        th = go.theta(c["P"]["ramp_time"], b["time"] - wait)[0]
        before = ((c["sched"][1][:2] <= th) & (np.arange(2)[:, None] < c["sched"][0])).sum(0)
        print("GAIT-EDGE boundaries %s wait %.2f: %d of %d instances have two switches before their time" % (kernel, wait, c["room"].sum(), n))
        assert (before[c["room"]] == 2).all() and (th[~c["room"]] < 2 * ge.BLEND + 0.02).all() and c["room"].mean() > 0.9
    check_rows("boundaries %s wait %.2f twin-to-oracle64" % (kernel, wait), got, c["o64"], c, kernel)
    if wait == 0.0:
        assert np.array_equal(b["time"], b["tau"])
        if "terrain" not in kernel:
            lifts = 0
            for f in range(4):
                at = b["lift"][f]
                lifts += int(at.sum())
                assert (got[18 + 9 * f + 2, at] == 0.0).all() and (got[18 + 9 * f + 5, at] == 0.0).all(), f
            assert lifts > 1000


def small_batches():
    """[(label, strides, P, batch)] of clock_start, ramp_end and sinc_edge"""
    first = [s for s in SIXTEEN if gait.stride(s)[1][0] != 0xF] + ["pronk"]
    assert all(x in first for x in ("pace", "trot", SIXTEEN[13])) and len(first) >= 8
    three = ["trot", "walk", "pace"]
    out = [("clock_start wait %.2f" % w, first, ge.params(wait_time=w), ge.clock_start(first, w)) for w in (0.0, 0.25)]
    out += [("ramp_end ramp %.1f" % r, three, ge.params(ramp_time=r), ge.ramp_end(len(three), r)) for r in (0.0, 0.5)]
    out += [("sinc_edge", ["trot"], ge.params(ramp_time=0.0), ge.sinc_edge())]
    return out


def check_small(label, strides, P, b, got, gmask, want, wmask, o64, m64, o80):
    """what every engine owes on a small batch: the double oracle's mask, finite rows, rows below 100 x |oracle64 - oracle80| per row
    group over the batch; the standing rows before the wait and phase 0 from tau = 0 on"""
    n = b["time"].shape[0]
    assert n % 16 != 0 and (gmask == wmask).all() and (wmask == m64).all() and np.isfinite(got).all()
    for name, rows in tgc.GROUPS:
        bar = 100.0 * float(np.abs(o64[rows] - o80[rows]).max())
        worst = float(np.abs(got[rows] - want[rows]).max())
        print("GAIT-EDGE %s %-13s worst %.3g bar %.3g" % (label, name, worst, bar))
        assert worst < bar or (bar == 0 and worst == 0), (label, name, worst, bar)
    if "before" in b:
        pre = b["before"]
        assert pre.any() and (~pre).any() and (gmask[pre] == 0xF).all()
        phase0 = np.array([gait.stride(s)[1][0] for s in strides])[b["gid"]]
        assert (gmask[~pre] == phase0[~pre]).all()                                   # tau = 0, 5e-324, ulp: phase 0, not the standing branch
        feet = [18 + 9 * f + r for f in range(4) for r in range(2, 9)]
        assert (got[feet][:, pre] == 0.0).all() and (got[tgc.VEL + tgc.ACC][:, pre] == 0.0).all()
        assert (got[0:2, pre] == b["st"][0:2, pre]).all() and (got[11, pre] == b["st"][2, pre]).all() and (got[2, pre] == P["height"]).all()


@pytest.mark.parametrize("scheduled", [False, True], ids=["plain", "schedule"])
def test_clock_start_ramp_end_and_sinc_edge_on_the_host_twins(scheduled):
    for label, strides, P, b in small_batches():
        sched = ge.schedule_for(P, b) if scheduled else None
        args = (strides, P, b["time"], b["cmd"], b["gid"], b["sc"], b["st"], None, sched)
        info = {}
        o80, _ = oracle(None, *args, dtype=np.longdouble, info=info)
        o64, m64 = oracle(None, *args)
        assert not scheduled or float(info["near"].min()) >= ge.NEAR
        got, gmask = twin(None, *args)
        check_small(label + (" schedule" if scheduled else " plain"), strides, P, b, got, gmask, o64, m64, o64, m64, o80)


def unresolved_case():
    """gait_edges.unresolved() on walk, stand and the eight-phase stride -> (strides, P, batch, lost [n]: the header's verdict)"""
    strides = ["walk", "stand", ge.EIGHT]
    P = ge.params()
    b = ge.unresolved(len(strides))
    lost = np.zeros(b["time"].shape[0], bool)
    for g, s in enumerate(strides):
        d, m = gait.stride(s)
        sel = b["gid"] == g
        lost[sel] = go.unresolved(d, m, b["time"][sel] - P["wait_time"], b["sc"][sel])
    return strides, P, b, lost


def unresolved_inputs(kernel, b, P):
    kw = ge.terrain_kw(b["gid"]) if "terrain" in kernel else None
    sched = ge.schedule_for(P, b) if "schedule" in kernel else None
    return kw, sched


@pytest.mark.parametrize("kernel", KERNELS)
def test_unresolved_clocks_are_malformed_not_half_nan_on_the_host_twins(kernel):
    """Every instance of unresolved(): all 54 rows finite, or all 54 NaN with mask 0xF; which of the two is the oracle's verdict, and
    the oracle's is the header's sentence (go.unresolved).  A foot that is always in contact has no run: `stand` is malformed only
    where T itself is lost, and the eight-phase stride's three standing feet decide nothing."""
    strides, P, b, lost = unresolved_case()
    kw, sched = unresolved_inputs(kernel, b, P)
    args = (strides, P, b["time"], b["cmd"], b["gid"], b["sc"], b["st"], kw, sched)
    got, gmask = twin(kernel, *args)
    with np.errstate(all="ignore"):                    # the oracle evaluates every run of a stride and selects: the unused ones overflow here
        want, wmask = oracle(kernel, *args)
    nan = np.isnan(got).sum(0)
    print("GAIT-EDGE unresolved %s: NaN rows per instance %s, masks %s" % (kernel, nan.tolist(), gmask.tolist()))
    assert set(nan.tolist()) <= {0, 54} and np.isfinite(got[:, nan == 0]).all() and (gmask[nan == 54] == 0xF).all()
    assert np.array_equal(nan == 54, np.isnan(want).all(0)) and np.array_equal(nan == 54, lost) and (gmask == wmask).all()
    table = {(g, i): bool(lost[g * len(ge.UNRESOLVED) + i]) for g in range(3) for i in range(len(ge.UNRESOLVED))}
    assert all(table[(0, i)] == (i < 6 or i == 9) for i in range(11))                # walk: T = 2 s overflows at scale 1e308 as well
    assert all(table[(1, i)] == (i in (0, 1, 5)) for i in range(11))                 # stand: no run; T underflows, or k T overflows
    assert all(table[(2, i)] == (i < 6) for i in range(11))                          # eight phases, one foot with runs


def feedback_ties_check(c, rows, offs, state, prev, plain, pmask, q, v):
    """What any engine owes on gait_edges.feedback_ties(): rows [ticks, 54, n], offsets [ticks, 8, n], the state [6, 4 n] and the previous
    masks [n] after the last tick equal the host twin's bit for bit; and for the two exact instances they equal the double oracle's,
    nothing left out -- where the oracle's decisions are the law's at the exact hits: a foot in the air with u == u_hold takes, the
    clamp does not bind at |d_raw| == d_max (g = 1), and `to` holds (3, 4) 2^-7 from the hit on."""
    import gait_feedback_oracle as gfo
    import plant_edges as pe
    import test_gait_feedback_cpu as tfc
    P, par, n, ex = c["P"], c["par"], c["sc"].shape[0], c["exact"]
    ticks = c["times"].shape[0]
    eng = [tfc.Twin(n), tfc.Oracle(n)]
    hits = lifts = 0
    for k in range(ticks):
        a = (c["times"][k], q[k], v[k], plain[k], pmask[k], None, c["sc"])
        (rt, ot), (rd, od) = (e.step(par, P, [ge.DYADIC], *a) for e in eng)
        assert pe.same_bits(rows[k], rt) and pe.same_bits(offs[k], ot), k
        feet = sum((r for _, r in tfc.GROUPS), [])
        assert (rows[k][feet][:, ex] == rd[feet][:, ex]).all() and (offs[k][:, ex] == od[:, ex]).all(), k
        dec = eng[1].decisions
        assert not dec[ex, 0].any() and not eng[1].skipped.any()                         # |d_raw| == d_max does not bind: g = 1
        for i in ex:
            up = ~dec[i, 5:9].astype(bool)
            lifts += int(c["edge"][k, i])
            if c["hold"][k, i]:                                                          # u == u_hold on the feet in the air: taken, with this tick's offset
                hits += 1
                assert up.any() and dec[i, 1:5][up].all()
                to = eng[1].st.to[:, :, i]
                assert (to[up] == np.array([3.0, 4.0]) * 2.0 ** -7).all(), (k, i)
    st, pv = eng[0].packed()
    assert pe.same_bits(state, st) and (prev == pv).all()
    sel = np.repeat(np.isin(np.arange(n), ex), 4)
    assert (state[:, sel] == eng[1].packed()[0][:, sel]).all()
    # after a swing's middle the next ticks offer (d_max, 0): a foot that landed since holds what it took at u == u_hold, exactly
    landed = np.abs(eng[1].st.cur[:, :, ex])
    assert set(np.unique(landed).tolist()) <= {0.0, 3.0 * 2.0 ** -7, 4.0 * 2.0 ** -7} and landed.max() > 0
    print("GAIT-EDGE feedback ties: %d ticks x %d instances equal the twin bit for bit; %d exact u == u_hold hits and %d exact edges on the "
          "two exact instances equal the oracle" % (ticks, n, hits, lifts))
    assert hits >= 8 and lifts >= 16


def test_feedback_on_exact_lift_offs_and_exact_u_hold_on_the_host_twin():
    import test_gait_feedback_cpu as tfc
    c = ge.feedback_ties()
    n, ticks = c["sc"].shape[0], c["times"].shape[0]
    plain, pmask, q, v = [], [], [], []
    for k in range(ticks):
        tg, mk = hg.run([ge.DYADIC], c["times"][k], c["cmd"], None, c["sc"], None, p=c["P"])
        qk, vk = tfc.measured(tg, c["dq"][k], c["dv"][k])
        plain.append(tg); pmask.append(mk); q.append(qk); v.append(vk)
    twin = tfc.Twin(n)
    rows, offs = zip(*(twin.step(c["par"], c["P"], [ge.DYADIC], c["times"][k], q[k], v[k], plain[k], pmask[k], None, c["sc"]) for k in range(ticks)))
    state, prev = twin.packed()
    assert ge.DYADIC == tgc.DYADIC
    feedback_ties_check(c, rows, offs, state, prev, plain, pmask, q, v)
