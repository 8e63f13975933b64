"""The kernels that feed and drain the tick on the MI355X at the edges of their laws: traj_lookup_kernel, robot_states_unpack_kernel,
robot_controls_pack_kernel and pd_step_kernel (csrc/wbc_traj.hip), wbc_integrate_kernel and the persistent rollout's lookup and clock
(csrc/wbc_kernels.hip) on the batches of tests/caller_edges.py, through the C ABI with ld = n + 5 -- the Python wrappers always pass
ld = n.  Inputs' padding holds NaN (bytes: 0xA5), outputs' and in-place arrays' the sentinels of tests/plant_edges.py, and every test
asserts that the padding came back as it was.  References: oracle/traj_oracle.py, checked on the same batches without a GPU in
tests/test_caller_edges_cpu.py.  What is asserted is what the headers claim: the lookup is numpy's argmin for every double (wbc.h),
the codec writes struct.pack's bytes and +-inf past FLT_MAX, the PD law is np.clip bit for bit, NaN included (wbc_extras.h), and the
persistent rollout equals the launch-per-stage loop bit for bit with a NaN and an infinite clock in the batch.  Each test prints its
figures on CALLER-EDGE lines; profiles/r18/caller_edges.md records them."""
import ctypes as C

import numpy as np
import pytest

import caller_edges as ce
import plant_edges as pe
from oracle import traj_oracle as to
from test_pd import gold
from test_rollout import _trot_trajectory

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = ce.PAD


def _t(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), device=DEV)


def _h(x):
    return x.cpu().numpy()


def _ptr(x):
    return None if x is None else C.c_void_p(x.data_ptr())


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream(0).cuda_stream)


def _sync():
    import torch
    torch.cuda.synchronize()


def _L():
    from quadruped_drake_amd import _lib
    return _lib.lib()


def _check(rc):
    from quadruped_drake_amd import _lib
    _lib.check(rc)


def _preset(rows, ld, dtype=np.float64):
    """An output array of ld columns that holds the dtype's sentinel everywhere"""
    return _t(np.full((rows, ld) if rows else (ld,), pe.sentinel(dtype), dtype))


def _ints(p):
    return None if p is None else (C.c_int * 12)(*[int(x) for x in p])


def _perms():
    _, order, act, _, _ = gold("pd_perm")
    return {"identity": (list(range(12)), list(range(12))), "pd_perm": (order, act)}


def _same_nan_aside(a, b):
    """Bit for bit where b is a number, a NaN exactly where b is one"""
    nan = np.isnan(b)
    return np.array_equal(np.isnan(a), nan) and pe.same_bits(a[~nan], b[~nan])


# =============================================================== lookup
def _trajectory(ts, wait):
    from quadruped_drake_amd.trajectory import TrunkTrajectory
    tg, mk, st = ce.table_rows(ts.size)
    return TrunkTrajectory(ts, tg, mk, wait_time=wait, device=0, standing_targets=st, standing_mask=ce.STANDING_MASK)


def _lookup(traj, t):
    """wbc_traj_lookup on n = len(t) times in arrays of n + PAD columns -> (targets [54, n], mask [n]); the padding is checked here"""
    n = t.shape[0]
    ld = n + PAD
    time = _t(pe.wide(t, ld, fill=np.nan))
    tg, mk = _preset(54, ld), _preset(0, ld, np.uint8)
    _check(traj._L.wbc_traj_lookup(traj._h, _stream(), n, ld, _ptr(time), _ptr(tg), _ptr(mk)))
    _sync()
    tg, mk = _h(tg), _h(mk)
    assert pe.padding_kept(tg, n) and pe.padding_kept(mk, n) and pe.same_bits(_h(time), pe.wide(t, ld, fill=np.nan))
    return tg[:, :n], mk[:n]


@pytest.mark.parametrize("name", list(ce.tables()))
def test_lookup_is_numpy_argmin_on_every_table_and_time(name):
    """Targets and masks bit-equal to traj_oracle.lookup on every query of the table under the three waits: ties, roundings, both
    ends, the wait and its neighbours, NaN, +-inf and the huge finite times."""
    for wait in ce.WAITS:
        ts, t, idx, out, m = ce.lookup_case(name, wait)
        traj = _trajectory(ts, wait)
        tg, mk = _lookup(traj, t)
        traj.close()
        got = np.where(tg[0] < 0, -1, tg[0] / 64.0).astype(np.int64)
        bad = got != idx
        kinds = {"nan": np.isnan(t), "inf": np.isinf(t), "huge": np.isfinite(t) & (np.abs(t) >= 2.0 ** 53)}
        print("CALLER-EDGE lookup %-12s wait %5.2f K %4d: %5d times, index differs from numpy on %d (nan %d, inf %d, huge %d, other %d)"
              % (name, wait, ts.size, t.size, bad.sum(), (bad & kinds["nan"]).sum(), (bad & kinds["inf"]).sum(), (bad & kinds["huge"]).sum(),
                 (bad & ~kinds["nan"] & ~kinds["inf"] & ~kinds["huge"]).sum()))
        assert not bad.any(), (wait, t[bad][:8], got[bad][:8], idx[bad][:8])
        assert pe.same_bits(tg, out) and np.array_equal(mk, m)


@pytest.mark.parametrize("n", ce.NS)
def test_lookup_at_the_tails_of_its_blocks(n):
    """n times drawn from the geometric table's queries (wait 0.5), NaN, +inf and 1e300 always among them: the tails of the 64-thread
    blocks with ld = n + 5."""
    ts, t, idx, out, m = ce.lookup_case("geometric", 0.5)
    special = np.flatnonzero(np.isnan(t) | np.isinf(t) | (t == 1e300))
    pick = np.concatenate([special, np.random.default_rng(n).permutation(t.size)])[:n]
    if n > 1:
        pick[-1] = special[0]                                    # the NaN on the last column of the batch
    traj = _trajectory(ts, 0.5)
    tg, mk = _lookup(traj, t[pick])
    traj.close()
    print("CALLER-EDGE lookup tails n %3d: rows differ on %d columns" % (n, (tg != out[:, pick]).any(0).sum()))
    assert pe.same_bits(tg, np.ascontiguousarray(out[:, pick])) and np.array_equal(mk, m[pick])


# =============================================================== wire format
@pytest.mark.parametrize("n", ce.NS)
def test_unpack_every_float32_word_in_every_field(n):
    """Bit-equal to traj_oracle.robot_state_decode on the decoded columns (denormals, +-0, +-FLT_MAX, +-inf kept; NaN as NaN), ok exact,
    columns of the messages with a foreign fingerprint (columns 0, 63, 64, n - 1, each wrong in another byte) left as preset, with
    ok and with ok = NULL."""
    raw, good = ce.state_messages(n)
    want_q, want_v = ce.decoded_states(raw, good)
    ld = n + PAD
    msgs = _t(np.frombuffer(raw + b"\xA5" * (PAD * 204), np.uint8))
    for with_ok in (True, False):
        q, v, ok = _preset(19, ld), _preset(18, ld), _preset(0, ld, np.uint8)
        _check(_L().wbc_robot_states_unpack(0, _stream(), n, ld, _ptr(msgs), _ptr(q), _ptr(v), _ptr(ok) if with_ok else None))
        _sync()
        q, v, ok = _h(q), _h(v), _h(ok)
        assert pe.padding_kept(q, n) and pe.padding_kept(v, n) and pe.padding_kept(ok, n if with_ok else 0)
        assert pe.padding_kept(q[:, :n][:, ~good], 0) and pe.padding_kept(v[:, :n][:, ~good], 0)
        assert not with_ok or np.array_equal(ok[:n], good.astype(np.uint8))
        gq, gv = q[:, :n][:, good], v[:, :n][:, good]
        wrong = int((np.isnan(gq) != np.isnan(want_q[:, good])).sum() + (np.isnan(gv) != np.isnan(want_v[:, good])).sum()
                    + (pe.bits(gq) != pe.bits(want_q[:, good]))[~np.isnan(gq)].sum() + (pe.bits(gv) != pe.bits(want_v[:, good]))[~np.isnan(gv)].sum())
        print("CALLER-EDGE unpack n %3d ok %-4s: %d rejected, %d of %d decoded words differ" % (n, "set" if with_ok else "NULL", (~good).sum(), wrong, gq.size + gv.size))
        assert _same_nan_aside(gq, want_q[:, good]) and _same_nan_aside(gv, want_v[:, good])
    assert _h(msgs).tobytes() == raw + b"\xA5" * (PAD * 204)


@pytest.mark.parametrize("n", ce.NS)
def test_pack_rounds_like_struct_pack_and_writes_inf_past_flt_max(n):
    """The messages equal struct.pack's under both numberings: halfway points to even, float32 denormals kept, the largest double that
    rounds to FLT_MAX, +-inf; NaN is a NaN; a double past FLT_MAX, where struct.pack raises, is +-inf (wbc_extras.h).  Fingerprint
    and the 37 zero words included; the bytes after message n - 1 are untouched."""
    ld = n + PAD
    tau = ce.control_torques(n)
    for label, (order, act) in _perms().items():
        words, nan = ce.control_messages(tau, order, act)
        msgs, tau_d = _t(np.full((n + PAD) * 204, pe.SENT_U8, np.uint8)), _t(pe.wide(tau, ld, fill=np.nan))
        _check(_L().wbc_robot_controls_pack(0, _stream(), n, ld, _ptr(tau_d), _ints(order), _ints(act), _ptr(msgs)))
        _sync()
        raw = _h(msgs).tobytes()
        got = np.frombuffer(raw[:n * 204], dtype=">u4").reshape(n, 51).astype(np.uint32)
        gnan = ((got & 0x7F800000) == 0x7F800000) & ((got & 0x007FFFFF) != 0)
        gnan[:, :39] = False
        diff = (got != words) & ~(nan & gnan)
        inf = (words[:, 39:] & 0x7FFFFFFF) == 0x7F800000
        den = ((words[:, 39:] & 0x7F800000) == 0) & ((words[:, 39:] & 0x007FFFFF) != 0)
        print("CALLER-EDGE pack n %3d %-8s: %d of %d words differ (of %d denormal words %d, of %d infinite words %d), NaN where expected: %s"
              % (n, label, diff.sum(), got.size, den.sum(), (diff[:, 39:] & den).sum(), inf.sum(), (diff[:, 39:] & inf).sum(), np.array_equal(gnan, nan)))
        assert np.array_equal(gnan, nan) and not diff.any()
        assert (got[:, 2:39] == 0).all() and raw[n * 204:] == bytes([pe.SENT_U8]) * (PAD * 204)


# =============================================================== PD
@pytest.mark.parametrize("gains", list(ce.PD_GAINS))
def test_pd_is_np_clip_bit_for_bit_and_keeps_nan(gains):
    """tau.tobytes() == pd_control_law(...).tobytes() on the entries that are numbers, NaN exactly where the oracle has NaN -- a NaN
    joint angle or rate is a NaN torque, never a saturated one; u on and one ulp either side of +-u_max, overflowing products, the
    signed zeros of np.clip at u_max = 0; both numberings, every batch tail.  NaN base rows do not matter."""
    g = ce.PD_GAINS[gains]
    qn = None if g["q_nom"] is None else np.ascontiguousarray(g["q_nom"], np.float64)
    for label, (order, act) in _perms().items():
        for n in ce.NS:
            ld = n + PAD
            q, v, which, names = ce.pd_batch(n, gains, order, act)
            want = ce.pd_oracle(q, v, gains, order, act)
            tau, q_d, v_d = _preset(12, ld), _t(pe.wide(q, ld, fill=np.nan)), _t(pe.wide(v, ld, fill=np.nan))
            _check(_L().wbc_pd_step(0, _stream(), n, ld, _ptr(q_d), _ptr(v_d),
                                    None if qn is None else qn.ctypes.data_as(C.POINTER(C.c_double)), g["kp"], g["kd"], g["u_max"],
                                    _ints(order), _ints(act), _ptr(tau)))
            _sync()
            tau = _h(tau)
            assert pe.padding_kept(tau, n)
            got = tau[:, :n]
            nan_lost = np.isnan(want) & ~np.isnan(got)
            differ = ~np.isnan(want) & (np.isnan(got) | (pe.bits(got) != pe.bits(want)))
            rows = sorted({names[k] for k in which[nan_lost | differ]})
            print("CALLER-EDGE pd %-8s %-8s n %3d: %d NaN of the oracle answered with a number (%s), %d other entries differ %s"
                  % (gains, label, n, nan_lost.sum(), sorted(set(np.abs(got[nan_lost]).tolist())), differ.sum(), rows))
            assert not nan_lost.any() and not differ.any(), rows
            assert got[~np.isnan(want)].tobytes() == want[~np.isnan(want)].tobytes() and np.array_equal(np.isnan(got), np.isnan(want))


# =============================================================== integrate and the rollout's clock
@pytest.mark.parametrize("dt", [5e-3, 0.0])
def test_integrate_at_the_branches_of_the_quaternion_step(dt):
    """wbc_integrate against to.integrate at atol = 1e-14 (the bar of tests/test_rollout.py) on every kind but the large angles; those
    (|w| dt / 2 near 1e3, |w| = 4e5) against the np.longdouble restatement at ten times the oracle64-to-oracle80 gap of the same
    columns (measured on this batch: gap 2.9e-11, the rounding of a rate of 4e5 to 2^-34 -- which is why 1e-14 cannot hold there).
    At dt = 0 every angle is zero and the 1e-14 bar holds on all kinds."""
    from quadruped_drake_amd import IDController
    ctrl = IDController(max_batch=272, device=0)
    for n in ce.NS:
        ld = n + PAD
        q0, v0, vd, kind = ce.integrate_batch(n, dt, seed=n)
        q, v, vd_d = _t(pe.wide(q0, ld)), _t(pe.wide(v0, ld)), _t(pe.wide(vd, ld, fill=np.nan))
        ctrl._bind_stream()
        _check(ctrl._L.wbc_integrate(ctrl._h, n, ld, float(dt), _ptr(q), _ptr(v), _ptr(vd_d)))
        ctrl.sync()
        q, v = _h(q), _h(v)
        assert pe.padding_kept(q, n) and pe.padding_kept(v, n)
        q, v = q[:, :n], v[:, :n]
        q64, v64 = to.integrate(q0, v0, vd, dt)
        large = (kind == 3) & (dt > 0)
        err = np.maximum(np.abs(q - q64).max(0), np.abs(v - v64).max(0))
        fig = {nm: float(err[kind == k].max()) for k, nm in enumerate(ce.INTEGRATE_KINDS) if (kind == k).any()}
        print("CALLER-EDGE integrate dt %g n %3d against oracle64: %s" % (dt, n, " ".join("%s %.3g" % kv for kv in fig.items())))
        assert np.isfinite(q).all() and np.isfinite(v).all()
        assert (err[~large] <= 1e-14).all(), fig
        if large.any():
            q80, v80 = ce.integrate_ld(q0, v0, vd, dt)
            gap = float(max(np.abs(q64 - q80)[:, large].max(), np.abs(v64 - v80)[:, large].max()))
            dev = float(max(np.abs(q - q80)[:, large].max(), np.abs(v - v80)[:, large].max()))
            print("CALLER-EDGE integrate dt %g n %3d large angles: device - oracle80 %.3g, oracle64 - oracle80 %.3g, bar %.3g" % (dt, n, dev, gap, 10.0 * gap))
            assert dev <= 10.0 * gap
    ctrl.close()


def test_rollout_equals_the_stage_loop_with_a_nan_and_an_infinite_clock():
    """n = 9, 40 ticks, the ID law on the 16-lane kernel, robot 3 with time = NaN and robot 6 with time = +inf: wbc_rollout and the loop
    wbc_traj_lookup / wbc_step / wbc_integrate / time += dt agree bit for bit in targets, mask, q, v, tau and status; the two malformed
    clocks get numpy's sample -- index 0 -- on both paths (the persistent kernel starts its search from K / 2 and then from the last
    index, the lookup kernel from an even-spacing guess: the hint must not show); ld = n + 5, and time[n:] and every other padding is
    as preset.  (wbc_advance_time_kernel is launched by no entry point: the clock is checked through the rollout.)"""
    import torch
    from quadruped_drake_amd import IDController, workloads
    from quadruped_drake_amd.trajectory import TrunkTrajectory
    n, steps, dt = 9, 40, 1e-3
    ld = n + PAD
    ts, tg, masks, st_t = _trot_trajectory(K=200)
    masks[:] = 0b1111
    masks[0] = 0b0111                                   # sample 0 is recognisable by its mask as well
    traj = TrunkTrajectory(ts, tg, masks, wait_time=0.01, device=0, standing_targets=st_t, standing_mask=0b1111)
    q0, v0 = workloads.nominal_state("mini_cheetah", n)
    t0 = np.linspace(0.0, 0.05, n)
    t0[3], t0[6] = np.nan, np.inf
    L = _L()

    def arrays():
        return dict(q=_t(pe.wide(q0, ld)), v=_t(pe.wide(v0, ld)), time=_t(pe.wide(t0, ld)), tg=_preset(54, ld), mk=_preset(0, ld, np.uint8),
                    tau=_preset(12, ld), met=_preset(4, ld), st=_preset(0, ld, np.int32), vd=_preset(18, ld))

    a = arrays()
    ca = IDController(max_batch=16, device=0); ca.set_variant("hex")
    ca._bind_stream()
    _check(L.wbc_rollout(ca._h, traj._h, steps, float(dt), n, ld, _ptr(a["q"]), _ptr(a["v"]), _ptr(a["time"]), _ptr(a["tg"]), _ptr(a["mk"]), None, None,
                         _ptr(a["tau"]), _ptr(a["met"]), _ptr(a["st"]), _ptr(a["vd"])))
    ca.sync()
    b = arrays()
    cb = IDController(max_batch=16, device=0); cb.set_variant("hex")
    cb._bind_stream()
    _check(L.wbc_set_vdot_output(cb._h, _ptr(b["vd"])))
    for _ in range(steps):
        _check(L.wbc_traj_lookup(traj._h, _stream(), n, ld, _ptr(b["time"]), _ptr(b["tg"]), _ptr(b["mk"])))
        torch.cuda.synchronize()
        _check(L.wbc_step(cb._h, n, ld, _ptr(b["q"]), _ptr(b["v"]), _ptr(b["tg"]), _ptr(b["mk"]), None, None, _ptr(b["tau"]), _ptr(b["met"]), _ptr(b["st"])))
        _check(L.wbc_integrate(cb._h, n, ld, float(dt), _ptr(b["q"]), _ptr(b["v"]), _ptr(b["vd"])))
        cb.sync()
        b["time"][:n] += dt
    _check(L.wbc_set_vdot_output(cb._h, None))
    a = {k: _h(x) for k, x in a.items()}
    b = {k: _h(x) for k, x in b.items()}
    ca.close(); cb.close(); traj.close()
    differ = {k: int((pe.bits(a[k][..., :n]) != pe.bits(b[k][..., :n])).sum()) for k in ("tg", "mk", "q", "v", "tau", "st", "met", "vd")}
    first = {"rollout": [int(a["mk"][i]) for i in (3, 6)], "loop": [int(b["mk"][i]) for i in (3, 6)]}
    print("CALLER-EDGE rollout against the stage loop, NaN and +inf clocks: entries that differ %s; masks of robots 3 and 6 %s (sample 0: %d)" % (differ, first, masks[0]))
    for x in (a, b):
        for k, arr in x.items():
            assert pe.padding_kept(arr, n), k
        assert pe.same_bits(x["tg"][:, [3, 6]], np.ascontiguousarray(tg[[0, 0]].T)) and (x["mk"][[3, 6]] == masks[0]).all()
        assert np.isfinite(x["q"][:, :n]).all() and np.isfinite(x["v"][:, :n]).all() and np.isfinite(x["tau"][:, :n]).all()
    assert not any(differ.values()), differ
    assert np.isnan(a["time"][3]) and np.isnan(b["time"][3]) and a["time"][6] == np.inf == b["time"][6]
    keep = np.isfinite(t0)
    assert pe.same_bits(a["time"][:n][keep], b["time"][:n][keep]) and np.allclose(a["time"][:n][keep], t0[keep] + steps * dt, rtol=0, atol=1e-12)
    assert len({int(m) for m in a["mk"][:n]}) >= 2
