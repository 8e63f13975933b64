"""The Python layer's marshalling on the MI355X: every method of the package that launches a kernel gives, with its own outputs, with
the caller's `out` and through a direct call of the same entry point of libwbc_hip.so on the same tensors, the same bits; and what the
marshaller refuses never reaches the library.

n = 5: no multiple of the four robots of a tick workgroup, the tail inside one wavefront of the quad kernels.  Every optional array is
given and no two arrays hold the same values, so two pointers that changed places change the answer."""
import ctypes as C
import functools

import numpy as np
import pytest

from quadruped_drake_amd import _lib, gait, lcm_io, pd, plant, terrain, trajectory, workloads
from quadruped_drake_amd.controller import IDController

pytestmark = pytest.mark.gpu
N, DT = 5, 2e-3
F64, U8, I32 = "float64", "uint8", "int32"


def _t(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), device="cuda:0")


def _new(rows, dtype, n=N, fill=None):
    """An output tensor the test allocates itself; fill: a sentinel that a kernel which skips it leaves behind"""
    import torch
    shape = (rows, n) if rows else (n,)
    return torch.empty(shape, dtype=getattr(torch, dtype), device="cuda:0") if fill is None else \
        torch.full(shape, fill, dtype=getattr(torch, dtype), device="cuda:0")


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream(0).cuda_stream)


def _bits(tensors):
    import torch
    torch.cuda.synchronize()
    return [t.cpu().numpy().tobytes() for t in tensors]


def _alive(*tensors):
    """Some finite nonzero number in every one of them: the comparison is not one of blanks"""
    import torch
    torch.cuda.synchronize()
    for t in tensors:
        a = t.cpu().numpy().astype(np.float64)
        assert (np.isfinite(a) & (a != 0)).any()


@functools.lru_cache(maxsize=None)
def _case():
    """numpy arrays, read-only; each test uploads its own copies (steps and loops write q, v, time and counts in place)"""
    b = workloads.make_batch(5, n=N, seed=2105, model="mini_cheetah")
    rng = np.random.default_rng(2106)
    k = np.arange(N, dtype=np.float64)
    c = dict(q=b["q"], v=0.2 * b["v"], targets=b["targets"], mask=b["mask"], mu=b["mu"], ms=b["mass_scale"],
             plant_mu=0.55 + 0.07 * k, plant_ms=0.92 + 0.03 * k, wrench=rng.uniform(-3.0, 3.0, (6, N)), tau=rng.uniform(-6.0, 6.0, (12, N)),
             time=np.array([0.0, 0.04, 0.101, 0.17, 0.31]), counts=np.arange(4 * N, dtype=np.int32).reshape(4, N) + 100,
             cmd=np.stack([0.3 + 0.1 * k, -0.2 + 0.05 * k, 0.4 - 0.15 * k]), gait_id=np.array([0, 1, 0, 1, 1], np.uint8),
             stride_scale=0.8 + 0.11 * k, start=np.stack([0.5 * k, -0.25 * k, 0.2 * k - 0.3]), terrain_id=np.array([1, 0, 1, 1, 0], np.uint8),
             terrain_scale=0.6 + 0.09 * k)
    assert c["mu"] is not None and c["ms"] is not None and (c["mask"] != 15).any()
    # the nearest-sample table: four samples whose targets and masks differ
    c["ts"] = np.array([0.0, 0.1, 0.2, 0.3])
    tg = np.repeat(workloads.standing_targets("mini_cheetah", 1).T, 4, axis=0)
    tg[:, 0] += 0.01 * np.arange(4)
    tg[:, 2] -= 0.004 * np.arange(4)
    c["traj_targets"], c["traj_masks"] = tg, np.array([15, 9, 6, 15], np.uint8)
    # a standing start for the loops, every robot a little different
    q0, v0 = workloads.nominal_state("mini_cheetah", N)
    q0[4] += 0.01 * k
    q0[6] += 0.002 * k
    q0[7:] += 0.01 * rng.uniform(-1.0, 1.0, (12, N))
    c["q0"], c["v0"] = q0, v0 + 0.01 * rng.uniform(-1.0, 1.0, (18, N))
    for a in c.values():
        a.setflags(write=False)
    return c


def _traj():
    c = _case()
    return trajectory.TrunkTrajectory(c["ts"], c["traj_targets"], c["traj_masks"], wait_time=0.05, device=0)


PROFILES = [terrain.slope(0.12, start=-1.0), terrain.ramp_step(0.1, 0.03)]


def _ground():
    """-> (a GroundContactPlant on a terrain with both per-instance arrays, the arrays)"""
    c = _case()
    g = plant.GroundContactPlant(device=0)
    tid, tsc = _t(c["terrain_id"]), _t(c["terrain_scale"])
    g.set_terrain(PROFILES, tid, tsc)
    return g, (tid, tsc)


# ---- the same bits three ways
def test_controller_step_and_rollout():
    c, L = _case(), _lib.lib()
    ctrl, traj = IDController(max_batch=8, device=0), _traj()
    ins = [_t(c[k]) for k in ("q", "v", "targets", "mask", "mu", "ms")]
    fresh = ctrl.step(*ins)
    mine = tuple(_new(rows, dt, fill=9) for rows, dt, _ in _lib.TICK_OUTS)
    given = ctrl.step(*ins, out=mine)
    assert all(a is b for a, b in zip(given, mine))
    direct = tuple(_new(rows, dt, fill=9) for rows, dt, _ in _lib.TICK_OUTS)
    _lib.check(L.wbc_step(ctrl._h, N, N, *[_p(t) for t in ins], *[_p(t) for t in direct]))
    assert _bits(fresh) == _bits(given) == _bits(direct)
    _alive(fresh[0], fresh[1])
    # rollout: q, v and time move in place; vdot is what ctrl._keep[5] holds
    def state():
        return [_t(c[k]) for k in ("q0", "v0", "time")]
    s1 = state()
    tau, met, st, tg, mk = ctrl.rollout(traj, 3, DT, *s1, mu=ins[4], mass_scale=ins[5])
    r1 = _bits([tau, met, st, tg, mk, ctrl._keep[5], *s1])
    s2 = state()
    o = dict(tg=_new(54, F64), mk=_new(0, U8), tau=_new(12, F64), met=_new(4, F64), st=_new(0, I32), vd=_new(18, F64))
    _lib.check(L.wbc_rollout(ctrl._h, traj._h, 3, DT, N, N, *[_p(t) for t in s2], _p(o["tg"]), _p(o["mk"]), _p(ins[4]), _p(ins[5]),
                             _p(o["tau"]), _p(o["met"]), _p(o["st"]), _p(o["vd"])))
    r2 = _bits([o["tau"], o["met"], o["st"], o["tg"], o["mk"], o["vd"], *s2])
    assert r1 == r2 and r1[6] != _bits([_t(c["q0"])])[0]
    _alive(tau, ctrl._keep[5])
    ctrl.set_vdot_output(None)
    ctrl.close(); traj.close()


def test_rigid_plant_forward_and_step():
    c, L = _case(), _lib.lib()
    p = plant.RigidContactPlant(device=0, tau_max=5.0, mu=0.7)
    ins = [_t(c[k]) for k in ("q", "v", "tau", "mask", "plant_mu", "plant_ms")]
    fresh = p.forward(*ins)
    mine = tuple(_new(rows, dt, fill=9) for rows, dt, _ in plant._RIGID_OUTS)
    given = p.forward(*ins, out=mine)
    assert all(a is b for a, b in zip(given, mine))
    direct = tuple(_new(rows, dt, fill=9) for rows, dt, _ in plant._RIGID_OUTS)
    _lib.check(L.wbc_plant_forward(p._h, p._stream(), N, N, *[_p(t) for t in ins], *[_p(t) for t in direct]))
    assert _bits(fresh) == _bits(given) == _bits(direct)
    _alive(fresh[0], fresh[1])
    results = []
    for way in ("fresh", "out", "direct"):
        q, v, tm, cnt = (_t(c[k]) for k in ("q", "v", "time", "counts"))
        outs = tuple(_new(rows, dt, fill=9) for rows, dt, _ in plant._RIGID_OUTS)
        if way == "direct":
            _lib.check(L.wbc_plant_step(p._h, p._stream(), N, N, DT, _p(q), _p(v), _p(tm), *[_p(t) for t in ins[2:]], *[_p(t) for t in outs], _p(cnt)))
        else:
            outs = p.step(q, v, ins[2], ins[3], DT, time=tm, mu=ins[4], mass_scale=ins[5], counts=cnt, out=outs if way == "out" else None)
        results.append(_bits([*outs, q, v, tm, cnt]))
    assert results[0] == results[1] == results[2] and results[0][4] != _bits([_t(c["v"])])[0]
    p.close()


def test_ground_plant_forward_step_and_follow_targets():
    c, L = _case(), _lib.lib()
    g, keep = _ground()
    ins = [_t(c[k]) for k in ("q", "v", "tau", "plant_mu", "plant_ms", "wrench")]
    fresh = g.forward(*ins)
    direct = tuple(_new(rows, dt, fill=9) for rows, dt, _ in plant._GROUND_OUTS)
    _lib.check(L.wbc_ground_forward(g._h, g._stream(), N, N, *[_p(t) for t in ins], *[_p(t) for t in direct]))
    assert _bits(fresh) == _bits(direct) and [tuple(t.shape) for t in fresh] == [(18, N), (12, N), (N,), (N,)]
    _alive(fresh[0])
    results = []
    for way in ("fresh", "out", "direct"):
        q, v, tm, cnt = (_t(c[k]) for k in ("q", "v", "time", "counts"))
        outs = tuple(_new(rows, dt, fill=9) for rows, dt, _ in plant._GROUND_STEP_OUTS)
        if way == "direct":
            _lib.check(L.wbc_ground_step(g._h, g._stream(), N, N, DT, _p(q), _p(v), _p(tm), *[_p(t) for t in ins[2:]], *[_p(t) for t in outs], _p(cnt)))
        else:
            outs = g.step(q, v, ins[2], DT, time=tm, mu=ins[3], mass_scale=ins[4], ext_wrench=ins[5], counts=cnt, out=outs if way == "out" else None)
        results.append(_bits([*outs, q, v, tm, cnt]))
    assert results[0] == results[1] == results[2] and results[0][4] != _bits([_t(c["v"])])[0]
    for mode in ("lift", "fit"):
        a, b = _t(c["targets"]), _t(c["targets"])
        assert g.follow_targets(a, mode) is a
        _lib.check(L.wbc_ground_follow_targets(g._h, g._stream(), N, N, plant.FOLLOW_MODES[mode], _p(b)))
        assert _bits([a]) == _bits([b]) and _bits([a]) != _bits([_t(c["targets"])])
    g.close()


def _planner():
    c = _case()
    g = gait.GaitPlanner(strides=("trot", "walk"), device=0, wait_time=0.05)
    keep = [_t(c[k]) for k in ("cmd", "gait_id", "stride_scale", "start")]
    g.set_commands(*keep)
    return g, keep


def test_gait_planner_targets_and_targets_measured():
    c, L = _case(), _lib.lib()
    g, keep = _planner()
    tm, q, v = _t(c["time"] + 0.4), _t(c["q"]), _t(c["v"])
    fresh = g.targets(tm)
    mine = (_new(54, F64, fill=9.0), _new(0, U8, fill=9))
    given = g.targets(tm, out=mine)
    assert all(a is b for a, b in zip(given, mine))
    direct = (_new(54, F64, fill=9.0), _new(0, U8, fill=9))
    _lib.check(L.wbc_gait_targets(g._h, g._stream(), N, N, _p(tm), _p(direct[0]), _p(direct[1])))
    assert _bits(fresh) == _bits(given) == _bits(direct)
    _alive(fresh[0])
    results = []
    for way in ("fresh", "out", "direct"):
        g.set_feedback(N, k_p=0.3)                                  # the pass has a state: each way starts from its zero
        off, outs = _new(8, F64, fill=9.0), (_new(54, F64, fill=9.0), _new(0, U8, fill=9))
        if way == "direct":
            _lib.check(L.wbc_gait_targets_measured(g._h, g._stream(), N, N, _p(tm), _p(q), _p(v), _p(outs[0]), _p(outs[1]), _p(off)))
        else:
            outs = g.targets_measured(tm, q, v, out=outs if way == "out" else None, offsets=off)
        results.append(_bits([*outs, off]))
    assert results[0] == results[1] == results[2]
    g.close()


def test_trajectory_lookup_pd_step_and_the_codec():
    import torch
    c, L = _case(), _lib.lib()
    traj, tm = _traj(), _t(c["time"])
    fresh = traj.lookup(tm)
    mine = (_new(54, F64, fill=9.0), _new(0, U8, fill=9))
    given = traj.lookup(tm, out=mine)
    assert all(a is b for a, b in zip(given, mine))
    direct = (_new(54, F64, fill=9.0), _new(0, U8, fill=9))
    _lib.check(L.wbc_traj_lookup(traj._h, _stream(), N, N, _p(tm), _p(direct[0]), _p(direct[1])))
    assert _bits(fresh) == _bits(given) == _bits(direct) and len(set(fresh[1].cpu().numpy().tolist())) > 1
    traj.close()
    # the joint-space PD law, both permutations given
    qp, ap = [(5 * i + 2) % 12 for i in range(12)], [(7 * i + 3) % 12 for i in range(12)]
    b = pd.BasicController(device=0, kp=31.0, kd=1.25, u_max=9.0, q_perm=qp, act_perm=ap)
    q, v = _t(c["q"]), _t(c["v"])
    fresh = b.step(q, v)
    mine = _new(12, F64, fill=9.0)
    assert b.step(q, v, out=mine) is mine
    direct = _new(12, F64, fill=9.0)
    ints = lambda p: (C.c_int * 12)(*p)
    _lib.check(L.wbc_pd_step(0, _stream(), N, N, _p(q), _p(v), b.q_nom.ctypes.data_as(_lib.c_double_p), 31.0, 1.25, 9.0, ints(qp), ints(ap),
                             _p(direct)))
    assert _bits([fresh]) == _bits([mine]) == _bits([direct])
    _alive(fresh)
    # the wire format: message 2 is foreign, so its columns keep what the arrays held -- zeros in the package's own
    raw = bytearray(b"".join(lcm_io.encode_robot_state(c["q"][:, i], c["v"][:, i], c["tau"][:, i]) for i in range(N)))
    raw[2 * lcm_io.MESSAGE_BYTES + 3] ^= 0x40
    msgs = torch.frombuffer(raw, dtype=torch.uint8).to("cuda:0")
    fq, fv, fok = lcm_io.unpack_states(msgs, device=0)
    assert fok.cpu().numpy().tolist() == [1, 1, 0, 1, 1] and not fq[:, 2].any() and not fv[:, 2].any()
    bq, bv, bok = lcm_io.unpack_states(bytes(raw), device=0)
    mine = (_new(19, F64, fill=9.0), _new(18, F64, fill=9.0))
    gq, gv, gok = lcm_io.unpack_states(msgs, device=0, out=mine)
    assert gq is mine[0] and gv is mine[1] and (gq[:, 2] == 9.0).all() and (gv[:, 2] == 9.0).all()
    dq, dv, dok = _new(19, F64, fill=0.0), _new(18, F64, fill=0.0), _new(0, U8, fill=9)
    _lib.check(L.wbc_robot_states_unpack(0, _stream(), N, N, _p(msgs), _p(dq), _p(dv), _p(dok)))
    assert _bits([fq, fv, fok]) == _bits([bq, bv, bok]) == _bits([dq, dv, dok])
    good = [0, 1, 3, 4]
    assert _bits([gq[:, good], gv[:, good], gok]) == _bits([fq[:, good], fv[:, good], fok])
    _alive(fq, fv)
    tau = _t(c["tau"])
    packed = lcm_io.pack_controls(tau, q_perm=qp, act_perm=ap)
    direct = _new(0, U8, n=N * lcm_io.MESSAGE_BYTES, fill=9)
    _lib.check(L.wbc_robot_controls_pack(0, _stream(), N, N, _p(tau), ints(qp), ints(ap), _p(direct)))
    assert _bits([packed]) == _bits([direct]) and tuple(packed.shape) == (N * lcm_io.MESSAGE_BYTES,) and packed.dtype == torch.uint8


@pytest.mark.parametrize("ground", [False, True], ids=["rigid", "ground"])
def test_closed_loop_three_steps(ground):
    c, L = _case(), _lib.lib()
    ctrl, traj = IDController(max_batch=8, device=0), _traj()
    p, keep = _ground() if ground else (plant.RigidContactPlant(device=0, tau_max=30.0), None)
    opt = [_t(c[k]) for k in ("mu", "ms", "plant_mu", "plant_ms")]
    wrench = _t(c["wrench"]) if ground else None

    def state():
        return [_t(c[k]) for k in ("q0", "v0", "time")], _t(c["counts"])
    s1, cnt1 = state()
    kw = dict(ext_wrench=wrench) if ground else {}
    res = plant.closed_loop(ctrl, p, traj, 3, DT, *s1, mu=opt[0], mass_scale=opt[1], plant_mu=opt[2], plant_mass_scale=opt[3], counts=cnt1, **kw)
    assert len(res) == (8 if ground else 7) and len(ctrl._keep) == (13 if ground else 11) and all(a is b for a, b in zip(ctrl._keep[2:5], res[:3]))
    r1 = _bits([*res, *s1, cnt1])
    s2, cnt2 = state()
    tg, mk, tau, met, st, f, fl, ct = (_new(54, F64), _new(0, U8), _new(12, F64), _new(4, F64), _new(0, I32), _new(12, F64, fill=0.0),
                                       _new(0, I32, fill=0), _new(0, U8, fill=0))
    stream = _stream()
    head = [ctrl._h, p._h, traj._h, stream, 3, DT, N, N, *[_p(t) for t in s2], _p(tg), _p(mk), *[_p(t) for t in opt]]
    if ground:
        _lib.check(L.wbc_ground_rollout(*head, _p(wrench), _p(tau), _p(met), _p(st), _p(f), _p(ct), _p(fl), _p(cnt2)))
    else:
        _lib.check(L.wbc_plant_rollout(*head, _p(tau), _p(met), _p(st), _p(f), _p(fl), _p(cnt2)))
    ctrl._bound_stream = stream.value or 0
    r2 = _bits([tau, met, st, tg, mk, f, fl, *([ct] if ground else []), *s2, cnt2])
    assert r1 == r2 and r1[len(res)] != _bits([_t(c["q0"])])[0]
    _alive(res[0], res[5])
    # no step at all: the plant's outputs come back as zeros, for nothing wrote them
    s0, cnt0 = state()
    res0 = plant.closed_loop(ctrl, p, traj, 0, DT, *s0, counts=cnt0, **kw)
    import torch
    torch.cuda.synchronize()
    assert all(not t.any() for t in res0[5:]) and _bits([*s0, cnt0]) == _bits([*state()[0], _t(c["counts"])])
    ctrl.close(); traj.close(); p.close()


# ---- what the marshaller refuses never reaches the library
class _Counting:
    """The bound library with every call counted"""

    def __init__(self, L):
        self.L, self.calls = L, []

    def __getattr__(self, name):
        fn = getattr(self.L, name)

        def call(*args):
            self.calls.append(name)
            return fn(*args)
        return call


def _wrong(good):
    """good: a valid tensor [rows, n] or [n] -> (what is wrong, the tensor): another dtype, the same shape over transposed (for [n]:
    strided) storage, n + 1 instances"""
    import torch
    other = torch.float32 if good.dtype == torch.float64 else torch.float64
    yield "dtype", good.to(other)
    view = good.T.contiguous().T if good.dim() == 2 else torch.stack([good, good], dim=1)[:, 0]
    assert view.shape == good.shape and view.dtype == good.dtype and not view.is_contiguous()
    yield "not contiguous", view
    yield "n + 1", torch.cat([good, good[..., :1]], dim=-1).contiguous()


def _refused(call, args, kwargs, names, counting):
    """Every argument named in `names` (a position or a keyword), wrong in each way, raises ValueError and no call reaches the library"""
    tried = 0
    for name in names:
        good = args[name] if isinstance(name, int) else kwargs[name]
        for what, bad in _wrong(good):
            a, k = list(args), dict(kwargs)
            if isinstance(name, int):
                a[name] = bad
            else:
                k[name] = bad
            with pytest.raises(ValueError):
                call(*a, **k)
            tried += 1
    assert tried == 3 * len(names) and counting.calls == [], counting.calls
    call(*args, **kwargs)                                          # and the right arguments do reach it
    assert len(counting.calls) >= 1
    del counting.calls[:]


def test_refusals_never_reach_the_library(monkeypatch):
    c = _case()
    counting = _Counting(_lib.lib())
    ctrl, traj, rigid, planner = IDController(max_batch=8, device=0), _traj(), plant.RigidContactPlant(device=0), _planner()[0]
    ground, keep = _ground()
    for o in (ctrl, traj, rigid, planner, ground):
        o._L = counting
    monkeypatch.setattr(_lib, "lib", lambda: counting)             # pd and lcm_io ask for the library at every call
    tick = [_t(c[k]) for k in ("q", "v", "targets", "mask")]
    tick_out = tuple(_new(rows, dt) for rows, dt, _ in _lib.TICK_OUTS)
    # the controller: q (required), mu (optional); the caller's metrics
    _refused(ctrl.step, tick, dict(mu=_t(c["mu"]), mass_scale=_t(c["ms"])), [0, "mu"], counting)
    for what, bad in _wrong(tick_out[1]):
        with pytest.raises(ValueError):
            ctrl.step(*tick, out=(tick_out[0], bad, tick_out[2]))
    assert counting.calls == []
    state = [_t(c[k]) for k in ("q", "v", "tau", "mask")]
    # the rigid plant: tau (required), counts (optional)
    _refused(lambda *a, **k: rigid.step(*a, DT, **k), state, dict(counts=_t(c["counts"]), time=_t(c["time"])), [2, "counts"], counting)
    # the ground plant: v (required), ext_wrench (optional)
    _refused(lambda *a, **k: ground.step(*a, DT, **k), state[:3], dict(ext_wrench=_t(c["wrench"])), [1, "ext_wrench"], counting)
    _refused(ground.follow_targets, [_t(c["targets"])], {}, [0], counting)
    # the planner: time (required), offsets (optional)
    planner.set_feedback(N)
    del counting.calls[:]
    _refused(planner.targets_measured, [_t(c["time"]), _t(c["q"]), _t(c["v"])], dict(offsets=_new(8, F64)), [0, "offsets"], counting)
    _refused(planner.set_commands, [_t(c["cmd"])], dict(start=_t(c["start"])), ["start"], counting)
    # the trajectory: time (required; n + 1 of them against n outputs), the caller's targets (optional)
    pair = (_new(54, F64), _new(0, U8))
    _refused(lambda tm, tg: traj.lookup(tm, out=(tg, pair[1])), [_t(c["time"]), pair[0]], {}, [0, 1], counting)
    # the PD law: q (required), out (optional)
    b = pd.BasicController(device=0)
    _refused(b.step, [_t(c["q"]), _t(c["v"])], dict(out=_new(12, F64)), [0, "out"], counting)
    # the codec: the messages (required; n + 1 bytes are no whole messages), the caller's v (optional)
    msgs = _t(np.frombuffer(b"".join(lcm_io.encode_robot_state(c["q"][:, i], c["v"][:, i]) for i in range(N)), np.uint8))
    qv = (_new(19, F64), _new(18, F64))
    del counting.calls[:]                                          # the host encoder's
    _refused(lambda m, v: lcm_io.unpack_states(m, device=0, out=(qv[0], v)), [msgs, qv[1]], {}, [0, 1], counting)
    for what, bad in list(_wrong(_t(c["tau"])))[:2]:
        with pytest.raises(ValueError):
            lcm_io.pack_controls(bad)
    assert counting.calls == []
    monkeypatch.undo()
    for o in (ctrl, traj, rigid, planner, ground):
        o._L = counting.L
        o.close()


def _gpus():
    import torch
    return torch.cuda.device_count()


@pytest.mark.skipif(_gpus() < 2, reason="a tensor on another GPU needs a second GPU")
def test_a_caller_s_out_on_another_gpu_is_refused(monkeypatch):
    """TrunkTrajectory.lookup(out=), BasicController.step(out=) and unpack_states(messages, out=) used to hand such a tensor to the kernel"""
    import torch
    c = _case()
    counting = _Counting(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: counting)
    there = lambda t: t.to("cuda:1")
    traj = _traj()
    traj._L = counting
    del counting.calls[:]
    pair = (_new(54, F64), _new(0, U8))
    for out in ((there(pair[0]), pair[1]), (pair[0], there(pair[1]))):
        with pytest.raises(ValueError, match="lives on cuda:1"):
            traj.lookup(_t(c["time"]), out=out)
    b = pd.BasicController(device=0)
    with pytest.raises(ValueError, match="lives on cuda:1"):
        b.step(_t(c["q"]), _t(c["v"]), out=there(_new(12, F64)))
    assert counting.calls == []
    msgs = _t(np.frombuffer(b"".join(lcm_io.encode_robot_state(c["q"][:, i], c["v"][:, i]) for i in range(N)), np.uint8))
    qv = (_new(19, F64), _new(18, F64))
    del counting.calls[:]                                          # the host encoder's
    for kw in (dict(messages=there(msgs), out=qv), dict(messages=msgs, out=(there(qv[0]), qv[1])), dict(messages=msgs, out=(qv[0], there(qv[1])))):
        with pytest.raises(ValueError, match="lives on cuda:1"):
            lcm_io.unpack_states(device=0, **kw)
    assert counting.calls == []
    traj._L = counting.L
    traj.close()
    torch.cuda.synchronize()
