"""Terrain of the compliant-ground plant on the MI355X (include/wbc_ground.h, GroundContactPlant.set_terrain): the two terrain
kernels against the host instantiation of the same templates (tests/host_terrain.py) and the dense numpy plant
(tests/terrain_oracle.py), malformed terrain choices in every robot slot of a wavefront, resources, a closed loop on a slope
followed tick by tick, and clearing."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import ground_oracle as go
import host_terrain as ht
import plant_edges as pe
import terrain_oracle as to
from quadruped_drake_amd import terrain as tr, workloads

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODEL, CFG = "anymal_b", 4
BACKENDS = ("oracle", "energy")
ORACLE_SAMPLE = 24          # instances per case that the dense plant answers (all of them where n is smaller)


def _t(a, dtype=None):
    import torch
    return torch.tensor(np.ascontiguousarray(a), device=DEV, dtype=dtype)


def _rel(a, b):
    return np.abs(a - b).max() / (1.0 + np.abs(b).max())


def _device(plant, b, n, ld, dt):
    """wbc_ground_forward (dt None) or wbc_ground_step through the C ABI with arrays of ld >= n columns -> dict of numpy arrays."""
    import torch
    w = lambda a: _t(pe.wide(a[..., :n], ld, np.nan))
    q, v = (_t(pe.wide(b[k][..., :n], ld, np.nan if dt is None else None)) for k in ("q", "v"))
    tau, mu, ms, we = w(b["tau"]), w(b["mu"]), w(b["mass_scale"]), w(b["ext_wrench"])
    vd, f, ct, fl = (_t(pe.wide(np.zeros(s + (0,), d), ld)) for s, d in (((18,), np.float64), ((12,), np.float64), ((), np.uint8), ((), np.int32)))
    p = lambda x: C.c_void_p(x.data_ptr())
    L = plant._L
    if dt is None:
        rc = L.wbc_ground_forward(plant._h, plant._stream(), n, ld, p(q), p(v), p(tau), p(mu), p(ms), p(we), p(vd), p(f), p(ct), p(fl))
    else:
        rc = L.wbc_ground_step(plant._h, plant._stream(), n, ld, float(dt), p(q), p(v), None, p(tau), p(mu), p(ms), p(we), p(f), p(ct), p(fl), None)
    assert rc == 0, L.wbc_last_error().decode()
    torch.cuda.synchronize()
    out = dict(force=f, contact=ct, flags=fl, **(dict(vdot=vd) if dt is None else dict(q=q, v=v)))
    out = {k: x.cpu().numpy() for k, x in out.items()}
    for k, x in out.items():
        assert pe.padding_kept(x, n, np.nan if (dt is None and k in ("q", "v")) else None), k
    return {k: np.ascontiguousarray(x[..., :n]) for k, x in out.items()}


MODES = {"forward": None, "step_S1": 6e-5, "step_S16": 1e-3}


@functools.lru_cache(maxsize=None)
def _case(mode):
    """The four-profile batch of 203 instances of tests/test_terrain_cpu.py for one mode, computed once: inputs, and for every n
    the host twin's answer on the first n instances and the dense plant's on a sample of them."""
    dt = MODES[mode]
    t, q, v, tau, sp, we, profiles, tid, tsc = to.draw(CFG, 203, 70 + len(mode), near_stance=dt is not None)
    b = dict(q=q, v=v, tau=tau, mu=np.random.default_rng(5).uniform(0.3, 1.0, 203), mass_scale=sp, ext_wrench=we)
    for a in b.values():
        a.setflags(write=False)
    return dict(t=t, b=b, profiles=profiles, tid=tid, tsc=tsc, dt=dt, S=None if dt is None else go.substeps(dt, 6.25e-5))


@functools.lru_cache(maxsize=None)
def _reference(mode, n, over=()):
    """over: handle parameters away from their defaults, as a tuple of (name, value)."""
    c = _case(mode)
    t, b, dt = c["t"], c["b"], c["dt"]
    P = go.params(t, dict(over))
    cut = {k: np.ascontiguousarray(x[..., :n]) for k, x in b.items()}
    tid, tsc = c["tid"][:n], c["tsc"][:n]
    host = ht.run(t["flat"], cut["q"], cut["v"], cut["tau"], mu=cut["mu"], mass_scale=cut["mass_scale"], ext_wrench=cut["ext_wrench"],
                  act_perm=t.get("act_perm"), dt=dt, profiles=c["profiles"], terrain_id=tid, terrain_scale=tsc,
                  params=dict(over) if over else None)
    margin = lambda i, backend: to.margin(t, cut["q"][:, i], cut["v"][:, i], cut["tau"][:, i], c["profiles"][tid[i]], tsc[i],
                                          mu=cut["mu"][i], s_p=cut["mass_scale"][i], P=P, backend=backend)
    host["keep"] = np.array([margin(i, "oracle") > 1e-6 for i in range(n)])       # every instance: the flags against the host twin
    idx = np.arange(n) if n <= ORACLE_SAMPLE else np.sort(np.random.default_rng(n).choice(n, ORACLE_SAMPLE, replace=False))
    sel = lambda a: np.ascontiguousarray(a[..., idx])
    dense = {}
    for backend in BACKENDS:
        kw = dict(mu=sel(cut["mu"]), mass_scale=sel(cut["mass_scale"]), ext_wrench=sel(cut["ext_wrench"]), P=P, backend=backend)
        if dt is None:
            vd, f, ct, fl = to.forward(t, sel(cut["q"]), sel(cut["v"]), sel(cut["tau"]), c["profiles"], tid[idx], tsc[idx], **kw)
            dense[backend] = dict(vdot=vd, force=f, contact=ct, flags=fl)
        else:
            qn, vn, fm, ct, fl = to.step(t, sel(cut["q"]), sel(cut["v"]), sel(cut["tau"]), dt, c["S"], c["profiles"], tid[idx], tsc[idx], **kw)
            dense[backend] = dict(q=qn, v=vn, force=fm, contact=ct, flags=fl)
        dense[backend]["keep"] = np.array([margin(i, backend) > 1e-6 for i in idx])
    return host, idx, dense


def _plant(c, n, **kw):
    from quadruped_drake_amd import GroundContactPlant
    plant = GroundContactPlant(MODEL, device=0, **kw)
    plant.set_terrain(c["profiles"], _t(c["tid"][:n]), _t(c["tsc"][:n]))
    return plant


def _compare(got, host, idx, dense, what):
    worst = {}
    for k, x in host.items():
        if not isinstance(x, np.ndarray) or k not in got or k == "keep":
            continue
        if x.dtype == np.float64:
            worst["host " + k] = _rel(got[k], x)
            assert worst["host " + k] < 1e-9, (what, k)
        elif k == "contact":
            assert np.array_equal(got[k], x), (what, k)
        elif k == "flags":
            assert host["keep"].sum() >= 0.9 * x.size, what
            assert np.array_equal(got[k][host["keep"]], x[host["keep"]]), (what, k)
    for backend, ref in dense.items():
        keep = ref["keep"]
        assert keep.sum() >= 0.9 * idx.size, (what, backend)
        for k, x in ref.items():
            if k == "keep":
                continue
            if x.dtype == np.float64:
                worst[backend + " " + k] = _rel(got[k][..., idx], x)
                assert worst[backend + " " + k] < 1e-9, (what, backend, k)
            elif k == "contact":
                assert np.array_equal(got[k][idx], x), (what, backend)
            else:
                assert np.array_equal(got[k][idx][keep], x[keep]), (what, backend, k)
    print(what, "worst", {k: float("%.3g" % x) for k, x in worst.items()})


@pytest.mark.parametrize("n,ld", [(1, 1), (17, 24), (203, 203)])
@pytest.mark.parametrize("mode", list(MODES))
def test_device_terrain_matches_host_twin_and_dense_oracle(mode, n, ld):
    c = _case(mode)
    host, idx, dense = _reference(mode, n)
    if c["dt"] is not None:
        assert host["substeps"] == c["S"] == {"step_S1": 1, "step_S16": 16}[mode]
    plant = _plant(c, n)
    got = _device(plant, c["b"], n, ld, c["dt"])
    plant.close()
    if n == 203:      # the batch is on every profile, on both sides of the surface, and the flags' outcomes differ
        assert set(c["tid"].tolist()) == {0, 1, 2, 3}
        bits = (got["contact"][None, :] >> np.arange(4)[:, None]) & 1
        assert bits.mean() >= 0.2 and (1 - bits).mean() >= 0.2
        assert (got["flags"] & go.BAD == 0).all()
    _compare(got, host, idx, dense, "%s n=%d ld=%d" % (mode, n, ld))


@pytest.mark.parametrize("mode", ["forward", "step_S16"])
def test_device_terrain_renumbered(mode):
    """Random q_perm / act_perm: the caller's joint rows permuted, the references on the canonical rows."""
    n = 203
    c = _case(mode)
    t, b = c["t"], c["b"]
    qp, ap = pe.perm_pair(8, avoid=t.get("act_perm", range(12)))
    b2 = dict(b)
    b2["q"], b2["v"] = pe.permute_rows(b["q"], b["v"], qp)
    b2["tau"] = np.ascontiguousarray(b["tau"][np.argsort(np.asarray(t.get("act_perm", range(12))))][ap])
    plant = _plant(c, n, q_perm=qp, act_perm=ap)
    got = _device(plant, b2, n, n, c["dt"])
    plant.close()
    for k in ("q",):
        if k in got:
            got[k] = pe.canonical_q(got[k], qp)
    for k in ("v", "vdot"):
        if k in got:
            got[k] = pe.canonical_v(got[k], qp)
    host, idx, dense = _reference(mode, n)
    _compare(got, host, idx, dense, "renumbered " + mode)


def _trunk_clearance(q, c, n):
    return np.array([q[6, i] - to.surface(c["profiles"][c["tid"][i]], c["tsc"][i], q[4, i], q[5, i])[0] for i in range(n)])


@pytest.mark.parametrize("mode", ["forward", "step_S16"])
def test_device_fell_on_the_terrain_and_foot_radius(mode):
    """fall_height at the median height of the trunks above their own ground and a foot radius of 0.7 mm: FELL splits the batch,
    in the given state (forward) and in the end state (step), is what the header's sentence says of the device's own end state,
    and is not what the flat rule (trunk height against fall_height alone) or the unscaled profile would give."""
    n = 203
    c = _case(mode)
    fh = float(np.median(_trunk_clearance(c["b"]["q"], c, n)))
    over = (("fall_height", fh), ("foot_radius", 0.7e-3))
    host, idx, dense = _reference(mode, n, over)
    plant = _plant(c, n, **dict(over))
    got = _device(plant, c["b"], n, n, c["dt"])
    plant.close()
    assert (got["flags"] & go.BAD == 0).all()
    fell = (got["flags"] & go.FELL) != 0
    qe = c["b"]["q"] if c["dt"] is None else got["q"]
    keep = np.abs(_trunk_clearance(qe, c, n) - fh) > 1e-9
    assert keep.sum() >= 0.9 * n and np.array_equal(fell[keep], (_trunk_clearance(qe, c, n) <= fh)[keep])
    assert 0.3 * n < fell.sum() < 0.7 * n
    assert (fell != ~(qe[6] > fh)).sum() > 0.1 * n                       # the flat rule
    unscaled = dict(c, tsc=np.ones(n))
    assert (fell != (_trunk_clearance(qe, unscaled, n) <= fh)).any()
    for ref in dense.values():
        assert ((ref["flags"] & go.FELL) != 0).any() and ((ref["flags"] & go.FELL) == 0).any()
    _compare(got, host, idx, dense, "fall_height and foot_radius, " + mode)
    # the radius reached the kernel: the default gives other contacts
    assert not np.array_equal(got["contact"], _reference(mode, n)[0]["contact"])


def test_simulate_on_a_slope_reports_fell_and_slip(capsys):
    """python -m quadruped_drake_amd.simulate --plant ground --terrain slope:0.1 (and --plant rigid): the closed loop runs and the
    JSON line carries the plant's flag counts."""
    import json
    from quadruped_drake_amd import simulate
    common = ["--control", "ID", "--n", "8", "--sim-time", "0.05", "--dt", "1e-3", "--log-every", "25"]
    rc = simulate.main(common + ["--plant", "ground", "--terrain", "slope:0.1"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rc in (0, 1) and line["plant"] == "ground" and line["terrain"] == "slope:0.1" and line["ticks"] == 50 * 8
    assert set(line["plant_flags"]) == {"slip", "fell", "clip", "bad"} and line["plant_flags"]["bad"] == 0
    assert line["FELL"] == line["plant_flags"]["fell"] and line["SLIP"] == line["plant_flags"]["slip"] and 0 <= line["FELL"] <= 8
    assert 0.2 < line["body_height_final"][0] <= line["body_height_final"][1] < 0.4       # still standing on the slope at the origin
    rc = simulate.main(common + ["--plant", "rigid"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rc in (0, 1) and line["plant"] == "rigid" and set(line["plant_flags"]) == {"pull", "cone", "clip", "bad"}
    assert "FELL" not in line
    simulate.main(common)
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert "plant" not in line and "plant_flags" not in line                # the default is the plan, its line unchanged


@pytest.mark.parametrize("kind", ["id_beyond_table", "nan_scale"])
def test_bad_terrain_choice_in_every_robot_slot(kind):
    """An out-of-range terrain_id / a NaN terrain_scale in each of the 16 robot slots of a wavefront (one slot per wavefront of
    five, pe.slots_of): that instance is BAD with its state untouched, its 15 wave-mates and everyone else keep their bits."""
    n = 80
    c = _case("step_S16")
    b = {k: np.ascontiguousarray(x[..., :n]) for k, x in c["b"].items()}
    hit = pe.slots_of(3 if kind == "nan_scale" else 0, n)
    tid, tsc = c["tid"][:n].copy(), c["tsc"][:n].copy()
    if kind == "nan_scale":
        tsc[hit] = np.nan
    else:
        tid[hit] = np.where(np.arange(hit.size) % 2 == 0, len(c["profiles"]), 255)
    runs = {}
    for name, (i_, s_) in dict(clean=(c["tid"][:n], c["tsc"][:n]), dirty=(tid, tsc)).items():
        from quadruped_drake_amd import GroundContactPlant
        plant = GroundContactPlant(MODEL, device=0)
        plant.set_terrain(c["profiles"], _t(i_), _t(s_))
        runs[name] = (_device(plant, b, n, n, None), _device(plant, b, n, n, c["dt"]))
        plant.close()
    ok = np.ones(n, bool); ok[hit] = False
    for clean, dirty in zip(runs["clean"], runs["dirty"]):
        assert (clean["flags"] & go.BAD == 0).all()
        assert (dirty["flags"][hit] == go.BAD).all()
        assert (dirty["force"][:, hit] == 0).all() and (dirty["contact"][hit] == 0).all()
        for k in clean:
            assert pe.same_bits(clean[k][..., ok], dirty[k][..., ok]), k
    assert (runs["dirty"][0]["vdot"][:, hit] == 0).all()
    assert pe.same_bits(runs["dirty"][1]["q"][:, hit], b["q"][:, hit]) and pe.same_bits(runs["dirty"][1]["v"][:, hit], b["v"][:, hit])
    assert not np.array_equal(runs["clean"][1]["q"][:, hit], b["q"][:, hit])


def test_terrain_kernel_resources():
    from quadruped_drake_amd import GroundContactPlant
    fresh = GroundContactPlant(MODEL, device=0)
    flat_info = fresh.kernel_info()
    plant = GroundContactPlant(MODEL, device=0)
    plant.set_terrain(to.four_profiles())
    info = plant.terrain_kernel_info()
    print("terrain kernel", info, "flat kernel", flat_info)
    assert info["scratch_bytes_per_lane"] == 0 and info["block_threads"] == 64
    assert 0 < info["lds_bytes"] <= 8192
    assert plant.kernel_info() == flat_info and flat_info["scratch_bytes_per_lane"] == 0 and flat_info["lds_bytes"] == 0
    with pytest.raises(ValueError):
        plant.set_terrain(to.four_profiles(), terrain_id=np.zeros(4, np.uint8))          # not a device tensor
    with pytest.raises(RuntimeError):
        plant.set_terrain([tr.flat(0.0)] * 17)
    plant.close(); fresh.close()


def test_closed_loop_on_a_slope_tick_by_tick():
    """closed_loop with the ID controller on slope(atan 0.1), 32 robots, 100 ticks of 1 ms, one tick per call: after every tick the
    device's state equals the host twin's step from the device's previous state under the device's torques.  The wiring of the
    terrain through wbc_ground_rollout, not the quality of ID on a slope.  Profile 0 of the table is another ground (level, 0.3 m
    up) and the scales differ per instance: a loop that dropped terrain_id or terrain_scale could not meet the host."""
    import torch
    from quadruped_drake_amd import GroundContactPlant, IDController, closed_loop
    from quadruped_drake_amd.trajectory import TrunkTrajectory
    n, dt, model = 32, 1e-3, "mini_cheetah"
    t, q0, v0, prof = to.slope_stance(model, 0.1, n=n)
    q0[4] = np.linspace(-0.5, 0.5, n)                    # along the slope; the height follows
    q0[6] += 0.1 * q0[4]
    profiles = [tr.flat(0.3), prof]
    tid = np.ones(n, np.uint8)
    tsc = np.where(np.arange(n) % 4 == 3, 0.99, 1.0)     # every fourth robot on a slightly flatter slope
    st_t = workloads.standing_targets(model, 1)[:, 0]
    traj = TrunkTrajectory(np.zeros(0), np.zeros((0, 54)), np.zeros(0, np.uint8), wait_time=1e9, device=0, standing_targets=st_t,
                           standing_mask=0b1111)
    ctrl = IDController(max_batch=n, device=0)
    plant = GroundContactPlant(model, device=0)
    plant.set_terrain(profiles, _t(tid), _t(tsc))
    q, v, tm = _t(q0), _t(v0), _t(np.zeros(n))
    counts = torch.zeros((4, n), dtype=torch.int32, device=DEV)
    worst, touched = 0.0, 0
    for k in range(100):
        qp, vp = q.cpu().numpy(), v.cpu().numpy()
        out = closed_loop(ctrl, plant, traj, 1, dt, q, v, tm, counts=counts)
        torch.cuda.synchronize()
        tau, f, fl, ct = (out[j].cpu().numpy() for j in (0, 5, 6, 7))
        ref = ht.run(t["flat"], qp, vp, tau, act_perm=t.get("act_perm"), dt=dt, profiles=profiles, terrain_id=tid, terrain_scale=tsc)
        assert (fl & go.BAD == 0).all(), k
        errs = (_rel(q.cpu().numpy(), ref["q"]), _rel(v.cpu().numpy(), ref["v"]), _rel(f, ref["force"]))
        worst = max(worst, *errs)
        assert max(errs) < 1e-9, (k, errs)
        assert np.array_equal(ct, ref["contact"]) and np.array_equal(fl, ref["flags"]), k
        touched += int((ct != 0).sum())
    print("closed loop on a slope: worst per-tick difference", worst, "FELL", int((counts[1] > 0).sum()), "SLIP", int((counts[0] > 0).sum()))
    assert touched > 50 * n                               # the feet were on the slope, not in the air
    assert np.allclose(tm.cpu().numpy(), 0.1)
    plant.close(); ctrl.close()


def test_clearing_the_terrain_gives_the_flat_bits():
    from quadruped_drake_amd import GroundContactPlant
    n = 203
    c = _case("step_S16")
    fresh = GroundContactPlant(MODEL, device=0)
    want = (_device(fresh, c["b"], n, n, None), _device(fresh, c["b"], n, n, c["dt"]))
    fresh.close()
    plant = _plant(c, n)
    on = _device(plant, c["b"], n, n, c["dt"])
    plant.set_terrain(None)
    got = (_device(plant, c["b"], n, n, None), _device(plant, c["b"], n, n, c["dt"]))
    plant.close()
    for a, b in zip(want, got):
        for k in a:
            assert pe.same_bits(a[k], b[k]), k
    assert not np.array_equal(on["q"], want[1]["q"])
