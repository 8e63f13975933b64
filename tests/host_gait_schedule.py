"""ctypes view of host_gait_schedule_batch of tools/libhost_gait.so: the gait planner's law under command schedules
(include/wbc_gait_schedule.h), the SCHEDULE instantiations of csrc/wbc_gait.hpp on the host (tests only).  run() takes the
planner as host_gait.run takes it, the schedule as wbc_gait_set_schedule does, an optional terrain as host_gait_terrain.run does, and
numpy arrays."""
import ctypes as C

import numpy as np

import host_gait as hg
from host_plant import _f64, _p
from quadruped_drake_amd import gait, terrain

_BOUND = False
KNOT_ROWS = 7 * 25


def lib():
    global _BOUND
    L = hg.lib()
    if not _BOUND:
        L.host_gait_schedule_batch.argtypes = ([C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 7 +
                                               [C.c_double] + [C.c_void_p] * 6)
        _BOUND = True
    return L


def run(strides, time, cmd, nswitch, when, cmds, blend, gait_id=None, stride_scale=None, start=None, profiles=None, terrain_id=None,
        terrain_scale=None, tp=None, n=None, out=None, rc=False, knots=False, **par):
    """-> (targets [54, ld], mask [ld]) of the instances at time [ld] under cmd [3, ld] and the schedule nswitch [ld], when [7, ld] (path
    parameters), cmds [21, ld], blend.  profiles: a list of terrain.Profile for the terrain law (tp: host_gait_terrain.run's), None: the
    plane.  par: host_gait.params()'s arguments, or `p` = such a dict; n, out: as host_gait.run.  rc: return the tool's return code
    instead of asserting that it is 0; knots: also return the resolved schedules [175, ld]."""
    P = par.pop("p", None) or hg.params(**par)
    cp = gait.c_params(P["stance"], P["height"], P["swing_height"], P["ramp_time"], P["wait_time"])
    strides = [strides] if isinstance(strides, str) else list(strides)
    cs = gait.c_strides(strides)
    time, cmd = _f64(time), _f64(cmd)
    ld = time.shape[0]
    n = ld if n is None else n
    assert cmd.shape == (3, ld)
    ss, st, ts, wh, cm = _f64(stride_scale), _f64(start), _f64(terrain_scale), _f64(when), _f64(cmds)
    u8 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.uint8)
    gi, ti, ns = u8(gait_id), u8(terrain_id), u8(nswitch)
    for a, shape in ((ss, (ld,)), (st, (3, ld)), (gi, (ld,)), (ti, (ld,)), (ts, (ld,)), (ns, (ld,)), (wh, (7, ld)), (cm, (21, ld))):
        assert a is None or a.shape == shape, (a.shape, shape)
    if profiles is not None:
        profiles = list(profiles)
        ctp = gait.c_terrain_params(**(tp or {}))
        arr = terrain.c_array(profiles)
        tpp, arrp, tcount = C.cast(C.byref(ctp), C.c_void_p), C.cast(arr, C.c_void_p), len(profiles)
    else:
        tpp, arrp, tcount = None, None, 0
    tg, mk = (np.zeros((54, ld)), np.zeros(ld, np.uint8)) if out is None else out
    assert tg.shape == (54, ld) and tg.dtype == np.float64 and tg.flags.c_contiguous and mk.dtype == np.uint8
    kn = np.zeros((KNOT_ROWS, ld)) if knots else None
    code = lib().host_gait_schedule_batch(C.cast(C.byref(cp), C.c_void_p), C.cast(cs, C.c_void_p), len(strides), tpp, arrp, tcount, n, ld,
                                          _p(time), _p(cmd), _p(gi), _p(ss), _p(st), _p(ti), _p(ts), float(blend), _p(ns), _p(wh), _p(cm),
                                          _p(tg), _p(mk), _p(kn))
    if rc:
        return code
    assert code == 0, code
    return (tg, mk, kn) if knots else (tg, mk)
