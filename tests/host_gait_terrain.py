"""ctypes view of host_gait_terrain_batch of tools/libhost_gait.so: the gait planner's law with a terrain
(include/wbc_gait_terrain.h), the TERRAIN instantiations of csrc/wbc_gait.hpp on the host (tests only).  run() takes
the planner as host_gait.run takes it, the terrain as gait.GaitPlanner.set_terrain does, and numpy arrays."""
import ctypes as C

import numpy as np

import host_gait as hg
from host_plant import _f64, _p
from quadruped_drake_amd import gait, terrain

_BOUND = False


def lib():
    global _BOUND
    L = hg.lib()
    if not _BOUND:
        L.host_gait_terrain_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 9
        _BOUND = True
    return L


def run(strides, profiles, time, cmd, gait_id=None, stride_scale=None, start=None, terrain_id=None, terrain_scale=None, n=None, out=None,
        tp=None, rc=False, **par):
    """-> (targets [54, ld], mask [ld]) of the instances at time [ld] under cmd [3, ld] on `profiles` (a list of terrain.Profile).
    tp: dict(body, max_grade, edge_margin, apex_max), None: GaitPlanner.set_terrain's defaults; par: host_gait.params()'s arguments,
    or `p` = such a dict; n, out: as host_gait.run.  rc: return the tool's return code instead of asserting that it is 0."""
    P = par.pop("p", None) or hg.params(**par)
    cp = gait.c_params(P["stance"], P["height"], P["swing_height"], P["ramp_time"], P["wait_time"])
    ctp = gait.c_terrain_params(**(tp or {}))
    strides = [strides] if isinstance(strides, str) else list(strides)
    cs = gait.c_strides(strides)
    profiles = list(profiles)
    arr = terrain.c_array(profiles)
    time, cmd = _f64(time), _f64(cmd)
    ld = time.shape[0]
    n = ld if n is None else n
    assert cmd.shape == (3, ld)
    ss, st, ts = _f64(stride_scale), _f64(start), _f64(terrain_scale)
    gi = None if gait_id is None else np.ascontiguousarray(gait_id, dtype=np.uint8)
    ti = None if terrain_id is None else np.ascontiguousarray(terrain_id, dtype=np.uint8)
    for a, shape in ((ss, (ld,)), (st, (3, ld)), (gi, (ld,)), (ti, (ld,)), (ts, (ld,))):
        assert a is None or a.shape == shape
    tg, mk = (np.zeros((54, ld)), np.zeros(ld, np.uint8)) if out is None else out
    assert tg.shape == (54, ld) and tg.dtype == np.float64 and tg.flags.c_contiguous and mk.dtype == np.uint8
    code = lib().host_gait_terrain_batch(C.cast(C.byref(cp), C.c_void_p), C.cast(cs, C.c_void_p), len(strides), C.cast(C.byref(ctp), C.c_void_p),
                                         C.cast(arr, C.c_void_p), len(profiles), n, ld, _p(time), _p(cmd), _p(gi), _p(ss), _p(st), _p(ti),
                                         _p(ts), _p(tg), _p(mk))
    if rc:
        return code
    assert code == 0, code
    return tg, mk
