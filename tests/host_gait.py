"""ctypes view of tools/libhost_gait.so: the gait planner's law of csrc/wbc_gait.hpp instantiated on the host (tests only).
run() takes the planner as gait.GaitPlanner takes it and the per-instance inputs as its set_commands does, as numpy arrays."""
import ctypes as C

import numpy as np

import __graft_entry__ as graft
from host_plant import _f64, _p
from quadruped_drake_amd import gait, workloads

_LIB = None
TABLE_DOUBLES = 12 + 16 * 204


def lib():
    global _LIB
    if _LIB is None:
        _LIB = C.CDLL(graft.build_target("host_gait"))
        _LIB.host_gait_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 9 + [C.c_int]
    return _LIB


def params(model="mini_cheetah", swing_height=0.05, ramp_time=0.5, wait_time=0.0, stance=None, height=None):
    """dict(stance [4, 2], height, swing_height, ramp_time, wait_time): GaitPlanner's defaults for `model`"""
    st = np.array(workloads.STAND_FEET[model] if stance is None else stance, dtype=np.float64)[:, :2]
    return dict(stance=st, height=float(workloads.NOMINAL_HEIGHT[model] if height is None else height), swing_height=float(swing_height),
                ramp_time=float(ramp_time), wait_time=float(wait_time))


def run(strides, time, cmd, gait_id=None, stride_scale=None, start=None, n=None, out=None, diag_foot=None, table=False, **par):
    """-> (targets [54, ld], mask [ld]) of the instances at time [ld] under cmd [3, ld] (+ diag [4, ld] = stride number, phase, u and
    run start of foot `diag_foot` when that is given; + the packed table when `table`).  strides: names of gait.STRIDES or
    (durations, masks) pairs; par: params()'s arguments, or `p` = such a dict.  n: the batch size where the arrays are wider;
    out: a preset (targets, mask) pair to write into."""
    P = par.pop("p", None) or params(**par)
    cp = gait.c_params(P["stance"], P["height"], P["swing_height"], P["ramp_time"], P["wait_time"])
    strides = [strides] if isinstance(strides, str) else list(strides)
    cs = gait.c_strides(strides)
    time, cmd = _f64(time), _f64(cmd)
    ld = time.shape[0]
    n = ld if n is None else n
    assert cmd.shape == (3, ld)
    ss, st = _f64(stride_scale), _f64(start)
    gi = None if gait_id is None else np.ascontiguousarray(gait_id, dtype=np.uint8)
    assert (ss is None or ss.shape == (ld,)) and (st is None or st.shape == (3, ld)) and (gi is None or gi.shape == (ld,))
    tg, mk = (np.zeros((54, ld)), np.zeros(ld, np.uint8)) if out is None else out
    assert tg.shape == (54, ld) and tg.dtype == np.float64 and tg.flags.c_contiguous and mk.dtype == np.uint8
    dg = None if diag_foot is None else np.zeros((4, ld))
    tb = np.zeros(TABLE_DOUBLES) if table else None
    rc = lib().host_gait_batch(C.cast(C.byref(cp), C.c_void_p), C.cast(cs, C.c_void_p), len(strides), n, ld, _p(time), _p(cmd), _p(gi),
                               _p(ss), _p(st), _p(tg), _p(mk), _p(tb), _p(dg), 0 if diag_foot is None else int(diag_foot))
    assert rc == 0, rc
    res = (tg, mk)
    if dg is not None:
        res += (dg,)
    if table:
        res += (tb,)
    return res
