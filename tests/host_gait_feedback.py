"""ctypes view of host_gait_feedback_batch of tools/libhost_gait.so: the gait planner's foot-placement feedback
(include/wbc_gait_feedback.h), csrc/wbc_gait_feedback.hpp instantiated on the host (tests only).  The caller holds the
state, in the device's layout, in a State."""
import ctypes as C

import numpy as np

import host_gait as hg
from host_plant import _f64, _p
from quadruped_drake_amd import _lib, gait

_BOUND = False


def lib():
    global _BOUND
    L = hg.lib()
    if not _BOUND:
        L.host_gait_feedback_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 8 + [C.c_int, C.c_void_p, C.c_void_p]
        L.host_gait_feedback_reset.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
        L.host_gait_feedback_reset.restype = None
        _BOUND = True
    return L


class State:
    """state [6, 4 cap] (rows cur_x, cur_y, from_x, from_y, to_x, to_y; foot f of instance i at 4 i + f) and prev [cap], as
    wbc_gait_set_feedback leaves them"""

    def __init__(self, cap):
        self.cap = int(cap)
        self.state, self.prev = np.empty((6, 4 * self.cap)), np.empty(self.cap, np.uint8)
        lib().host_gait_feedback_reset(self.cap, _p(self.state), _p(self.prev))

    def copy(self):
        s = State.__new__(State)
        s.cap, s.state, s.prev = self.cap, self.state.copy(), self.prev.copy()
        return s


def c_feedback(par):
    return _lib.WbcGaitFeedbackParams(**{k: float(par[k]) for k in ("k_v", "k_p", "d_max", "u_hold")})


def run(strides, par, time, q, v, targets, mask, state, gait_id=None, stride_scale=None, n=None, offsets=True, rc=False, **gpar):
    """The pass on targets [54, ld] and mask [ld], in place, advancing `state`; -> (targets, offsets [8, ld] or None).  par: dict(k_v,
    k_p, d_max, u_hold); gpar: host_gait.params()'s arguments, or `p` = such a dict.  rc: return the tool's return code."""
    P = gpar.pop("p", None) or hg.params(**gpar)
    cp = gait.c_params(P["stance"], P["height"], P["swing_height"], P["ramp_time"], P["wait_time"])
    strides = [strides] if isinstance(strides, str) else list(strides)
    cs = gait.c_strides(strides)
    fp = c_feedback(par)
    time, q, v = _f64(time), _f64(q), _f64(v)
    ld = time.shape[0]
    n = ld if n is None else n
    ss = _f64(stride_scale)
    gi = None if gait_id is None else np.ascontiguousarray(gait_id, dtype=np.uint8)
    assert q.shape == (19, ld) and v.shape == (18, ld) and targets.shape == (54, ld) and targets.dtype == np.float64 and targets.flags.c_contiguous
    assert mask.dtype == np.uint8 and mask.shape == (ld,) and (ss is None or ss.shape == (ld,)) and (gi is None or gi.shape == (ld,))
    off = np.zeros((8, ld)) if offsets is True else (None if offsets is None or offsets is False else offsets)
    code = lib().host_gait_feedback_batch(C.cast(C.byref(cp), C.c_void_p), C.cast(cs, C.c_void_p), len(strides), C.cast(C.byref(fp), C.c_void_p),
                                          n, ld, _p(time), _p(gi), _p(ss), _p(q), _p(v), _p(targets), _p(mask), _p(off), state.cap,
                                          _p(state.state), _p(state.prev))
    if rc:
        return code
    assert code == 0, code
    return targets, off
