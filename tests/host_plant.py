"""ctypes view of tools/libhost_plant.so: the plant math of csrc/wbc_plant.hpp instantiated on the host (tests only)."""
import ctypes as C

import numpy as np

import __graft_entry__ as graft

_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        _LIB = C.CDLL(graft.build_target("host_plant"))
        _LIB.host_plant_batch.argtypes = ([C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_int, C.c_double] + [C.c_void_p] * 11)
    return _LIB


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _f64(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


def batch(flat, q, v, tau, q_perm, act_perm, time, counts, n):
    """What every host plant's run() makes of its arguments: copies of q, v (and time, counts where given) for the step to work
    on, contiguous flat, tau and permutations, and the batch size n within the arrays' ld columns.
    -> (flat, q, v, tau, q_perm, act_perm, time, counts, n, ld)"""
    q = np.array(q, dtype=np.float64, order="C"); v = np.array(v, dtype=np.float64, order="C")
    ld = q.shape[1]
    n = ld if n is None else int(n)
    assert 0 < n <= ld
    qp = np.ascontiguousarray(range(12) if q_perm is None else q_perm, dtype=np.int32)
    ap = np.ascontiguousarray(range(12) if act_perm is None else act_perm, dtype=np.int32)
    tm = None if time is None else np.array(time, dtype=np.float64)
    cn = None if counts is None else np.array(counts, dtype=np.int32)
    return _f64(flat), q, v, _f64(tau), qp, ap, tm, cn, n, ld


def run(flat, q, v, tau, mask, mu=None, mass_scale=None, params3=None, q_perm=None, act_perm=None, dt=None, time=None, counts=None,
        n=None, out=None):
    """Forward (dt None) or step.  Returns dict(vdot, force, flags[, q, v, time, counts]) -- copies, inputs untouched.
    n: the batch size where the arrays are wider (ld = q.shape[1] > n; every 2-D array then has ld columns).  out: a dict of
    preset vdot / force / flags arrays to write into (for looking at what is left of the padding columns)."""
    flat, q, v, tau, qp, ap, tm, cn, n, ld = batch(flat, q, v, tau, q_perm, act_perm, time, counts, n)
    mask = np.ascontiguousarray(mask, dtype=np.uint8)
    pr, mu, ms = _f64(params3), _f64(mu), _f64(mass_scale)
    vd = np.zeros((18, ld)); f = np.zeros((12, ld)); fl = np.zeros(ld, np.int32)
    if out is not None:
        vd, f, fl = out["vdot"], out["force"], out["flags"]
        assert vd.shape == (18, ld) and f.shape == (12, ld) and vd.dtype == f.dtype == np.float64
        assert fl.dtype == np.int32 and all(a.flags.c_contiguous for a in (vd, f, fl))
    for a, rows in ((tau, 12), (cn, 4)):
        assert a is None or a.shape == (rows, ld)
    rc = lib().host_plant_batch(_p(flat), _p(qp), _p(ap), _p(pr), n, ld, 0 if dt is None else 1, 0.0 if dt is None else float(dt),
                                _p(q), _p(v), _p(tm), _p(tau), _p(mask), _p(mu), _p(ms), _p(vd), _p(f), _p(fl), _p(cn))
    assert rc == 0
    out = dict(vdot=vd, force=f, flags=fl)
    if dt is not None:
        out.update(q=q, v=v, time=tm, counts=cn)
    return out
