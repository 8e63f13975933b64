"""ctypes view of tools/libhost_terrain.so: the compliant-ground plant math of csrc/wbc_ground.hpp with its TERRAIN instantiation
on the host (tests only).  run() takes what host_ground.run takes, and the terrain as GroundContactPlant.set_terrain takes it."""
import ctypes as C
import os
import subprocess

import numpy as np

import host_ground as hg
from quadruped_drake_amd import terrain as tr

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = None
PARAM_NAMES = hg.PARAM_NAMES
defaults = hg.defaults


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_ROOT, "tools", "libhost_terrain.so")
        srcs = [os.path.join(_ROOT, "tools", "host_terrain.cpp"), os.path.join(_ROOT, "include", "wbc_ground.h")] + [
            os.path.join(_ROOT, "quadruped_drake_amd", "csrc", f) for f in ("wbc_ground.hpp", "wbc_plant.hpp", "wbc_tick.hpp", "wbc_model.hpp")]
        if not os.path.exists(so) or any(os.path.getmtime(so) < os.path.getmtime(s) for s in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++20", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, srcs[0]])
        _LIB = C.CDLL(so)
        _LIB.host_terrain_batch.argtypes = ([C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double] + [C.c_void_p] * 12 +
                                            [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p])
    return _LIB


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def run(flat, q, v, tau, mu=None, mass_scale=None, ext_wrench=None, params=None, q_perm=None, act_perm=None, dt=None, substeps=0,
        time=None, counts=None, n=None, profiles=None, terrain_id=None, terrain_scale=None):
    """One force evaluation (dt None) or one step of `substeps` substeps (0: ceil(dt / max_substep)) on the terrain `profiles` (a
    list of terrain.Profile; None: no terrain), instance i on profile terrain_id[i] (default 0) scaled by terrain_scale[i]
    (default 1).  Returns dict(vdot, force, contact, flags[, q, v, time, counts, substeps]) -- copies, inputs untouched."""
    q = np.array(q, dtype=np.float64, order="C"); v = np.array(v, dtype=np.float64, order="C")
    tau = np.ascontiguousarray(tau, dtype=np.float64)
    ld = q.shape[1]
    n = ld if n is None else int(n)
    assert 0 < n <= ld
    flat = np.ascontiguousarray(flat, dtype=np.float64)
    qp = np.ascontiguousarray(range(12) if q_perm is None else q_perm, dtype=np.int32)
    ap = np.ascontiguousarray(range(12) if act_perm is None else act_perm, dtype=np.int32)
    pr = None
    if params is not None:
        d = defaults(flat); d.update(params)
        pr = np.array([d[k] for k in PARAM_NAMES], dtype=np.float64)
    f64 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
    mu, ms, we, ts = f64(mu), f64(mass_scale), f64(ext_wrench), f64(terrain_scale)
    ti = None if terrain_id is None else np.ascontiguousarray(terrain_id, dtype=np.uint8)
    tm = None if time is None else np.array(time, dtype=np.float64)
    cn = None if counts is None else np.array(counts, dtype=np.int32)
    vd = np.zeros((18, ld)); f = np.zeros((12, ld)); ct = np.zeros(ld, np.uint8); fl = np.zeros(ld, np.int32)
    for a, rows in ((tau, 12), (we, 6), (cn, 4)):
        assert a is None or a.shape == (rows, ld)
    for a in (mu, ms, ts, ti):
        assert a is None or a.shape == (ld,)
    arr, count = (None, 0) if not profiles else (tr.c_array(profiles), len(profiles))
    rc = lib().host_terrain_batch(_p(flat), _p(qp), _p(ap), _p(pr), n, ld, 0 if dt is None else 1, int(substeps),
                                  0.0 if dt is None else float(dt), _p(q), _p(v), _p(tm), _p(tau), _p(mu), _p(ms), _p(we), _p(vd), _p(f),
                                  _p(ct), _p(fl), _p(cn), None if arr is None else C.cast(arr, C.c_void_p), count, _p(ti), _p(ts))
    assert rc > 0, rc
    out = dict(vdot=vd, force=f, contact=ct, flags=fl)
    if dt is not None:
        out.update(q=q, v=v, time=tm, counts=cn, substeps=rc)
    return out
