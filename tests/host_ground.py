"""ctypes view of tools/libhost_ground.so: the compliant-ground plant math of csrc/wbc_ground.hpp instantiated on the host
(tests only)."""
import ctypes as C

import numpy as np

import __graft_entry__ as graft
from host_plant import _f64, _p, batch

_LIB = None
PARAM_NAMES = ("stiffness", "dissipation", "mu", "v_stiction", "foot_radius", "tau_max", "max_substep", "fall_height")


def lib():
    global _LIB
    if _LIB is None:
        _LIB = C.CDLL(graft.build_target("host_ground"))
        _LIB.host_ground_defaults.argtypes = [C.c_void_p, C.c_void_p]
        _LIB.host_ground_batch.argtypes = ([C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double] + [C.c_void_p] * 12)
        _LIB.host_terrain_batch.argtypes = _LIB.host_ground_batch.argtypes + [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    return _LIB


def defaults(flat):
    """The default parameters of a model as a dict keyed by PARAM_NAMES."""
    flat = np.ascontiguousarray(flat, dtype=np.float64)
    out = np.zeros(8)
    assert lib().host_ground_defaults(_p(flat), _p(out)) == 0
    return dict(zip(PARAM_NAMES, out.tolist()))


def call(entry, tail, flat, q, v, tau, mu, mass_scale, ext_wrench, params, q_perm, act_perm, dt, substeps, time, counts, n, out):
    """run() of this module and of host_terrain: `entry` is host_ground_batch or host_terrain_batch, `tail` the arguments the
    latter takes after the former's."""
    flat, q, v, tau, qp, ap, tm, cn, n, ld = batch(flat, q, v, tau, q_perm, act_perm, time, counts, n)
    pr = None
    if params is not None:
        d = defaults(flat); d.update(params)
        pr = np.array([d[k] for k in PARAM_NAMES], dtype=np.float64)
    mu, ms, we = _f64(mu), _f64(mass_scale), _f64(ext_wrench)
    vd = np.zeros((18, ld)); f = np.zeros((12, ld)); ct = np.zeros(ld, np.uint8); fl = np.zeros(ld, np.int32)
    if out is not None:
        vd, f, ct, fl = out["vdot"], out["force"], out["contact"], out["flags"]
        assert vd.shape == (18, ld) and f.shape == (12, ld) and vd.dtype == f.dtype == np.float64
        assert ct.dtype == np.uint8 and fl.dtype == np.int32 and all(a.flags.c_contiguous for a in (vd, f, ct, fl))
    for a, rows in ((tau, 12), (we, 6), (cn, 4)):
        assert a is None or a.shape == (rows, ld)
    rc = entry(_p(flat), _p(qp), _p(ap), _p(pr), n, ld, 0 if dt is None else 1, int(substeps), 0.0 if dt is None else float(dt),
               _p(q), _p(v), _p(tm), _p(tau), _p(mu), _p(ms), _p(we), _p(vd), _p(f), _p(ct), _p(fl), _p(cn), *tail)
    assert rc > 0, rc
    out = dict(vdot=vd, force=f, contact=ct, flags=fl)
    if dt is not None:
        out.update(q=q, v=v, time=tm, counts=cn, substeps=rc)
    return out


def run(flat, q, v, tau, mu=None, mass_scale=None, ext_wrench=None, params=None, q_perm=None, act_perm=None, dt=None, substeps=0,
        time=None, counts=None, n=None, out=None):
    """One force evaluation (dt None) or one step of `substeps` substeps (0: ceil(dt / max_substep)).  params: a dict overriding
    defaults(flat).  Returns dict(vdot, force, contact, flags[, q, v, time, counts, substeps]) -- copies, inputs untouched.
    n: the batch size where the arrays are wider (ld = q.shape[1] > n; every 2-D array then has ld columns).  out: a dict of
    preset vdot / force / contact / flags arrays to write into (for looking at what is left of the padding columns)."""
    return call(lib().host_ground_batch, (), flat, q, v, tau, mu, mass_scale, ext_wrench, params, q_perm, act_perm, dt, substeps, time,
                counts, n, out)
