"""ctypes view of host_terrain_batch of tools/libhost_ground.so: the compliant-ground plant math of csrc/wbc_ground.hpp with its
TERRAIN instantiation on the host (tests only).  run() takes what host_ground.run takes, and the terrain as
GroundContactPlant.set_terrain takes it."""
import ctypes as C

import numpy as np

import host_ground as hg
from quadruped_drake_amd import terrain as tr

PARAM_NAMES = hg.PARAM_NAMES
defaults = hg.defaults
lib = hg.lib


def run(flat, q, v, tau, mu=None, mass_scale=None, ext_wrench=None, params=None, q_perm=None, act_perm=None, dt=None, substeps=0,
        time=None, counts=None, n=None, profiles=None, terrain_id=None, terrain_scale=None):
    """One force evaluation (dt None) or one step of `substeps` substeps (0: ceil(dt / max_substep)) on the terrain `profiles` (a
    list of terrain.Profile; None: no terrain), instance i on profile terrain_id[i] (default 0) scaled by terrain_scale[i]
    (default 1).  Returns dict(vdot, force, contact, flags[, q, v, time, counts, substeps]) -- copies, inputs untouched."""
    ld = np.shape(q)[1]
    ts = hg._f64(terrain_scale)
    ti = None if terrain_id is None else np.ascontiguousarray(terrain_id, dtype=np.uint8)
    for a in (mu, mass_scale, ts, ti):
        assert a is None or np.shape(a) == (ld,)
    arr, count = (None, 0) if not profiles else (tr.c_array(profiles), len(profiles))
    tail = (None if arr is None else C.cast(arr, C.c_void_p), count, hg._p(ti), hg._p(ts))
    return hg.call(lib().host_terrain_batch, tail, flat, q, v, tau, mu, mass_scale, ext_wrench, params, q_perm, act_perm, dt, substeps,
                   time, counts, n, None)
