"""ctypes view of host_follow_batch of tools/libhost_ground.so: the follow law of csrc/wbc_ground_follow.hpp instantiated on the
host (tests only).  run() takes the terrain as GroundContactPlant.set_terrain takes it and the targets as follow_targets does."""
import ctypes as C

import numpy as np

import host_ground as hg
from quadruped_drake_amd import terrain as tr

MODES = {"off": 0, "lift": 1, "fit": 2}


def run(profiles, targets, mode="fit", terrain_id=None, terrain_scale=None, n=None):
    """-> the followed copy of targets [54, ld] (n: the batch size where the array is wider); profiles None: no terrain."""
    L = hg.lib()
    L.host_follow_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    out = np.array(targets, dtype=np.float64, order="C")
    assert out.ndim == 2 and out.shape[0] == 54
    ld = out.shape[1]
    n = ld if n is None else n
    ts = hg._f64(terrain_scale)
    ti = None if terrain_id is None else np.ascontiguousarray(terrain_id, dtype=np.uint8)
    for a in (ts, ti):
        assert a is None or a.shape[0] >= n
    arr, count = (None, 0) if not profiles else (tr.c_array(profiles), len(profiles))
    rc = L.host_follow_batch(None if arr is None else C.cast(arr, C.c_void_p), count, hg._p(ti), hg._p(ts), n, ld,
                             MODES[mode] if isinstance(mode, str) else int(mode), hg._p(out))
    assert rc == 0, rc
    return out
