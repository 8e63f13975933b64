"""ctypes view of tools/libhost_tick.so: the kernel math instantiated on the host (tests only)."""
import ctypes as C
import os
import subprocess

import numpy as np

import __graft_entry__ as graft

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = None
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_mp = C.POINTER(C.c_ubyte)
_V, _I, _D = C.c_void_p, C.c_int, C.c_double
# kind, flat215, params12, q_perm, act_perm, n, stride, q, v, tg, mask, mu, mass_scale, tau, met, status, iters
_TICK = [_I, _dp, _dp, _ip, _ip, _I, _I, _dp, _dp, _dp, _mp, _dp, _dp, _dp, _dp, _ip, _ip]
# name: (restype, argtypes), after tools/host_tick.cpp
_PROTOTYPES = {
    "host_tick_batch": (_I, _TICK),
    "host_tick_count": (_I, [_I, _dp, _dp, _I, _I, _dp, _dp, _dp, _mp, _dp, _dp, _dp]),
    "host_set_vdot_sink": (None, [_V]),
    "host_hex_batch": (_I, _TICK),
    "host_gi_dump": (None, [_V]),
    "host_gi_adds": (None, [_V]),
    "host_gi_force_bail": (None, [_I]),
    "host_gi_stats": (None, [_ip, _I]),
    "host_hex_rollout": (_I, [_I, _dp, _dp, _I, _I, _I, _D, _I, _dp, _dp, _dp, _mp, _dp, _dp, _dp, _dp, _ip, _dp, _ip]),
    "host_traj_index": (_I, [_dp, _I, _D, _D, _I]),
}


def bind(path):
    """The library at `path` with the prototypes above; a -DHOST_TICK_HEX_ONLY build (build_variant) exports the hex half of them only."""
    l = C.CDLL(path)
    for name, (restype, argtypes) in _PROTOTYPES.items():
        if hasattr(l, name):
            fn = getattr(l, name)
            fn.restype, fn.argtypes = restype, argtypes
    return l


def lib():
    global _LIB
    if _LIB is None:
        _LIB = bind(graft.build_target("host_tick"))
    return _LIB


_default = lib


def build_variant(tmp_path, name, flags, compiler=None):
    """A host instantiation of the kernel headers with the CLOSED alternatives available again (the -DWBC_... switches that round 6 removed from
    the product source: tools/lab/patches/closed_switches.patch re-introduces them): the sources are copied to `tmp_path`, patched there and
    compiled with `flags` and -DHOST_TICK_HEX_ONLY.  Without flags the patched tree is the product's code, so a comparison against the default build is a comparison
    against what ships.  Returns the loaded library."""
    import shutil
    tree = os.path.join(str(tmp_path), "tree_" + name)
    for sub in ("quadruped_drake_amd/csrc", "tools", "include"):
        os.makedirs(os.path.join(tree, sub), exist_ok=True)
    for f in os.listdir(os.path.join(_ROOT, "quadruped_drake_amd", "csrc")):
        shutil.copy(os.path.join(_ROOT, "quadruped_drake_amd", "csrc", f), os.path.join(tree, "quadruped_drake_amd", "csrc", f))
    for f in ("host_tick.cpp", "wbc_scalar_tick.hpp"):
        shutil.copy(os.path.join(_ROOT, "tools", f), os.path.join(tree, "tools", f))
    for f in os.listdir(os.path.join(_ROOT, "include")):
        shutil.copy(os.path.join(_ROOT, "include", f), os.path.join(tree, "include", f))
    subprocess.check_call(["patch", "-p1", "-s", "--no-backup-if-mismatch", "-i", os.path.join(_ROOT, "tools", "lab", "patches", "closed_switches.patch")], cwd=tree)
    so = os.path.join(str(tmp_path), name)
    # HOST_TICK_HEX_ONLY: the 16-lane emulation alone (host_hex_batch is all a variant is asked) -- half the compile time of the full tool
    graft.host_shared(so, [os.path.join(tree, "tools", "host_tick.cpp")], ["-pthread", "-DHOST_TICK_HEX_ONLY"] + list(flags), compiler)
    return bind(so)


def _p(a, dtype=np.float64):
    """`a` (or None) as the contiguous array of `dtype` the ABI reads and the pointer to it; the array must outlive the call."""
    if a is None:
        return None, None
    a = np.ascontiguousarray(a, dtype=dtype)
    return a, a.ctypes.data_as({np.float64: _dp, np.int32: _ip, np.uint8: _mp}[dtype])


def _batch(kind, flat, q, v, targets, mask, mu, mass_scale):
    """What run and count marshal alike: the law's number, n, the arrays kept alive, and the pointers flat | q, v, targets, mask, mu, mass_scale."""
    k = {"id": 0, "mptc": 1, "pc": 2, "clf": 3}[kind.lower()] if isinstance(kind, str) else int(kind)
    pairs = [_p(a) for a in (flat, q, v, targets)] + [_p(mask, np.uint8), _p(mu), _p(mass_scale)]
    ptrs = [p for _, p in pairs]
    return k, pairs[1][0].shape[1], pairs, ptrs[0], ptrs[1:]


def run(kind, flat, q, v, targets, mask, mu=None, mass_scale=None, params12=None, q_perm=None, act_perm=None,
        want_vdot=False, hexv=False, lib=None):
    """One batch through host_tick_batch (hexv: host_hex_batch) of `lib` (None: the default build) -> tau, met, status, iters[, vdot]"""
    L = _default() if lib is None else lib
    k, n, _keep, flat_p, batch_p = _batch(kind, flat, q, v, targets, mask, mu, mass_scale)
    tau = np.zeros((12, n)); met = np.zeros((4, n)); st = np.zeros(n, np.int32); it = np.zeros(n, np.int32)
    extra = [_p(params12), _p(q_perm, np.int32), _p(act_perm, np.int32)]
    vdot = np.zeros((18, n)) if want_vdot else None
    if want_vdot:                                    # (a HEX_ONLY variant has no sink)
        L.host_set_vdot_sink(vdot.ctypes.data_as(C.c_void_p))
    fn = L.host_hex_batch if hexv else L.host_tick_batch
    try:
        rc = fn(k, flat_p, *[p for _, p in extra], n, n, *batch_p, _p(tau)[1], _p(met)[1], _p(st, np.int32)[1], _p(it, np.int32)[1])
    finally:
        if want_vdot:
            L.host_set_vdot_sink(None)
    assert rc == 0
    return (tau, met, st, it, vdot) if want_vdot else (tau, met, st, it)


def count(kind, flat, q, v, targets, mask, mu=None, mass_scale=None):
    k, n, _keep, flat_p, batch_p = _batch(kind, flat, q, v, targets, mask, mu, mass_scale)
    out = np.zeros(6)
    rc = lib().host_tick_count(k, flat_p, None, n, n, *batch_p, _p(out)[1])
    assert rc == 0
    return dict(zip(["add", "mul", "div", "sqrt", "trig", "cmp"], out))
