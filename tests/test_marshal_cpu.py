"""The Python layer's one handle base and one tensor marshaller (quadruped_drake_amd/_lib.py: Handle, dev_ptr, new_out, outputs), as far
as they can be pinned without a device: what the marshaller refuses before it takes a pointer, the controller's host-pointer branch, the
lifetime of an object that never ran its __init__, and where in the package raw pointers, streams and finalisers may be written."""
import ctypes as C
import gc
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

from quadruped_drake_amd import _lib, controller, gait, plant, trajectory

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HANDLE_CLASSES = [(controller.IDController, "wbc_destroy"), (plant.RigidContactPlant, "wbc_plant_destroy"),
                  (plant.GroundContactPlant, "wbc_ground_destroy"), (gait.GaitPlanner, "wbc_gait_destroy"),
                  (trajectory.TrunkTrajectory, "wbc_traj_destroy")]


def test_the_marshaller_refuses_before_it_takes_a_pointer():
    import torch
    cpu = torch.zeros((19, 3), dtype=torch.float64)
    with pytest.raises(ValueError, match="q is required"):
        _lib.dev_ptr(None, 19, 3, "float64", "q", 0, "the plant")
    assert _lib.dev_ptr(None, 0, 3, "float64", "mu", 0, "the plant", True) is None
    for what in (np.zeros((19, 3)), [[0.0] * 3] * 19, 1.0, cpu):                      # no tensor; a tensor, but not on a GPU
        with pytest.raises(ValueError, match="q: expected a contiguous CUDA tensor of dtype torch.float64"):
            _lib.dev_ptr(what, 19, 3, "float64", "q", 0, "the plant")
        with pytest.raises(ValueError, match="q: expected a contiguous CUDA tensor"):
            _lib.dev_ptr(what, 19, 3, "float64", "q", 0, "the plant", True)            # optional: absent is fine, wrong is not
    # the wrappers of the owners are the same function under their owner word
    for ptr in (plant._dev_ptr, gait._dev_ptr):
        assert ptr(None, 0, 3, "float64", "mu", 0, True) is None
        with pytest.raises(ValueError, match="tau is required"):
            ptr(None, 12, 3, "float64", "tau", 0)
        with pytest.raises(ValueError, match="tau: expected"):
            ptr(cpu, 12, 3, "float64", "tau", 0)
    # a caller's `out`: as many tensors as the set has, each checked like an input
    with pytest.raises(ValueError, match="out: expected \\(targets, contact_mask\\)"):
        _lib.outputs((cpu,), _lib.TARGET_OUTS, 3, 0, "the planner")
    with pytest.raises(ValueError, match="targets: expected a contiguous CUDA tensor"):
        _lib.outputs((cpu, cpu), _lib.TARGET_OUTS, 3, 0, "the planner")
    # and the device-pointer controller's thin wrapper over it
    c = object.__new__(controller.IDController)
    c.host_ptrs, c.device = False, 0
    assert c._ptr(None, 0, 3, "float64", "mu", optional=True) == (None, None)
    for bad in (None, np.zeros((19, 3)), cpu):
        with pytest.raises(ValueError, match="q"):
            c._ptr(bad, 19, 3, "float64", "q")
    with pytest.raises(ValueError, match="tau: expected"):
        c._outs((cpu[:12], cpu[:4], cpu[0]), _lib.TICK_OUTS, 3)


def test_the_controller_s_host_pointer_branch_converts_what_numpy_converts():
    c = object.__new__(controller.IDController)
    c.host_ptrs, c.device = True, 0
    with pytest.raises(ValueError, match="q is required"):
        c._ptr(None, 19, 3, "float64", "q")
    assert c._ptr(None, 0, 3, "float64", "mu", optional=True) == (None, None)
    for shape in ((19, 2), (18, 3), (3, 19), (57,)):
        with pytest.raises(ValueError, match="q: expected shape \\(19, 3\\), got"):
            c._ptr(np.zeros(shape), 19, 3, "float64", "q")
    with pytest.raises(ValueError, match="contact_mask: expected shape \\(3,\\)"):
        c._ptr(np.zeros((1, 3), np.uint8), 0, 3, "uint8", "contact_mask")
    rows = [[float(10 * r + k) for k in range(3)] for r in range(19)]
    arr, p = c._ptr(rows, 19, 3, "float64", "q")                                     # a list of lists
    assert isinstance(arr, np.ndarray) and arr.dtype == np.float64 and arr.flags.c_contiguous and arr.tolist() == rows
    assert isinstance(p, C.c_void_p) and p.value == arr.ctypes.data
    arr, p = c._ptr([1, 0, 15], 0, 3, "uint8", "contact_mask")
    assert arr.dtype == np.uint8 and arr.tolist() == [1, 0, 15] and p.value == arr.ctypes.data
    f = np.asfortranarray(np.arange(57.0).reshape(19, 3))                            # not contiguous: copied, the copy is what is kept
    arr, p = c._ptr(f, 19, 3, "float64", "q")
    assert arr.flags.c_contiguous and (arr == f).all() and p.value == arr.ctypes.data and arr is not f
    ok = np.arange(57.0).reshape(19, 3)
    arr, p = c._ptr(ok, 19, 3, "float64", "q")                                       # already right: taken as it is
    assert arr is ok and p.value == ok.ctypes.data
    # fresh outputs are zeroed numpy arrays; a caller's are converted like inputs, and counted
    outs, ptrs = c._outs(None, _lib.TICK_OUTS, 3)
    assert [(a.shape, a.dtype) for a in outs] == [((12, 3), np.float64), ((4, 3), np.float64), ((3,), np.int32)]
    assert all(not a.any() for a in outs) and [p.value for p in ptrs] == [a.ctypes.data for a in outs]
    mine = (np.ones((12, 3)), np.ones((4, 3)), np.ones(3, np.int32))
    outs, ptrs = c._outs(mine, _lib.TICK_OUTS, 3)
    assert all(a is b for a, b in zip(outs, mine)) and [p.value for p in ptrs] == [a.ctypes.data for a in mine]
    with pytest.raises(ValueError):
        c._outs(mine[:2], _lib.TICK_OUTS, 3)
    with pytest.raises(ValueError, match="metrics: expected shape \\(4, 3\\)"):
        c._outs((mine[0], np.ones((4, 2)), mine[2]), _lib.TICK_OUTS, 3)


class _Recorder:
    """A stand-in library that records every call"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *args: self.calls.append((name, args)) or 0


@pytest.mark.parametrize("cls,destroy", HANDLE_CLASSES, ids=[c.__name__ for c, _ in HANDLE_CLASSES])
def test_an_object_that_never_ran_its_init_closes_twice_and_goes_quietly(cls, destroy, monkeypatch):
    unraisable = []
    monkeypatch.setattr(sys, "unraisablehook", unraisable.append)
    assert issubclass(cls, _lib.Handle) and cls._destroy == destroy
    o = object.__new__(cls)
    assert o._h is None and o._L is None and o._n is None and o._keep is None and o._terrain is None and o._follow == "off"
    if cls is gait.GaitPlanner:
        assert o.has_terrain is False and o.has_schedule is False and o.has_feedback is False
    o.close()
    o.close()
    del o
    gc.collect()
    assert unraisable == []
    # with a handle: its own wbc_*_destroy once, however often it is closed, and what a subclass holds beside it is let go
    o = object.__new__(cls)
    o._L, o._h = _Recorder(), C.c_void_p(64)
    o._keep, o._terrain, o._schedule, o._feedback = ("kept",), ([], None, None, None), ("s",), (4, {})
    L = o._L
    o.close()
    o.close()
    assert [name for name, _ in L.calls] == [destroy] and L.calls[0][1][0].value == 64 and o._h is None
    if cls is gait.GaitPlanner:
        assert (o._keep, o._terrain, o._schedule, o._feedback) == (None,) * 4 and not (o.has_terrain or o.has_schedule or o.has_feedback)
    if cls is plant.GroundContactPlant:
        assert o._terrain is None
    del o
    gc.collect()
    assert len(L.calls) == 1 and unraisable == []
    # a finaliser swallows what its library raises (an interpreter that is shutting down has taken the library away)
    o = object.__new__(cls)
    o._L, o._h = None, C.c_void_p(64)
    with pytest.raises(AttributeError):
        o.close()
    del o
    gc.collect()
    assert unraisable == []


def test_raw_pointers_streams_and_finalisers_are_written_in_one_module():
    counts = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "quadruped_drake_amd", "*.py"))):
        text = open(path).read()
        counts[os.path.basename(path)] = [text.count(s) for s in ("data_ptr(", "current_stream(", "def __del__", 'getattr(self, "_')]
    assert len(counts) >= 13 and "_lib.py" in counts
    assert counts.pop("_lib.py") == [2, 1, 1, 0]        # dev_ptr and the fresh tensors of outputs; stream_of; Handle.__del__
    assert all(c == [0, 0, 0, 0] for c in counts.values()), counts


def test_importing_the_package_does_not_import_torch():
    r = subprocess.run([sys.executable, "-c", "import sys, quadruped_drake_amd; assert 'torch' not in sys.modules"], cwd=ROOT,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
