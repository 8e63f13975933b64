"""ctypes binding of libwbc_hip.so (include/wbc.h).  No fallback: if the HIP library is missing or a
call fails, this raises -- the product has no CPU path."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("WBC_HIP_LIB", os.path.join(_HERE, "libwbc_hip.so"))  # override = A/B kernel builds

c_double_p = C.POINTER(C.c_double)
c_u8_p = C.POINTER(C.c_uint8)
c_i32_p = C.POINTER(C.c_int32)

KIND_ID, KIND_MPTC, KIND_PC, KIND_CLF = 0, 1, 2, 3
DEVICE_PTRS, HOST_PTRS = 0, 1

class WbcModel(C.Structure):
    _fields_ = [("flat", C.c_double * 215), ("q_perm", C.c_int32 * 12), ("act_perm", C.c_int32 * 12)]


class WbcParams(C.Structure):
    _fields_ = [(k, C.c_double) for k in
                ("Kp_body_p", "Kd_body_p", "Kp_body_rpy", "Kd_body_rpy", "Kp_foot", "Kd_foot",
                 "w_body", "w_foot", "mu", "Kd_contact", "tau_max", "eps2")]


class WbcStats(C.Structure):
    _fields_ = [("ticks", C.c_double), ("status_nonzero", C.c_double), ("iters_sum", C.c_double),
                ("tau_abs_sum", C.c_double), ("tau_abs_max", C.c_double), ("err_sum", C.c_double),
                ("mask_count", C.c_double * 16)]


class WbcTrunkState(C.Structure):
    _fields_ = [("timestamp", C.c_double), ("finished", C.c_uint8),
                ("base_p", C.c_double * 3), ("base_pd", C.c_double * 3), ("base_pdd", C.c_double * 3),
                ("base_rpy", C.c_double * 3), ("base_rpyd", C.c_double * 3), ("base_rpydd", C.c_double * 3),
                ("foot_p", (C.c_double * 3) * 4), ("foot_pd", (C.c_double * 3) * 4), ("foot_pdd", (C.c_double * 3) * 4),
                ("contact", C.c_uint8 * 4), ("foot_f", (C.c_double * 3) * 4)]


class WbcRobotState(C.Structure):
    _fields_ = [("q", C.c_float * 19), ("v", C.c_float * 18), ("tau", C.c_float * 12)]


class WbcPlantParams(C.Structure):
    _fields_ = [("Kd_contact", C.c_double), ("tau_max", C.c_double), ("mu", C.c_double)]


class WbcGroundParams(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("stiffness", "dissipation", "mu", "v_stiction", "foot_radius", "tau_max", "max_substep",
                                          "fall_height")]


class WbcTerrainProfile(C.Structure):
    _fields_ = [("nk", C.c_int), ("x0", C.c_double), ("y0", C.c_double), ("yaw", C.c_double), ("s", C.c_double * 8),
                ("h", C.c_double * 8)]


class WbcGaitStride(C.Structure):
    _fields_ = [("nphase", C.c_int), ("duration", C.c_double * 8), ("contact", C.c_uint8 * 8)]


class WbcGaitParams(C.Structure):
    _fields_ = [("stance", (C.c_double * 2) * 4), ("height", C.c_double), ("swing_height", C.c_double), ("ramp_time", C.c_double),
                ("wait_time", C.c_double)]


class WbcGaitTerrainParams(C.Structure):
    _fields_ = [("body_mode", C.c_int), ("max_grade", C.c_double), ("edge_margin", C.c_double), ("apex_max", C.c_double)]


class WbcGaitFeedbackParams(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("k_v", "k_p", "d_max", "u_hold")]


_P, _I, _D = C.c_void_p, C.c_int, C.c_double
_IP, _FP, _HP = C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_void_p)
_MODEL, _PARAMS, _STATS = C.POINTER(WbcModel), C.POINTER(WbcParams), C.POINTER(WbcStats)
_TRUNK, _ROBOT = C.POINTER(WbcTrunkState), C.POINTER(WbcRobotState)
_PLANTP, _GROUNDP = C.POINTER(WbcPlantParams), C.POINTER(WbcGroundParams)
_GAITP, _GAITS, _GAITTP = C.POINTER(WbcGaitParams), C.POINTER(WbcGaitStride), C.POINTER(WbcGaitTerrainParams)
_GAITFP = C.POINTER(WbcGaitFeedbackParams)

# name: (restype, argtypes) of every function the headers of include/ declare, one position per argument in the header's order
# (tests/test_abi_cpu.py lays each row beside the header's prototype).  A handle, a stream and a device array are _P.
PROTOTYPES = {
    # wbc.h: the controller interface
    "wbc_last_error": (C.c_char_p, []),
    "wbc_version": (_I, []),
    "wbc_params_default": (_I, [_I, _PARAMS]),
    "wbc_create": (_I, [_MODEL, _I, _PARAMS, _I, _I, C.c_uint32, _HP]),
    "wbc_destroy": (_I, [_P]),
    "wbc_set_stream": (_I, [_P, _P]),
    "wbc_step": (_I, [_P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "wbc_sync": (_I, [_P]),
    "wbc_time_steps": (_I, [_P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _FP]),
    "wbc_time_steps_result": (_I, [_P, _FP]),
    "wbc_time_steps_each": (_I, [_P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _FP]),
    "wbc_stats_get": (_I, [_P, _STATS]),
    "wbc_stats_reset": (_I, [_P]),
    "wbc_stats_pack": (_I, [_P, c_double_p]),
    "wbc_stats_reduce": (_I, [c_double_p, _I, _STATS]),
    "wbc_set_vdot_output": (_I, [_P, _P]),
    "wbc_integrate": (_I, [_P, _I, _I, _D, _P, _P, _P]),
    "wbc_rollout": (_I, [_P, _P, _I, _D, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "wbc_set_warm_start": (_I, [_P, _I]),
    "wbc_set_variant": (_I, [_P, _I]),
    "wbc_variant_for": (_I, [_P, _I]),
    "wbc_kernel_info": (_I, [_P, _IP, _IP, _IP, _IP]),
    "wbc_rollout_kernel_info": (_I, [_P, _IP, _IP, _IP, _IP]),
    "wbc_trunk_state_decode": (_I, [C.c_char_p, C.c_size_t, _TRUNK]),
    "wbc_trunk_state_to_targets": (_I, [_TRUNK, c_double_p, c_u8_p]),
    "wbc_traj_create": (_I, [_I, _I, c_double_p, c_double_p, c_u8_p, c_double_p, C.c_uint8, _D, _HP]),
    "wbc_traj_destroy": (_I, [_P]),
    "wbc_traj_lookup": (_I, [_P, _P, _I, _I, _P, _P, _P]),
    # wbc_extras.h: frozen out-of-scope exports
    "wbc_robot_state_decode": (_I, [C.c_char_p, C.c_size_t, _ROBOT]),
    "wbc_robot_state_encode": (_I, [_ROBOT, C.c_char_p, C.c_size_t]),
    "wbc_robot_states_unpack": (_I, [_I, _P, _I, _I, _P, _P, _P, _P]),
    "wbc_robot_controls_pack": (_I, [_I, _P, _I, _I, _P, _IP, _IP, _P]),
    "wbc_pd_step": (_I, [_I, _P, _I, _I, _P, _P, c_double_p, _D, _D, _D, _IP, _IP, _P]),
    # wbc_plant.h: the rigid-contact plant
    "wbc_plant_params_default": (_I, [_PLANTP]),
    "wbc_plant_create": (_I, [_MODEL, _PLANTP, _I, _HP]),
    "wbc_plant_destroy": (_I, [_P]),
    "wbc_plant_forward": (_I, [_P, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "wbc_plant_step": (_I, [_P, _P, _I, _I, _D, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "wbc_plant_rollout": (_I, [_P, _P, _P, _P, _I, _D, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "wbc_plant_kernel_info": (_I, [_P, _IP, _IP, _IP, _IP]),
    # wbc_ground.h: the compliant-ground plant, its terrain and the follow law
    "wbc_ground_params_default": (_I, [_MODEL, _GROUNDP]),
    "wbc_ground_create": (_I, [_MODEL, _GROUNDP, _I, _HP]),
    "wbc_ground_destroy": (_I, [_P]),
    "wbc_ground_forward": (_I, [_P, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "wbc_ground_step": (_I, [_P, _P, _I, _I, _D, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "wbc_ground_rollout": (_I, [_P, _P, _P, _P, _I, _D, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "wbc_ground_kernel_info": (_I, [_P, _IP, _IP, _IP, _IP]),
    "wbc_terrain_check": (_I, [_P, _I]),
    "wbc_ground_set_terrain": (_I, [_P, _P, _I, _P, _P]),
    "wbc_ground_terrain_kernel_info": (_I, [_P, _IP, _IP, _IP, _IP]),
    "wbc_ground_follow_targets": (_I, [_P, _P, _I, _I, _I, _P]),
    "wbc_ground_set_follow": (_I, [_P, _I]),
    "wbc_ground_follow_kernel_info": (_I, [_P, _IP, _IP, _IP, _IP]),
    # wbc_gait.h: the gait planner
    "wbc_gait_check": (_I, [_GAITP, _GAITS, _I]),
    "wbc_gait_create": (_I, [_GAITP, _GAITS, _I, _I, _HP]),
    "wbc_gait_destroy": (_I, [_P]),
    "wbc_gait_set_commands": (_I, [_P, _P, _P, _P, _P]),
    "wbc_gait_targets": (_I, [_P, _P, _I, _I, _P, _P, _P]),
    "wbc_gait_kernel_info": (_I, [_P, _IP, _IP, _IP, _IP]),
    "wbc_ground_set_gait": (_I, [_P, _P]),
    "wbc_plant_set_gait": (_I, [_P, _P]),
    # wbc_gait_terrain.h: the gait planner's terrain
    "wbc_gait_terrain_check": (_I, [_GAITTP, _P, _I]),
    "wbc_gait_set_terrain": (_I, [_P, _GAITTP, _P, _I, _P, _P]),
    "wbc_gait_terrain_kernel_info": (_I, [_P, _IP, _IP, _IP, _IP]),
    # wbc_gait_schedule.h: the gait planner's command schedules
    "wbc_gait_set_schedule": (_I, [_P, _P, _I, _I, _D, _P, _P, _P]),
    "wbc_gait_clear_schedule": (_I, [_P]),
    "wbc_gait_schedule_kernel_info": (_I, [_P, _I, _IP, _IP, _IP, _IP]),
    # wbc_gait_feedback.h: the gait planner's foot-placement feedback
    "wbc_gait_feedback_check": (_I, [_GAITFP]),
    "wbc_gait_feedback_params_default": (_I, [_GAITP, _GAITFP]),
    "wbc_gait_set_feedback": (_I, [_P, _GAITFP, _I]),
    "wbc_gait_clear_feedback": (_I, [_P]),
    "wbc_gait_targets_measured": (_I, [_P, _P, _I, _I, _P, _P, _P, _P, _P, _P]),
    "wbc_gait_feedback_kernel_info": (_I, [_P, _IP, _IP, _IP, _IP]),
}
SYMBOLS = list(PROTOTYPES)
# the names newer than the oldest kernel build still timed against (A/B timing: WBC_HIP_LIB; tools/qt.py --lib): the statistics
# exchange, the follow law, the gait planner, its terrain, its command schedules and its foot-placement feedback
_NEWER = ("wbc_stats_pack", "wbc_stats_reduce", "wbc_ground_follow_targets", "wbc_ground_set_follow", "wbc_ground_follow_kernel_info",
          "wbc_gait_check", "wbc_gait_create", "wbc_gait_destroy", "wbc_gait_set_commands", "wbc_gait_targets", "wbc_gait_kernel_info",
          "wbc_ground_set_gait", "wbc_plant_set_gait", "wbc_gait_terrain_check", "wbc_gait_set_terrain", "wbc_gait_terrain_kernel_info",
          "wbc_gait_set_schedule", "wbc_gait_clear_schedule", "wbc_gait_schedule_kernel_info", "wbc_gait_feedback_check",
          "wbc_gait_feedback_params_default", "wbc_gait_set_feedback", "wbc_gait_clear_feedback", "wbc_gait_targets_measured",
          "wbc_gait_feedback_kernel_info")
# what a library may lack: any library the terrain, a library under A/B timing the newer names too
_MAY_LACK = ("wbc_terrain_check", "wbc_ground_set_terrain", "wbc_ground_terrain_kernel_info") + (_NEWER if "WBC_HIP_LIB" in os.environ else ())


class WbcError(RuntimeError):
    pass


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise WbcError("HIP extension %s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback)" % LIB_PATH)
        # ONE HIP runtime per process: libwbc_hip.so is linked against libamdhip64.so by soname and PyTorch-ROCm ships its own copy.
        # Loaded after torch, the library binds to the copy torch already mapped; loaded BEFORE it (build() then smoke() in one
        # process) the system copy comes in first, torch then maps its own, and the second runtime finds no device.  Device memory
        # and streams are torch's here anyway, so torch goes first whenever it is installed.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        l = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in PROTOTYPES.items():
            if not (name in _MAY_LACK and not hasattr(l, name)):
                fn = getattr(l, name)
                fn.restype, fn.argtypes = restype, argtypes
        _lib = l
    return _lib


def check(rc):
    if rc != 0:
        raise WbcError("libwbc_hip: rc=%d: %s" % (rc, lib().wbc_last_error().decode()))


def fill_model(table, q_perm=None, act_perm=None):
    """The wbc_model of a model table; q_perm None: the identity, act_perm None: the table's own."""
    m = WbcModel()
    assert len(table["flat"]) == 215
    m.flat[:] = [float(x) for x in table["flat"]]
    m.q_perm[:] = list(range(12)) if q_perm is None else [int(x) for x in q_perm]
    m.act_perm[:] = [int(x) for x in (table.get("act_perm", range(12)) if act_perm is None else act_perm)]
    return m


def dev_ptr(a, rows, n, dtype, name, device, owner, optional=False):
    """Pointer to a contiguous CUDA tensor of the dtype torch and numpy call `dtype` ("float64", "uint8", "int32") and shape [rows, n]
    ([n] when rows is 0) on cuda:`device`, where `owner` ("the plant", "this controller's handle") lives; None for an absent optional
    tensor."""
    import torch
    if a is None:
        if optional:
            return None
        raise ValueError(name + " is required")
    tdt = getattr(torch, dtype)
    if not (isinstance(a, torch.Tensor) and a.is_cuda and a.dtype == tdt and a.is_contiguous()):
        raise ValueError("%s: expected a contiguous CUDA tensor of dtype %s" % (name, tdt))
    if a.device.index != device:
        raise ValueError("%s: tensor lives on cuda:%s, %s on cuda:%d" % (name, a.device.index, owner, device))
    if tuple(a.shape) != ((rows, n) if rows else (n,)):
        raise ValueError("%s: expected shape %s, got %s" % (name, (rows, n) if rows else (n,), tuple(a.shape)))
    return C.c_void_p(a.data_ptr())


def new_out(rows, n, dtype, device, zero=False):
    """A fresh output tensor of `dtype` (a name, as dev_ptr takes it) and shape [rows, n] ([n] when rows is 0) on `device`; zeroed where
    the caller may see it unwritten."""
    import torch
    return (torch.zeros if zero else torch.empty)((rows, n) if rows else (n,), dtype=getattr(torch, dtype), device=device)


def outputs(out, specs, n, device, owner, zero=False):
    """The caller's `out` or fresh tensors -> (tensors, pointers).  specs: (rows, dtype, name) per tensor, in the order of `out`.  The
    caller's tensors are checked as dev_ptr checks them; fresh ones live on cuda:`device`, zeroed if `zero`."""
    if out is None:
        ts = tuple(new_out(rows, n, dtype, device, zero) for rows, dtype, _ in specs)
        return ts, [C.c_void_p(t.data_ptr()) for t in ts]
    ts = tuple(out)
    if len(ts) != len(specs):
        raise ValueError("out: expected (%s)" % ", ".join(name for _, _, name in specs))
    return ts, [dev_ptr(t, rows, n, dtype, name, device, owner) for t, (rows, dtype, name) in zip(ts, specs)]


# the output sets more than one module allocates, as `outputs` takes them
TICK_OUTS = ((12, "float64", "tau"), (4, "float64", "metrics"), (0, "int32", "status"))
TARGET_OUTS = ((54, "float64", "targets"), (0, "uint8", "contact_mask"))


_torch = None


def stream_of(device):
    """torch's current stream on cuda:`device`, as the integer hipStream_t.  Every tick asks: the module is looked up once."""
    global _torch
    if _torch is None:
        import torch as _torch
    return _torch.cuda.current_stream(device).cuda_stream


def kernel_info(fn, handle):
    """The answer of a wbc_*_kernel_info entry point as a dict"""
    a, b, c, d = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    check(fn(handle, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
    return dict(num_regs=a.value, scratch_bytes_per_lane=b.value, lds_bytes=c.value, block_threads=d.value)


class Handle:
    """What the owners of a wbc_* handle share: the bound library `_L`, the handle `_h` and its device, the handle's lifetime, torch's
    stream, kernel_info's answer.  A subclass names its wbc_*_destroy in `_destroy` and sets _L, _h and device in its __init__; the state
    some of them add starts out absent here, so an object that never ran its __init__ answers like one that set nothing."""
    _destroy = None
    _L = _h = device = None
    _keep = None                            # the controller's and the planner's: the tensors of the last call, kept alive
    _terrain = None                         # GroundContactPlant's and GaitPlanner's: what set_terrain stored
    _follow = "off"                         # GroundContactPlant's: set_follow's mode
    _n = _schedule = _feedback = None       # GaitPlanner's: set_commands' N, set_schedule's arrays, set_feedback's (n, parameters)

    def close(self):
        if self._h:
            getattr(self._L, self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return C.c_void_p(stream_of(self.device))

    def _kernel_info(self, entry_point):
        return kernel_info(getattr(self._L, entry_point), self._h)
