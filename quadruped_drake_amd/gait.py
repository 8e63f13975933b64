"""Gait planner on the device (include/wbc_gait.h): walking targets from a velocity command.

The reference gets its walking `trunk_input` from TOWR, which is out of scope here.  As far as the controllers see it, that is a
contact schedule, footholds, swing splines and a base motion.  The schedule is data -- TOWR's stride tables, restated in `STRIDES`
-- and once the base follows a commanded velocity the rest has a closed form (the law: the head of include/wbc_gait.h).
`GaitPlanner` evaluates it per instance on the GPU: every robot of a batch has its own command (vx, vy, yaw rate), its own stride
and its own stride period, and no table of samples.  `plant.closed_loop` takes a GaitPlanner where it takes a trajectory.
`GaitPlanner.set_terrain` gives the planner the plant's terrain (include/wbc_gait_terrain.h): its targets are then the
finished targets on that ground -- footholds off the risers, swings that clear the knots, a body that follows the feet -- and no
follow pass runs after them.
`GaitPlanner.set_schedule` steers it (include/wbc_gait_schedule.h): every robot walks its own sequence of commands,
switched at its own times and joined by smooth turns -- up to a kerb and along it, a square, to a stop, into reverse.
`GaitPlanner.set_feedback` closes the loop on the footholds (include/wbc_gait_feedback.h): a pass after the gait's kernel
shifts every swing's landing point by what the measured trunk velocity asks for, so that a pushed robot steps after its trunk.
Torch tensors and torch's current stream, as in controller.py and plant.py.
"""
import ctypes as C
import operator

import numpy as np

from . import _lib, terrain, workloads

FEET = ("LF", "RF", "LH", "RH")   # bit i of a contact mask (towr/include/towr/models/endeffector_mappings.h: enum QuadrupedIDs)
# towr/src/quadruped_gait_generator.cc:50-70 names a contact state by two letters, hind legs then front legs: I none, P the left
# one, b the right one, B both.
_II, _PI, _bI, _IP, _Ib = 0b0000, 0b0100, 0b1000, 0b0001, 0b0010
_Pb, _bP, _BI, _IB, _PP, _bb = 0b0110, 0b1001, 0b1100, 0b0011, 0b0101, 0b1010
_Bb, _BP, _bB, _PB, _BB = 0b1110, 0b1101, 0b1011, 0b0111, 0b1111

# name -> (durations [s], contact masks), one entry per phase: the strides of towr/src/quadruped_gait_generator.cc
STRIDES = {
    "stand": ((0.3,), (_BB,)),                                                                      # :113-126 GetStrideStand
    "walk": ((0.3, 0.2, 0.3, 0.2, 0.3, 0.2, 0.3, 0.2), (_bB, _BB, _Bb, _BB, _PB, _BB, _BP, _BB)),   # :162-179 GetStrideWalk
    "walk_overlap": ((0.25, 0.13, 0.25, 0.13, 0.25, 0.13, 0.25, 0.13),
                     (_bB, _bb, _Bb, _Pb, _PB, _PP, _BP, _bP)),                                     # :181-204 GetStrideWalkOverlap
    "trot": ((0.3, 0.2, 0.3, 0.2), (_bP, _BB, _Pb, _BB)),                                           # :206-221 GetStrideTrot
    "trot_fly": ((0.4, 0.1, 0.4, 0.1), (_bP, _II, _Pb, _II)),                                       # :223-240 GetStrideTrotFly
    "pace": ((0.3, 0.1, 0.3, 0.1), (_PP, _II, _bb, _II)),                                           # :257-273 GetStridePace
    "bound": ((0.3, 0.1, 0.3, 0.1), (_BI, _II, _IB, _II)),                                          # :290-306 GetStrideBound
    "pronk": ((0.3, 0.4, 0.3), (_BB, _II, _BB)),                                                    # :143-160 GetStridePronk
    "gallop": ((0.2, 0.3, 0.2, 0.2, 0.2, 0.3, 0.2, 0.2), (_Bb, _BI, _BP, _bP, _bB, _IB, _PB, _Pb)),  # :323-345 GetStrideGallop
    "limp": ((0.1, 0.2, 0.1, 0.1, 0.2, 0.1), (_Bb, _BB, _IP, _Bb, _BB, _IP)),                       # :347-366 GetStrideLimp
}
MAX_STRIDES, MAX_PHASES = 16, 8   # WBC_GAIT_MAX_STRIDES, WBC_GAIT_MAX_PHASES
MAX_SWITCHES = 7                  # WBC_GAIT_MAX_SWITCHES


def path_parameter(ramp_time, t):
    """theta(t) of include/wbc_gait.h: the body's path parameter at t >= 0 [s after wait_time], numpy"""
    t = np.asarray(t, dtype=np.float64)
    if ramp_time > 0:
        x = np.minimum(t / ramp_time, 1.0)
        return np.where(t < ramp_time, ramp_time * (2.5 * x**4 - 3.0 * x**5 + x**6), t - 0.5 * ramp_time)
    return t.copy()


def schedule_arrays(times, cmds, n, ramp_time):
    """(nswitch [n] uint8, when [7, n], cmds [21, n]) as wbc_gait_set_schedule takes them, numpy.  times: [M] or [M, n] seconds after
    wait_time, M <= 7, +inf from a robot's last switch on; cmds: [M, 3] or [M, 3, n] = (vx, vy, yaw rate) from each switch on."""
    times, cmds = np.asarray(times, dtype=np.float64), np.asarray(cmds, dtype=np.float64)
    if times.ndim == 1:
        times = np.repeat(times[:, None], n, axis=1)
    if cmds.ndim == 2:
        cmds = np.repeat(cmds[:, :, None], n, axis=2)
    m = times.shape[0]
    if times.ndim != 2 or m > MAX_SWITCHES or times.shape[1] != n or cmds.shape != (m, 3, n):
        raise ValueError("set_schedule: times [M] or [M, N] and cmds [M, 3] or [M, 3, N] with M <= %d and N = %d" % (MAX_SWITCHES, n))
    used = times < np.inf
    if np.isnan(times).any() or (used[1:] & ~used[:-1]).any():
        raise ValueError("set_schedule: times are numbers, +inf from a robot's last switch on")
    if (times[used] < ramp_time).any():
        raise ValueError("set_schedule: a switch must lie at or after ramp_time (%g s)" % ramp_time)
    when = np.full((MAX_SWITCHES, n), np.inf)
    when[:m] = np.where(used, path_parameter(ramp_time, np.where(used, times, ramp_time)), np.inf)
    c = np.zeros((3 * MAX_SWITCHES, n))
    c[:3 * m] = np.where(used[:, None, :], cmds, 0.0).reshape(3 * m, n)
    return used.sum(0).astype(np.uint8), when, c


def stride(spec):
    """(durations, masks) of a stride given by its name in STRIDES or as such a pair."""
    if isinstance(spec, str):
        if spec not in STRIDES:
            raise ValueError("gait %r: expected one of %s" % (spec, ", ".join(STRIDES)))
        spec = STRIDES[spec]
    d, m = spec
    d, m = [float(x) for x in d], [int(x) for x in m]
    if len(d) != len(m) or not 1 <= len(d) <= MAX_PHASES:
        raise ValueError("a stride is 1 .. %d phases, a duration and a contact mask each" % MAX_PHASES)
    return d, m


def c_strides(specs):
    """The wbc_gait_stride array of a list of strides (names or (durations, masks) pairs)."""
    specs = list(specs)
    arr = (_lib.WbcGaitStride * max(len(specs), 1))()
    for s, spec in zip(arr, specs):
        d, m = stride(spec)
        s.nphase = len(d)
        for j in range(len(d)):
            s.duration[j] = d[j]
            s.contact[j] = m[j] & 0xFF
    return arr


def c_params(stance, height, swing_height, ramp_time, wait_time):
    """The wbc_gait_params of stance [4, 2] (or [4, 3]: workloads.STAND_FEET) and the four scalars."""
    p = _lib.WbcGaitParams()
    st = np.asarray(stance, dtype=np.float64)
    for f in range(4):
        p.stance[f][0], p.stance[f][1] = float(st[f, 0]), float(st[f, 1])
    p.height, p.swing_height, p.ramp_time, p.wait_time = float(height), float(swing_height), float(ramp_time), float(wait_time)
    return p


BODY_MODES = ("lift", "fit")   # WBC_GAIT_BODY_LIFT, WBC_GAIT_BODY_FIT


def c_terrain_params(body="fit", max_grade=0.5, edge_margin=0.03, apex_max=0.25):
    """The wbc_gait_terrain_params of a body mode (a name of BODY_MODES or its number) and the three scalars."""
    p = _lib.WbcGaitTerrainParams()
    p.body_mode = BODY_MODES.index(body) if body in BODY_MODES else int(body)
    p.max_grade, p.edge_margin, p.apex_max = float(max_grade), float(edge_margin), float(apex_max)
    return p


def _dev_ptr(a, rows, n, dtype, name, device, optional=False):
    return _lib.dev_ptr(a, rows, n, dtype, name, device, "the planner", optional)


class GaitPlanner(_lib.Handle):
    """The targets of N walking robots, each with its own command (include/wbc_gait.h).

    model: a name of workloads.STAND_FEET, which gives the nominal stance and height (or pass stance [4, 2] and height);
    strides: up to 16 strides, names of STRIDES or (durations, masks) pairs; instance i walks strides[gait_id[i]].
    swing_height [m]; ramp_time [s]: the body reaches its commanded velocity smoothly over this time, stepping in place at first;
    wait_time [s]: standing targets before it, as the trajectories have it."""

    _destroy = "wbc_gait_destroy"

    def __init__(self, model="mini_cheetah", strides=("trot",), swing_height=0.05, ramp_time=0.5, wait_time=0.0, device=0, stance=None,
                 height=None):
        if stance is None or height is None:
            if model not in workloads.STAND_FEET:
                raise ValueError("GaitPlanner: no nominal stance for model %r; pass stance and height" % (model,))
            stance = workloads.STAND_FEET[model] if stance is None else stance
            height = workloads.NOMINAL_HEIGHT[model] if height is None else height
        strides = [strides] if isinstance(strides, str) else list(strides)
        self.strides = [stride(s) for s in strides]
        self.params = c_params(stance, height, swing_height, ramp_time, wait_time)
        self.device = int(device)
        self._L = _lib.lib()
        h = C.c_void_p()
        _lib.check(self._L.wbc_gait_create(C.byref(self.params), c_strides(self.strides), len(self.strides), self.device, C.byref(h)))
        self._h = h

    def set_commands(self, cmd, gait_id=None, stride_scale=None, start=None):
        """cmd [3, N] float64 = (vx, vy, yaw rate), velocity in the heading frame; gait_id [N] uint8 (None: stride 0); stride_scale [N]
        float64 (None: 1.0; the stride's durations times it); start [3, N] float64 = (x0, y0, yaw0) (None: 0).  The tensors live on
        the planner's device and are kept alive here; rewriting them changes what the next targets() gives."""
        import torch
        if not (isinstance(cmd, torch.Tensor) and cmd.dim() == 2):
            raise ValueError("cmd: expected a CUDA tensor of shape [3, N]")
        n, d = int(cmd.shape[1]), self.device
        pc = _dev_ptr(cmd, 3, n, "float64", "cmd", d)
        pg = _dev_ptr(gait_id, 0, n, "uint8", "gait_id", d, True)
        ps = _dev_ptr(stride_scale, 0, n, "float64", "stride_scale", d, True)
        p0 = _dev_ptr(start, 3, n, "float64", "start", d, True)
        _lib.check(self._L.wbc_gait_set_commands(self._h, pc, pg, ps, p0))
        self._n, self._keep = n, (cmd, gait_id, stride_scale, start)

    def set_schedule(self, times, cmds, blend=0.5):
        """Steer the planner (include/wbc_gait_schedule.h): from times[j] [s after wait_time] on a robot walks cmds[j]
        instead of the command before it, the first being set_commands' cmd.  times: [M] or [M, N], M <= 7, each at or after
        ramp_time, +inf from a robot's last switch on; cmds: [M, 3] or [M, 3, N]; numpy or lists, one column per robot or one for
        all.  blend [s of steady walking]: the length of the smooth turn after a switch, which must end before the next switch
        (a robot whose switches are closer gets NaN targets).  Needs set_commands, and is called again after cmd or start are
        rewritten.  Synchronises torch's current stream."""
        import torch
        if self._n is None:
            raise ValueError("GaitPlanner.set_schedule: set_commands first")
        n, d = self._n, self.device
        m, when, c = schedule_arrays(times, cmds, n, self.params.ramp_time)
        tm, tw, tc = (torch.tensor(a, device="cuda:%d" % d) for a in (m, when, c))      # alive until the call has synchronised
        _lib.check(self._L.wbc_gait_set_schedule(self._h, self._stream(), n, n, float(blend), _dev_ptr(tm, 0, n, "uint8", "nswitch", d),
                                                 _dev_ptr(tw, MAX_SWITCHES, n, "float64", "when", d),
                                                 _dev_ptr(tc, 3 * MAX_SWITCHES, n, "float64", "cmds", d)))
        self._schedule = (m, when, c, float(blend))

    def clear_schedule(self):
        """One command per robot again: the kernels a planner without a schedule launches."""
        _lib.check(self._L.wbc_gait_clear_schedule(self._h))
        self._schedule = None

    @property
    def has_schedule(self):
        return self._schedule is not None

    def schedule_kernel_info(self, terrain=False):
        """kernel_info() of the kernel that runs while a schedule is set, without or with a terrain."""
        return _lib.kernel_info(lambda h, *out: self._L.wbc_gait_schedule_kernel_info(h, int(bool(terrain)), *out), self._h)

    def feedback_defaults(self):
        """dict(k_v, k_p, d_max, u_hold) of wbc_gait_feedback_params_default for this planner's body height."""
        p = _lib.WbcGaitFeedbackParams()
        _lib.check(self._L.wbc_gait_feedback_params_default(C.byref(self.params), C.byref(p)))
        return dict(k_v=p.k_v, k_p=p.k_p, d_max=p.d_max, u_hold=p.u_hold)

    def set_feedback(self, n, **params):
        """Let the footholds react to the measured trunk (include/wbc_gait_feedback.h): allocates and zeroes the state
        of n robots; called again, it resets it.  params: k_v [s], k_p, d_max [m], u_hold over feedback_defaults().  From then on
        targets_measured() works, and a rollout that takes this planner (plant.closed_loop) feeds it its own q and v; targets() is
        unchanged.  Not with a terrain.  Synchronises the device."""
        d = self.feedback_defaults()
        unknown = set(params) - set(d)
        if unknown:
            raise ValueError("set_feedback: unknown parameter %s; expected k_v, k_p, d_max, u_hold" % ", ".join(sorted(unknown)))
        d.update({k: float(x) for k, x in params.items()})
        p = _lib.WbcGaitFeedbackParams(**d)
        _lib.check(self._L.wbc_gait_set_feedback(self._h, C.byref(p), int(n)))
        self._feedback = (int(n), d)

    def clear_feedback(self):
        """The planner is a function of the time again; rollouts issue the launches they issue without feedback."""
        _lib.check(self._L.wbc_gait_clear_feedback(self._h))
        self._feedback = None

    @property
    def has_feedback(self):
        return self._feedback is not None

    def feedback_kernel_info(self):
        """kernel_info() of the feedback pass's kernel."""
        return self._kernel_info("wbc_gait_feedback_kernel_info")

    def targets_measured(self, time, q, v, out=None, offsets=None):
        """targets(time, out), then the feedback pass on the measured q [19, N] and v [18, N]: the foot rows shifted, the state
        advanced by one call.  offsets: an optional [8, N] float64 tensor that receives the (x, y) offset of each foot.  Needs
        set_feedback.  Asynchronous on torch's current stream."""
        if self._n is None:
            raise ValueError("GaitPlanner.targets_measured: set_commands first")
        n, d = self._n, self.device
        pt = _dev_ptr(time, 0, n, "float64", "time", d)
        pq = _dev_ptr(q, 19, n, "float64", "q", d)
        pv = _dev_ptr(v, 18, n, "float64", "v", d)
        outs, pouts = _lib.outputs(out, _lib.TARGET_OUTS, n, d, "the planner")
        pof = _dev_ptr(offsets, 8, n, "float64", "offsets", d, True)
        _lib.check(self._L.wbc_gait_targets_measured(self._h, self._stream(), n, n, pt, pq, pv, *pouts, pof))
        return outs

    def targets(self, time, out=None):
        """-> (targets [54, N] float64, contact_mask [N] uint8) at time [N] float64; out: such a pair to write into.  Asynchronous on
        torch's current stream."""
        if self._n is None:
            raise ValueError("GaitPlanner.targets: set_commands first")
        n, d = self._n, self.device
        self._check_terrain_n(n)
        pt = _dev_ptr(time, 0, n, "float64", "time", d)
        outs, pouts = _lib.outputs(out, _lib.TARGET_OUTS, n, d, "the planner")
        _lib.check(self._L.wbc_gait_targets(self._h, self._stream(), n, n, pt, *pouts))
        return outs

    def set_terrain(self, profiles, terrain_id=None, terrain_scale=None, body="fit", max_grade=0.5, edge_margin=0.03, apex_max=0.25):
        """Make the planner's targets the finished targets on a terrain (include/wbc_gait_terrain.h): footholds on the
        surface and moved `edge_margin` [m] clear of every piece steeper than `max_grade`, swings that clear the knots between their
        footholds (apex at most `apex_max` [m]), a body that follows the feet -- body "lift": its height, "fit": also its pitch and
        roll.  profiles: 1 .. 16 terrain.Profile, what GroundContactPlant.set_terrain takes; instance i walks on
        profiles[terrain_id[i]] (uint8 [N]; None: profile 0) scaled by terrain_scale[i] (float64 [N]; None: 1.0); the tensors are kept
        alive here.  No follow pass may run after such targets.  Synchronises the device."""
        if body not in BODY_MODES:
            raise ValueError("body %r: expected one of %s" % (body, ", ".join(BODY_MODES)))
        *args, stored = terrain.bind(profiles, terrain_id, terrain_scale, self.device, "the planner", " (clear_terrain() takes the terrain away)")
        tp = c_terrain_params(body, max_grade, edge_margin, apex_max)
        _lib.check(self._L.wbc_gait_set_terrain(self._h, C.byref(tp), *args))
        self._terrain = stored + (body,)

    def clear_terrain(self):
        """The plain gait again: targets about the plane z = 0, the kernel a planner without a terrain launches."""
        _lib.check(self._L.wbc_gait_set_terrain(self._h, None, None, 0, None, None))
        self._terrain = None

    def _check_terrain_n(self, n):
        terrain._check_terrain_n(self._terrain, n, operator.ne, "the GaitPlanner's ")   # the planner's terrain is set for one batch size

    @property
    def has_terrain(self):
        return self._terrain is not None

    def kernel_info(self):
        """Registers, scratch bytes per lane, LDS bytes and threads per block of the gait kernel."""
        return self._kernel_info("wbc_gait_kernel_info")

    def terrain_kernel_info(self):
        """kernel_info() of the kernel that runs while a terrain is set."""
        return self._kernel_info("wbc_gait_terrain_kernel_info")

    def close(self):
        super().close()
        self._keep = self._terrain = self._schedule = self._feedback = None
