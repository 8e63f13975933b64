"""Batched rigid-contact plant step (include/wbc_plant.h): the robot that a closed loop's torques act on.

`wbc_integrate` / `BatchedController.rollout` replay the controller's own plan (the QP's accelerations).  `RigidContactPlant`
instead applies the controller's torques to a robot of its own -- the same kinematic tree with its own trunk mass scale, friction
and actuator limit -- holds the stance feet with rigid contacts and reports, per instance and step, where a real ground would have
let go (PULL, CONE), where a torque was clipped (CLIP) and what it could not answer (BAD).  `closed_loop` chains
lookup -> controller tick -> plant step on the device.  Torch tensors and torch's current stream, as in controller.py.

`GroundContactPlant` (include/wbc_ground.h) has a ground instead of held feet: a compliant half-space z = 0 whose force on each
foot is an explicit function of the state, so feet lift off, land and slip and a robot that tips falls.  One `step` runs all
explicit substeps of a control period in a single launch.  `set_terrain` replaces the plane by per-instance slopes, ramps and
steps (terrain.py), and `follow_targets` / `set_follow` make the planners' level-ground targets follow it.  `closed_loop` takes
either plant.
"""
import contextlib
import ctypes as C
import math
import operator

from . import _lib, terrain
from ._lib import WbcGroundParams, WbcPlantParams  # noqa: F401 (the mirrors of wbc_plant_params / wbc_ground_params, under their names here)
from .controller import BatchedController, load_model

PULL, CONE, CLIP, BAD = 1, 2, 4, 8
SLIP, FELL = 1, 2   # GroundContactPlant's bits 0 and 1 (CLIP and BAD as above)
FOLLOW_MODES = {"off": 0, "lift": 1, "fit": 2}   # WBC_FOLLOW_OFF / _LIFT / _FIT of include/wbc_ground.h


def _follow_mode(mode):
    """The WBC_FOLLOW_* number of a mode given by name or by number."""
    if isinstance(mode, str):
        if mode not in FOLLOW_MODES:
            raise ValueError("follow mode %r: expected one of %s" % (mode, ", ".join(FOLLOW_MODES)))
        return FOLLOW_MODES[mode]
    return int(mode)


_L = _lib.lib   # libwbc_hip.so, bound (the prototypes of every header: _lib.PROTOTYPES)


def _dev_ptr(a, rows, n, dtype, name, device, optional=False):
    return _lib.dev_ptr(a, rows, n, dtype, name, device, "the plant", optional)


def _outputs(out, specs, n, device):
    return _lib.outputs(out, specs, n, device, "the plant")


_wbc_model = _lib.fill_model

# the plants' output sets, as _lib.outputs takes them, in the order of the entry points' arguments
_RIGID_OUTS = ((18, "float64", "vdot"), (12, "float64", "force"), (0, "int32", "flags"))
_RIGID_LOOP_OUTS = _RIGID_OUTS[1:]
_GROUND_OUTS = ((18, "float64", "vdot"), (12, "float64", "force"), (0, "uint8", "contact"), (0, "int32", "flags"))
_GROUND_STEP_OUTS = _GROUND_OUTS[1:]


class _Plant(_lib.Handle):
    """What the two plants share beyond _lib.Handle: the model table and its wbc_model.  A subclass sets self._h in its __init__."""

    def _open(self, model, device, q_perm, act_perm):
        """-> (the bound library, the wbc_model of `model`)"""
        self.table = load_model(model) if isinstance(model, str) else model
        self.device = int(device)
        self._L = _L()
        return self._L, _wbc_model(self.table, q_perm, act_perm)


class RigidContactPlant(_Plant):
    """Forward dynamics of N robots under applied torques, stance feet held by rigid contacts, semi-implicit Euler step.

    model: name or path (as the controllers take it), or a model table; q_perm / act_perm as in the controllers.
    kd_contact: the stance rows' velocity gain (the controllers' Kd_contact); tau_max: actuator limit (torques are clipped,
    CLIP reported); mu: the plant's friction where no per-instance value is given (1.0: the reference's ground)."""

    _destroy = "wbc_plant_destroy"

    def __init__(self, model="mini_cheetah", device=0, kd_contact=100.0, tau_max=math.inf, mu=1.0, q_perm=None, act_perm=None):
        L, m = self._open(model, device, q_perm, act_perm)
        p = WbcPlantParams(float(kd_contact), float(tau_max), float(mu))
        self.params = p
        h = C.c_void_p()
        _lib.check(L.wbc_plant_create(C.byref(m), C.byref(p), self.device, C.byref(h)))
        self._h = h

    def _inputs(self, q, v, tau, contact_mask, mu, mass_scale):
        n = int(q.shape[1])
        d = self.device
        return n, [_dev_ptr(q, 19, n, "float64", "q", d), _dev_ptr(v, 18, n, "float64", "v", d),
                   _dev_ptr(tau, 12, n, "float64", "tau", d), _dev_ptr(contact_mask, 0, n, "uint8", "contact_mask", d),
                   _dev_ptr(mu, 0, n, "float64", "mu", d, True), _dev_ptr(mass_scale, 0, n, "float64", "mass_scale", d, True)]

    def forward(self, q, v, tau, contact_mask, mu=None, mass_scale=None, out=None):
        """-> (vdot[18, N], force[12, N], flags[N]); q and v are not changed.  Asynchronous on torch's current stream."""
        n, ins = self._inputs(q, v, tau, contact_mask, mu, mass_scale)
        outs, pouts = _outputs(out, _RIGID_OUTS, n, self.device)
        _lib.check(self._L.wbc_plant_forward(self._h, self._stream(), n, n, *ins, *pouts))
        return outs

    def step(self, q, v, tau, contact_mask, dt, time=None, mu=None, mass_scale=None, counts=None, out=None):
        """forward, then the semi-implicit Euler step in place on q, v (time += dt when given; counts[4, N] int32: row b += 1
        when flag bit b is raised).  -> (vdot, force, flags)"""
        n, ins = self._inputs(q, v, tau, contact_mask, mu, mass_scale)
        pt = _dev_ptr(time, 0, n, "float64", "time", self.device, True)
        pc = _dev_ptr(counts, 4, n, "int32", "counts", self.device, True)
        outs, pouts = _outputs(out, _RIGID_OUTS, n, self.device)
        _lib.check(self._L.wbc_plant_step(self._h, self._stream(), n, n, float(dt), ins[0], ins[1], pt, *ins[2:], *pouts, pc))
        return outs

    def kernel_info(self):
        """Registers, scratch bytes per lane, LDS bytes and threads per block of the plant-step kernel."""
        return self._kernel_info("wbc_plant_kernel_info")


class GroundContactPlant(_Plant):
    """Forward dynamics of N robots under applied torques on a compliant half-space z = 0 (include/wbc_ground.h): Hunt-Crossley
    normal force, Coulomb friction regularised below v_stiction, explicit substeps of at most max_substep inside one launch.

    model, q_perm, act_perm as RigidContactPlant.  Every parameter left None takes the model's default (wbc_ground_params_default:
    stiffness = weight / 1 mm, dissipation = 1 / sqrt(g 1 mm), mu 1.0, v_stiction 0.05 m/s, foot_radius 0, tau_max inf,
    max_substep 0.0625 ms, fall_height 0).  Below v_stiction a loaded foot creeps at up to v_stiction."""

    _destroy = "wbc_ground_destroy"

    def __init__(self, model="mini_cheetah", device=0, stiffness=None, dissipation=None, mu=None, v_stiction=None, foot_radius=None,
                 tau_max=None, max_substep=None, fall_height=None, q_perm=None, act_perm=None):
        L, m = self._open(model, device, q_perm, act_perm)
        p = WbcGroundParams()
        _lib.check(L.wbc_ground_params_default(C.byref(m), C.byref(p)))
        for k, x in (("stiffness", stiffness), ("dissipation", dissipation), ("mu", mu), ("v_stiction", v_stiction),
                     ("foot_radius", foot_radius), ("tau_max", tau_max), ("max_substep", max_substep), ("fall_height", fall_height)):
            if x is not None:
                setattr(p, k, float(x))
        self.params = p
        h = C.c_void_p()
        _lib.check(L.wbc_ground_create(C.byref(m), C.byref(p), self.device, C.byref(h)))
        self._h = h

    def close(self):
        super().close()
        self._terrain = None

    def set_terrain(self, profiles, terrain_id=None, terrain_scale=None):
        """Put the ground of terrain.py under the feet: `profiles`, a list of 1 .. 16 terrain.Profile, or None for the plane z = 0
        again.  Instance i stands on profiles[terrain_id[i]] (uint8 [N] on the plant's device; None: profile 0) scaled in height
        by terrain_scale[i] (float64 [N]; None: 1.0).  Both tensors must cover the N of every later forward / step / closed_loop
        and are kept alive here.  An id beyond the list or a non-finite scale makes the instance BAD.  Synchronises the device."""
        if profiles is None:
            if terrain_id is not None or terrain_scale is not None:
                raise ValueError("set_terrain: terrain_id / terrain_scale need profiles")
            _lib.check(self._L.wbc_ground_set_terrain(self._h, None, 0, None, None))
            self._terrain = None
            return
        *args, stored = terrain.bind(profiles, terrain_id, terrain_scale, self.device, "the plant")
        _lib.check(self._L.wbc_ground_set_terrain(self._h, *args))
        self._terrain = stored

    def follow_targets(self, targets, mode="fit"):
        """Make targets [54, N] follow the terrain set on this plant, in place (include/wbc_ground.h, "Following the ground"):
        "lift" raises every foot target onto the surface under it and the body target onto the line fitted through the four planned
        footholds; "fit" also turns the body's attitude with that line; "off" does nothing.  Without a terrain nothing is launched.
        Asynchronous on torch's current stream.  -> targets"""
        n = int(targets.shape[1])
        self._check_terrain_n(n)
        pt = _dev_ptr(targets, 54, n, "float64", "targets", self.device)
        _lib.check(self._L.wbc_ground_follow_targets(self._h, self._stream(), n, n, _follow_mode(mode), pt))
        return targets

    def set_follow(self, mode):
        """What closed_loop does between the target lookup and the tick on this plant: "off" (the default), "lift" or "fit", as
        follow_targets.  With "off", or without a terrain, closed_loop launches what it launches without this call."""
        _lib.check(self._L.wbc_ground_set_follow(self._h, _follow_mode(mode)))
        self._follow = ("off", "lift", "fit")[_follow_mode(mode)]

    def follow_kernel_info(self):
        """kernel_info() of the kernel behind follow_targets."""
        return self._kernel_info("wbc_ground_follow_kernel_info")

    def _check_terrain_n(self, n):
        terrain._check_terrain_n(self._terrain, n, operator.lt)     # a call may take the first n of a longer terrain

    def substeps(self, dt):
        """The number of explicit substeps wbc_ground_step takes for a period dt."""
        return max(1, int(math.ceil(float(dt) / self.params.max_substep * (1.0 - 1e-12))))

    def _inputs(self, q, v, tau, mu, mass_scale, ext_wrench):
        n = int(q.shape[1])
        d = self.device
        self._check_terrain_n(n)
        return n, [_dev_ptr(q, 19, n, "float64", "q", d), _dev_ptr(v, 18, n, "float64", "v", d),
                   _dev_ptr(tau, 12, n, "float64", "tau", d), _dev_ptr(mu, 0, n, "float64", "mu", d, True),
                   _dev_ptr(mass_scale, 0, n, "float64", "mass_scale", d, True),
                   _dev_ptr(ext_wrench, 6, n, "float64", "ext_wrench", d, True)]

    def forward(self, q, v, tau, mu=None, mass_scale=None, ext_wrench=None):
        """One force evaluation -> (vdot[18, N], force[12, N], contact[N] uint8 foot bits, flags[N]); q and v are not changed.
        Asynchronous on torch's current stream."""
        n, ins = self._inputs(q, v, tau, mu, mass_scale, ext_wrench)
        outs, pouts = _outputs(None, _GROUND_OUTS, n, self.device)
        _lib.check(self._L.wbc_ground_forward(self._h, self._stream(), n, n, *ins, *pouts))
        return outs

    def step(self, q, v, tau, dt, time=None, mu=None, mass_scale=None, ext_wrench=None, counts=None, out=None):
        """One control period dt in substeps(dt) explicit substeps, in place on q, v (time += dt when given; counts[4, N] int32:
        row b += 1 when flag bit b is raised).  -> (force[12, N] mean over the substeps, contact[N] of the last substep, flags[N]);
        out: such a triple to write into."""
        n, ins = self._inputs(q, v, tau, mu, mass_scale, ext_wrench)
        pt = _dev_ptr(time, 0, n, "float64", "time", self.device, True)
        pc = _dev_ptr(counts, 4, n, "int32", "counts", self.device, True)
        outs, pouts = _outputs(out, _GROUND_STEP_OUTS, n, self.device)
        _lib.check(self._L.wbc_ground_step(self._h, self._stream(), n, n, float(dt), ins[0], ins[1], pt, *ins[2:], *pouts, pc))
        return outs

    def kernel_info(self):
        """Registers, scratch bytes per lane, LDS bytes and threads per block of the ground-step kernel."""
        return self._kernel_info("wbc_ground_kernel_info")

    def terrain_kernel_info(self):
        """kernel_info() of the step kernel that runs while a terrain is set."""
        return self._kernel_info("wbc_ground_terrain_kernel_info")


@contextlib.contextmanager
def _gait_set(plant, setter, gait):
    """The gait as the target source of the plant's rollout for the length of the block; gait None: nothing, and no entry point of
    include/wbc_gait.h is looked up (a library from before the gait planner runs every trajectory loop)."""
    if gait is None:
        yield
        return
    set_gait = getattr(plant._L, setter)
    _lib.check(set_gait(plant._h, gait._h))
    try:
        yield
    finally:
        set_gait(plant._h, None)     # the rollout has issued its launches: the handle goes back to trajectories


def closed_loop(ctrl, plant, traj, steps, dt, q, v, time, mu=None, mass_scale=None, plant_mu=None, plant_mass_scale=None, counts=None,
                ext_wrench=None):
    """`steps` x (target lookup at time -> ctrl tick -> plant step) on the device, on torch's current stream: wbc_plant_rollout for
    a RigidContactPlant, wbc_ground_rollout for a GroundContactPlant.  Updates q, v, time in place; counts (int32 [4, N], optional)
    accumulates the plant's flag bits.  mu / mass_scale go to the controller, plant_mu / plant_mass_scale to the plant.
    ext_wrench ([6, N], GroundContactPlant only): a world-frame wrench on the trunk held over the whole loop.
    traj: a trajectory (planners.py), or a gait.GaitPlanner whose set_commands covers these N instances: every tick's targets and
    mask are then the gait's at `time` (gait -> follow, if set -> tick -> plant step).  A GaitPlanner with a terrain
    (GaitPlanner.set_terrain) gives finished targets: with a follow mode set on a plant with a terrain this raises ValueError.
    Returns the last tick's (tau, metrics, status, targets, mask, force, flags), and for a GroundContactPlant also contact."""
    from .gait import GaitPlanner
    if ctrl.host_ptrs:
        raise ValueError("closed_loop: needs a device-pointer controller")
    ground = isinstance(plant, GroundContactPlant)
    if not ground and not isinstance(plant, RigidContactPlant):
        raise TypeError("closed_loop: plant must be a RigidContactPlant or a GroundContactPlant")
    if ext_wrench is not None and not ground:
        raise ValueError("closed_loop: ext_wrench needs a GroundContactPlant")
    n = int(q.shape[1])
    d = plant.device
    if ground:
        plant._check_terrain_n(n)
    gait = traj if isinstance(traj, GaitPlanner) else None
    if gait is not None:
        if gait._n != n:
            raise ValueError("closed_loop: the GaitPlanner's commands hold %s instances, the call has %d" % (gait._n, n))
        if gait.device != d:
            raise ValueError("closed_loop: the GaitPlanner lives on cuda:%d, the plant on cuda:%d" % (gait.device, d))
        if gait.has_terrain:
            gait._check_terrain_n(n)
            if plant._follow != "off" and plant._terrain is not None:
                raise ValueError("closed_loop: the GaitPlanner has a terrain, so its targets are finished; the plant's follow mode %r "
                                 "would lift them a second time (set_follow('off'))" % (plant._follow,))
    htraj = None if gait is not None else traj._h
    ptr = lambda a, rows, dtype, name, opt=False: _dev_ptr(a, rows, n, dtype, name, d, opt)
    pq, pv, pt = ptr(q, 19, "float64", "q"), ptr(v, 18, "float64", "v"), ptr(time, 0, "float64", "time")
    pmu, pms = ptr(mu, 0, "float64", "mu", True), ptr(mass_scale, 0, "float64", "mass_scale", True)
    ppmu, ppms = ptr(plant_mu, 0, "float64", "plant_mu", True), ptr(plant_mass_scale, 0, "float64", "plant_mass_scale", True)
    pc = ptr(counts, 4, "int32", "counts", True)

    def fresh(specs, zero=False):
        """Fresh outputs beside q -> (tensors, their pointers, taken as the caller's tensors' are)"""
        ts = [_lib.new_out(rows, n, dtype, q.device, zero) for rows, dtype, _ in specs]
        return ts, [ptr(t, rows, dtype, name) for t, (rows, dtype, name) in zip(ts, specs)]

    (tg, mk), (ptg, pmk) = fresh(_lib.TARGET_OUTS)
    (tau, met, st), ptick = fresh(_lib.TICK_OUTS)
    # what only the ground has sits in lists of one or none: the wrench among the arguments, the contact between force and flags.
    # The plant's outputs are zeroed: with steps == 0 the caller sees them unwritten.
    if ground:
        (f, ct, fl), pplant = fresh(_GROUND_STEP_OUTS, zero=True)
        rollout, set_gait, contact = "wbc_ground_rollout", "wbc_ground_set_gait", [ct]
        wrench, pwrench = [ext_wrench], [ptr(ext_wrench, 6, "float64", "ext_wrench", True)]
    else:
        (f, fl), pplant = fresh(_RIGID_LOOP_OUTS, zero=True)
        rollout, set_gait, contact = "wbc_plant_rollout", "wbc_plant_set_gait", []
        wrench, pwrench = [], []
    s = _lib.stream_of(d)
    with _gait_set(plant, set_gait, gait):
        _lib.check(getattr(plant._L, rollout)(ctrl._h, plant._h, htraj, C.c_void_p(s), int(steps), float(dt), n, n, pq, pv, pt, ptg, pmk,
                                              pmu, pms, ppmu, ppms, *pwrench, *ptick, *pplant, pc))
    # The rollout bound the controller to this stream (wbc_set_stream).  Through the class: whatever stands in for a controller here
    # need hold no more than host_ptrs and _h.
    BatchedController._adopt(ctrl, s, (tg, mk, tau, met, st, f, fl, *contact, mu, mass_scale, plant_mu, plant_mass_scale, *wrench))
    return (tau, met, st, tg, mk, f, fl, *contact)
