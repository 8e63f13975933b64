"""Every misuse path of the C ABI that answers before the device is touched, and the exact text wbc_last_error() then holds.

The strings are literals, recorded from the library as it was before its host side was folded into csrc/wbc_host.hpp; the one
sentence that changed on purpose is the x-y-y sentence of the plants, which now reads as wbc_create's always did.

A handle is an opaque pointer, and the argument checks of an entry point read at most the handle's plain fields before they
answer.  Where a check sits behind the null-handle test, the calls below pass a zeroed block as the handle (max_batch 0, flags 0,
all parameters 0): enough to reach the check, and nothing that is reached with it touches the device.
"""
import ctypes as C

import pytest

from quadruped_drake_amd import _lib, plant
from quadruped_drake_amd.controller import load_model

XYY = ("unsupported kinematic tree -- the kernels are specialised to legs with the abduction joint about +-x and the hip and knee "
       "joints about +-y (Mini Cheetah, ANYmal)")
MAX_LD = 1 << 23
N9, N10, N11, N15, N17 = ([None] * k for k in (9, 10, 11, 15, 17))


@pytest.fixture(scope="module")
def L():
    return plant._L()


def _model(axis=None, q_perm=None, act_perm=None):
    """Mini Cheetah's table; `axis`: the joint axis of the first link (flat[13:16]) replaced"""
    m = _lib.fill_model(load_model("mini_cheetah"), q_perm, act_perm if act_perm is not None else list(range(12)))
    if axis is not None:
        m.flat[13:16] = axis
    return m


def _blank():
    return C.create_string_buffer(4096)


def _says(L, rc, text):
    """rc: the answer of a call just made, or the call to make"""
    rc = rc() if callable(rc) else rc
    assert rc == -1, (rc, L.wbc_last_error())
    assert L.wbc_last_error().decode() == text


def test_null_handles(L):
    z = [None] * 9
    f = C.c_float()
    i4 = [C.byref(C.c_int()) for _ in range(4)]
    for rc, text in (
            (lambda: L.wbc_set_stream(None, None), "wbc_set_stream: null handle"),
            (lambda: L.wbc_step(None, 0, 0, *z), "wbc_step: null handle"),
            (lambda: L.wbc_sync(None), "wbc_sync: null handle"),
            (lambda: L.wbc_time_steps(None, 1, 0, 0, *z, None), "wbc_step: null handle"),
            (lambda: L.wbc_time_steps_result(None, C.byref(f)), "wbc_time_steps_result: null argument"),
            (lambda: L.wbc_time_steps_each(None, 1, 0, 0, *z, None), "wbc_step: null handle"),
            (lambda: L.wbc_stats_get(None, None), "wbc_stats_get: null argument"),
            (lambda: L.wbc_stats_pack(None, None), "wbc_stats_pack: null argument"),
            (lambda: L.wbc_stats_reduce(None, 1, None), "wbc_stats_reduce: null argument or world < 1"),
            (lambda: L.wbc_stats_reset(None), "wbc_stats_reset: null handle"),
            (lambda: L.wbc_set_vdot_output(None, None), "wbc_set_vdot_output: null handle"),
            (lambda: L.wbc_integrate(None, 0, 0, 0.0, None, None, None), "wbc_integrate: null handle"),
            (lambda: L.wbc_rollout(None, None, 0, 0.0, 0, 0, *N11), "wbc_rollout: null handle"),
            (lambda: L.wbc_set_warm_start(None, 1), "wbc_set_warm_start: null handle"),
            (lambda: L.wbc_set_variant(None, 0), "wbc_set_variant: null handle"),
            (lambda: L.wbc_variant_for(None, 1), "wbc_variant_for: bad argument"),
            (lambda: L.wbc_kernel_info(None, *i4), "wbc_kernel_info: null handle"),
            (lambda: L.wbc_rollout_kernel_info(None, *i4), "wbc_rollout_kernel_info: null handle"),
            (lambda: L.wbc_traj_lookup(None, None, 0, 0, None, None, None), "wbc_traj_lookup: bad argument"),
            (lambda: L.wbc_plant_kernel_info(None, *i4), "wbc_plant_kernel_info: null plant handle"),
            (lambda: L.wbc_plant_step(None, None, 0, 0, 1e-3, *N11), "wbc_plant_step: null plant handle"),
            (lambda: L.wbc_plant_forward(None, None, 0, 0, *N9), "wbc_plant_forward: null plant handle"),
            (lambda: L.wbc_plant_rollout(None, None, None, None, 0, 1e-3, 0, 0, *N15), "wbc_plant_rollout: null plant handle"),
            (lambda: L.wbc_ground_kernel_info(None, *i4), "wbc_ground_kernel_info: null ground handle"),
            (lambda: L.wbc_ground_terrain_kernel_info(None, *i4), "wbc_ground_terrain_kernel_info: null ground handle"),
            (lambda: L.wbc_ground_step(None, None, 0, 0, 1e-3, *N11), "wbc_ground_step: null ground handle"),
            (lambda: L.wbc_ground_forward(None, None, 0, 0, *N10), "wbc_ground_forward: null ground handle"),
            (lambda: L.wbc_ground_rollout(None, None, None, None, 0, 1e-3, 0, 0, *N17), "wbc_ground_rollout: null ground handle"),
            (lambda: L.wbc_ground_set_terrain(None, None, 0, None, None), "wbc_ground_set_terrain: null ground handle")):
        _says(L, rc, text)
    assert L.wbc_destroy(None) == 0 and L.wbc_traj_destroy(None) == 0 and L.wbc_plant_destroy(None) == 0 and L.wbc_ground_destroy(None) == 0


def test_null_arguments_of_the_constructors(L):
    h = C.c_void_p()
    m = _model()
    for rc, text in (
            (lambda: L.wbc_params_default(0, None), "wbc_params_default: bad argument"),
            (lambda: L.wbc_params_default(4, C.byref(_lib.WbcParams())), "wbc_params_default: bad argument"),
            (lambda: L.wbc_create(None, 0, None, 8, 0, 0, C.byref(h)), "wbc_create: null argument"),
            (lambda: L.wbc_create(C.byref(m), 0, None, 8, 0, 0, None), "wbc_create: null argument"),
            (lambda: L.wbc_plant_params_default(None), "wbc_plant_params_default: null argument"),
            (lambda: L.wbc_plant_create(None, None, 0, C.byref(h)), "wbc_plant_create: null argument"),
            (lambda: L.wbc_plant_create(C.byref(m), None, 0, None), "wbc_plant_create: null argument"),
            (lambda: L.wbc_ground_params_default(None, None), "wbc_ground_params_default: null argument"),
            (lambda: L.wbc_ground_create(None, None, 0, C.byref(h)), "wbc_ground_create: null argument"),
            (lambda: L.wbc_traj_create(0, 0, None, None, None, None, 0, 0.0, C.byref(h)), "wbc_traj_create: bad argument")):
        _says(L, rc, text)


def test_wbc_create_kind_batch_and_parameters(L):
    h = C.c_void_p()
    m = _model()
    p = _lib.WbcParams()
    assert L.wbc_params_default(1, C.byref(p)) == 0
    p.mu = 0.0
    for rc, text in (
            (lambda: L.wbc_create(C.byref(m), -1, None, 8, 0, 0, C.byref(h)), "wbc_create: kind must be WBC_KIND_ID, _MPTC, _PC or _CLF"),
            (lambda: L.wbc_create(C.byref(m), 4, None, 8, 0, 0, C.byref(h)), "wbc_create: kind must be WBC_KIND_ID, _MPTC, _PC or _CLF"),
            (lambda: L.wbc_create(C.byref(m), 0, None, 0, 0, 0, C.byref(h)), "wbc_create: max_batch must be in 1 .. WBC_MAX_LD (2^23)"),
            (lambda: L.wbc_create(C.byref(m), 0, None, MAX_LD + 1, 0, 0, C.byref(h)), "wbc_create: max_batch must be in 1 .. WBC_MAX_LD (2^23)"),
            (lambda: L.wbc_create(C.byref(m), 1, C.byref(p), 8, 0, 0, C.byref(h)), "wbc_create: mu, eps2, w_body, w_foot and tau_max must be positive")):
        _says(L, rc, text)
    pp = plant.WbcPlantParams(100.0, 1.0, -1.0)
    _says(L, L.wbc_plant_create(C.byref(m), C.byref(pp), 0, C.byref(h)),
          "wbc_plant_create: mu must be positive and finite, tau_max positive, Kd_contact non-negative and finite")
    gp = plant.WbcGroundParams()
    assert L.wbc_ground_params_default(C.byref(m), C.byref(gp)) == 0
    gp.stiffness = 0.0
    _says(L, L.wbc_ground_create(C.byref(m), C.byref(gp), 0, C.byref(h)),
          "wbc_ground_create: stiffness, mu, v_stiction, tau_max and max_substep must be positive, dissipation non-negative, and all but "
          "tau_max finite")


@pytest.mark.parametrize("fn", ["wbc_create", "wbc_plant_create", "wbc_ground_create", "wbc_ground_params_default"])
def test_model_tables_that_are_refused(L, fn):
    h = C.c_void_p()
    gp = plant.WbcGroundParams()
    call = {"wbc_create": lambda m: L.wbc_create(C.byref(m), 0, None, 8, 0, 0, C.byref(h)),
            "wbc_plant_create": lambda m: L.wbc_plant_create(C.byref(m), None, 0, C.byref(h)),
            "wbc_ground_create": lambda m: L.wbc_ground_create(C.byref(m), None, 0, C.byref(h)),
            "wbc_ground_params_default": lambda m: L.wbc_ground_params_default(C.byref(m), C.byref(gp))}[fn]
    _says(L, call(_model(axis=[0.6, 0.8, 0.0])), fn + ": joint axes must be axis-aligned")
    _says(L, call(_model(axis=[0.0, 0.0, 1.0])), fn + ": " + XYY)
    if fn == "wbc_ground_params_default":      # reads the table only, not the permutations
        return
    twice = list(range(12)); twice[3] = 4
    for kw in (dict(q_perm=twice), dict(act_perm=twice), dict(q_perm=[12] + list(range(1, 12))), dict(act_perm=[-1] + list(range(1, 12)))):
        _says(L, call(_model(**kw)), fn + ": q_perm/act_perm must be permutations of 0..11")


def test_step_argument_checks_behind_the_handle(L):
    b = _blank()
    z = [None] * 9
    f = C.c_float()
    for rc, text in (
            (lambda: L.wbc_step(b, -1, 0, *z), "wbc_step: n out of range (0..max_batch)"),
            (lambda: L.wbc_step(b, 1, 1, *z), "wbc_step: n out of range (0..max_batch)"),
            (lambda: L.wbc_step(b, 0, MAX_LD + 1, *z),
             "wbc_step: ld exceeds WBC_MAX_LD (2^23 instances: the kernels address a row block with 32-bit offsets)"),
            (lambda: L.wbc_time_steps(b, 0, 0, 0, *z, None), "wbc_time_steps: steps must be positive"),
            (lambda: L.wbc_time_steps_result(b, C.byref(f)), "wbc_time_steps_result: no wbc_time_steps call to report"),
            (lambda: L.wbc_time_steps_each(b, 1, 0, 0, *z, None), "wbc_time_steps_each: steps must be positive and ms_each non-null"),
            (lambda: L.wbc_integrate(b, -1, 0, 0.0, None, None, None), "wbc_integrate: bad arguments"),
            (lambda: L.wbc_integrate(b, 2, 1, 0.0, None, None, None), "wbc_integrate: bad arguments"),
            (lambda: L.wbc_rollout(b, b, -1, 1e-3, 0, 0, *N11), "wbc_rollout: steps >= 0, time and vdot are required"),
            (lambda: L.wbc_rollout(b, b, 1, 1e-3, 1, 1, None, None, b, None, None, None, None, None, None, None, b),
             "wbc_step: n out of range (0..max_batch)")):
        _says(L, rc, text)
    assert L.wbc_step(b, 0, 0, *z) == 0 and L.wbc_integrate(b, 0, 0, 0.0, None, None, None) == 0


def test_variant_numbers_of_the_abi(L):
    b = _blank()
    _says(L, L.wbc_set_variant(b, 2),
          "wbc_set_variant: 0 = auto or 3 = 16 lanes per robot (the lane- and quad-per-robot kernels of round 1 are retired)")
    _says(L, L.wbc_set_variant(b, 1),
          "wbc_set_variant: 0 = auto or 3 = 16 lanes per robot (the lane- and quad-per-robot kernels of round 1 are retired)")
    assert L.wbc_set_variant(b, 0) == 0 and L.wbc_set_variant(b, 3) == 0
    assert L.wbc_variant_for(b, 0) == 3 and L.wbc_variant_for(b, 1) == 3 and L.wbc_variant_for(b, 1 << 20) == 3
    _says(L, L.wbc_variant_for(b, -1), "wbc_variant_for: bad argument")


@pytest.mark.parametrize("noun,arrays", [("plant", "q, v, tau and contact_mask"), ("ground", "q, v and tau")])
def test_batch_checks_of_the_plants(L, noun, arrays):
    b = _blank()
    tail = {"plant": (N9, N11, N15), "ground": (N10, N11, N17)}[noun]
    calls = {"wbc_%s_forward" % noun: lambda h, n, ld: getattr(L, "wbc_%s_forward" % noun)(h, None, n, ld, *tail[0]),
             "wbc_%s_step" % noun: lambda h, n, ld: getattr(L, "wbc_%s_step" % noun)(h, None, n, ld, 1e-3, *tail[1]),
             "wbc_%s_rollout" % noun: lambda h, n, ld: getattr(L, "wbc_%s_rollout" % noun)(b, h, b, None, 1, 1e-3, n, ld, *tail[2])}
    for fn, call in calls.items():
        for n, ld, text in ((-1, 0, "n out of range (0 .. WBC_MAX_LD)"), (MAX_LD + 1, MAX_LD + 1, "n out of range (0 .. WBC_MAX_LD)"),
                            (0, MAX_LD + 1, "ld exceeds WBC_MAX_LD"), (4, 3, "ld must be >= n")):
            _says(L, call(None, n, ld), "%s: %s" % (fn, text))
        _says(L, call(None, 4, 4), "%s: null %s handle" % (fn, noun))
        _says(L, call(b, 4, 4), "%s: %s are required" % (fn, arrays))


def test_rollout_checks_of_the_plants(L):
    b = _blank()
    for rc, text in (
            (lambda: L.wbc_plant_rollout(None, b, b, None, 1, 1e-3, 0, 0, *N15), "wbc_plant_rollout: null controller or trajectory handle"),
            (lambda: L.wbc_plant_rollout(b, b, None, None, 1, 1e-3, 0, 0, *N15), "wbc_plant_rollout: null controller or trajectory handle"),
            (lambda: L.wbc_plant_rollout(b, b, b, None, -1, 1e-3, 0, 0, *N15), "wbc_plant_rollout: steps must be >= 0"),
            (lambda: L.wbc_ground_rollout(None, b, b, None, 1, 1e-3, 0, 0, *N17), "wbc_ground_rollout: null controller or trajectory handle"),
            (lambda: L.wbc_ground_rollout(b, b, b, None, -1, 1e-3, 0, 0, *N17), "wbc_ground_rollout: steps must be >= 0"),
            (lambda: L.wbc_ground_rollout(b, b, b, None, 1, 0.0, 0, 0, *N17), "wbc_ground_rollout: dt must be positive and finite"),
            (lambda: L.wbc_ground_step(b, None, 0, 0, -1.0, *N11), "wbc_ground_step: dt must be positive and finite"),
            (lambda: L.wbc_ground_step(b, None, 0, 0, float("inf"), *N11), "wbc_ground_step: dt must be positive and finite"),
            (lambda: L.wbc_ground_step(b, None, 0, 0, float("nan"), *N11), "wbc_ground_step: dt must be positive and finite")):
        _says(L, rc, text)
    q = (C.c_double * 4)()
    p = C.cast(q, C.c_void_p)
    # q, v, tau (and the mask) are there, time and targets are not
    _says(L, L.wbc_plant_rollout(b, b, b, None, 1, 1e-3, 1, 1, p, p, None, None, p, None, None, None, None, p, None, None, None, None, None),
          "wbc_plant_rollout: time and targets are required")
    _says(L, L.wbc_ground_rollout(b, b, b, None, 1, 1e-3, 1, 1, p, p, None, None, None, None, None, None, None, None, p, *([None] * 6)),
          "wbc_ground_rollout: time, targets and contact_mask are required")


def test_terrain_checks(L):
    _says(L, L.wbc_terrain_check(None, 1), "wbc_terrain_check: null profiles")
    b = _blank()
    _says(L, L.wbc_terrain_check(b, 0), "wbc_terrain_check: count must be 1 .. WBC_GROUND_MAX_PROFILES (16)")
    _says(L, L.wbc_terrain_check(b, 17), "wbc_terrain_check: count must be 1 .. WBC_GROUND_MAX_PROFILES (16)")


def test_wire_format_and_pd_argument_checks(L):
    ident = (C.c_int * 12)(*range(12))
    twice = (C.c_int * 12)(*range(12)); twice[3] = 4
    big = (C.c_int * 12)(*range(12)); big[0] = 12
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    odd = C.c_void_p(C.addressof(buf) + 2)
    for fn, call in (("wbc_robot_controls_pack", lambda qp, ap: L.wbc_robot_controls_pack(0, None, 0, 0, None, qp, ap, None)),
                     ("wbc_pd_step", lambda qp, ap: L.wbc_pd_step(0, None, 0, 0, None, None, None, 1.0, 1.0, 1.0, qp, ap, None))):
        _says(L, call(ident, big), fn + ": act_perm must be a permutation of 0..11")
        _says(L, call(None, big), fn + ": act_perm must be a permutation of 0..11")
        _says(L, call(big, ident), fn + ": q_perm / act_perm must be permutations of 0..11")
        _says(L, call(twice, None), fn + ": q_perm / act_perm must be permutations of 0..11")
        _says(L, call(None, twice), fn + ": q_perm / act_perm must be permutations of 0..11")
        assert call(None, None) == 0 and call(ident, ident) == 0        # n = 0: checked, nothing launched
    for rc, text in (
            (lambda: L.wbc_robot_states_unpack(0, None, -1, 0, None, None, None, None), "wbc_robot_states_unpack: bad argument"),
            (lambda: L.wbc_robot_states_unpack(0, None, 1, 1, None, None, None, None), "wbc_robot_states_unpack: bad argument"),
            (lambda: L.wbc_robot_states_unpack(0, None, 1, 1, odd, p, p, None), "wbc_robot_states_unpack: msgs must be 4-byte aligned"),
            (lambda: L.wbc_robot_controls_pack(0, None, 2, 1, None, None, None, None), "wbc_robot_controls_pack: bad argument"),
            (lambda: L.wbc_robot_controls_pack(0, None, 1, 1, p, None, None, odd), "wbc_robot_controls_pack: msgs must be 4-byte aligned"),
            (lambda: L.wbc_pd_step(0, None, 1, 1, None, None, None, 1.0, 1.0, 1.0, None, None, None), "wbc_pd_step: bad argument"),
            (lambda: L.wbc_pd_step(0, None, 0, 0, None, None, None, 1.0, 1.0, -1.0, None, None, None), "wbc_pd_step: u_max must be non-negative"),
            (lambda: L.wbc_pd_step(0, None, 0, 0, None, None, None, 1.0, 1.0, float("nan"), None, None, None), "wbc_pd_step: u_max must be non-negative")):
        _says(L, rc, text)
    h = C.c_void_p()
    ts = (C.c_double * 3)(0.0, 2.0, 1.0)
    tg = (C.c_double * (3 * 54))()
    mk = (C.c_uint8 * 3)()
    _says(L, L.wbc_traj_create(0, 3, ts, tg, mk, C.cast(tg, _lib.c_double_p), 15, 0.0, C.byref(h)),
          "wbc_traj_create: timestamps must be non-decreasing")
    # a NaN timestamp is in no order: refused wherever it stands, in a table of one sample too (no neighbour to compare it with)
    for K, where in ((1, 0), (2, 0), (2, 1), (3, 1)):
        ts = (C.c_double * 3)(0.0, 1.0, 2.0)
        ts[where] = float("nan")
        _says(L, L.wbc_traj_create(0, K, ts, tg, mk, C.cast(tg, _lib.c_double_p), 15, 0.0, C.byref(h)),
              "wbc_traj_create: timestamps must be non-decreasing")
