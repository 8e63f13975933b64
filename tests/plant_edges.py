"""Shared pieces of the plant edge tests (tests/test_plant_edges_gpu.py and their host twins in tests/test_ground_cpu.py and
tests/test_plant_cpu.py): joint / actuator renumbering, arrays with ld > n whose padding is watched, the handle parameters that
differ from every default, the malformed-instance table of the two plants (the plants' counterpart of tests/poisons.py) and the
heterogeneous trot start of the ground closed loop.  Test infrastructure only."""
import math

import numpy as np

import ground_oracle as go

BAD, CLIP = 8, 4

# ---- padding: what the columns n .. ld-1 hold before a call.  Inputs: NaN (read by mistake, it poisons the answer).  Outputs and
# in-place arrays: a bit pattern no kernel produces (a finite double, so that it cannot be mistaken for a NaN input).
SENT_F64 = np.array([0xC0DEC0DEC0DEC0DE], np.uint64).view(np.float64)[0]
SENT_I32 = np.int32(-559038737)          # 0xDEADBEEF
SENT_U8 = np.uint8(0xA5)


def sentinel(dtype):
    return {np.dtype(np.float64): SENT_F64, np.dtype(np.int32): SENT_I32, np.dtype(np.uint8): SENT_U8}[np.dtype(dtype)]


def wide(a, ld, fill=None):
    """a[..., :n] embedded in an array of ld columns; the padding holds `fill` (default: the dtype's sentinel)."""
    a = np.asarray(a)
    out = np.empty(a.shape[:-1] + (ld,), a.dtype)
    out[...] = sentinel(a.dtype) if fill is None else fill
    out[..., :a.shape[-1]] = a
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32, 1: np.uint8}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def padding_kept(a, n, fill=None):
    """The columns n .. of `a` still hold `fill` (default: the dtype's sentinel), bit for bit."""
    a = np.asarray(a)
    pad = a[..., n:]
    want = np.empty_like(pad)
    want[...] = sentinel(a.dtype) if fill is None else fill
    return same_bits(pad, want)


def rel(a, b):
    return np.abs(a - b).max() / (1.0 + np.abs(b).max())


# ---- renumbering
def perm_pair(seed, avoid=None):
    """(q_perm, act_perm): random permutations of 0..11 whose squares have no fixed point, so that p[j] != p^-1[j] for EVERY j
    (a permutation taken for its inverse in any single row address moves data), and act_perm differs from `avoid` everywhere."""
    rng = np.random.default_rng(seed)

    def one(avoid_):
        while True:
            p = rng.permutation(12)
            if (p[p] != np.arange(12)).all() and (avoid_ is None or (p != np.asarray(avoid_)).all()):
                return p
    return one(None), one(avoid)


def permute_rows(q, v, q_perm):
    """The caller's arrays under q_perm: canonical joint j lives in row 7 + q_perm[j] of q and 6 + q_perm[j] of v."""
    q2, v2 = q.copy(), v.copy()
    q2[7 + q_perm] = q[7:]
    v2[6 + q_perm] = v[6:]
    return q2, v2


def canonical_q(q2, q_perm):
    out = q2.copy()
    out[7:] = q2[7 + q_perm]
    return out


def canonical_v(v2, q_perm):
    """Rows of a v-shaped array (v, vdot) back in canonical order."""
    out = v2.copy()
    out[6:] = v2[6 + q_perm]
    return out


def tau_for_identity(tau, act_perm):
    """The torques that a handle with act_perm = identity needs to apply what `tau` applies under `act_perm`."""
    out = np.empty_like(tau)
    out[np.asarray(act_perm)] = tau
    return out


def table_with(table, act_perm):
    t = dict(table)
    t["act_perm"] = [int(x) for x in act_perm]
    return t


# ---- handle parameters that differ from every default (scaled per model)
def odd_ground_params(table, q):
    """foot_radius 0.7 mm, tau_max 25, mu 0.45, 1.7 x stiffness, dissipation 3.0, v_stiction 0.02 and fall_height at the median
    trunk height of the batch `q`.  Torques of draw() are uniform in +-30: about nine instances in ten clip, the others do not."""
    d = go.defaults(table)
    return dict(foot_radius=0.7e-3, tau_max=25.0, mu=0.45, stiffness=1.7 * d["stiffness"], dissipation=3.0, v_stiction=0.02,
                fall_height=float(np.median(q[6])))


def ground_params_that_matter(t, q, v, tau, sp, we, over):
    """The parameters of `over` whose default gives the dense plant another answer (vdot by more than 1e-6, or other flags) on
    this batch: a kernel that were handed the default instead could not meet the dense plant there."""
    d = go.defaults(t)
    ref = go.forward(t, q, v, tau, mass_scale=sp, ext_wrench=we, P=go.params(t, over))
    out = set()
    for k in over:
        if k != "max_substep":
            alt = go.forward(t, q, v, tau, mass_scale=sp, ext_wrench=we, P=go.params(t, dict(over, **{k: d[k]})))
            if rel(alt[0], ref[0]) > 1e-6 or not np.array_equal(alt[3], ref[3]):
                out.add(k)
    return out


def ground_margin_keep(t, q, v, tau, sp, P, backend, idx=None, mu=None):
    idx = range(q.shape[1]) if idx is None else idx
    return np.array([go.margin(t, q[:, i], v[:, i], tau[:, i], mu=None if mu is None else mu[i], s_p=1.0 if sp is None else sp[i],
                               P=P, backend=backend) > 1e-6 for i in idx])


# ---- malformed instances of the plants.  A batch is a dict of q [19, n], v [18, n], tau [12, n], mu [n], mass_scale [n] and
# ext_wrench [6, n] (compliant ground) or mask [n] (rigid contacts); an entry damages column i in place.
def _set(arr, row, val):
    def f(b, i):
        b[arr][row, i] = val
    return f


def _vec(arr, val):
    def f(b, i):
        b[arr][i] = val
    return f


def _scale_quat(s):
    def f(b, i):
        b["q"][0:4, i] *= s
    return f


def _clip_and(damage, row, torque):
    def f(b, i):
        damage(b, i)
        b["tau"][row, i] = torque
    return f


def plant_poisons(act_perm, ground, over_limit):
    """name -> (damage, expected): expected "bad" (flags == BAD exactly), "clip_bad" (flags == CLIP | BAD exactly: the handle
    has a finite tau_max below `over_limit`) or "legal" (an input that only looks odd: answered, no BAD).
    Joint angle, joint rate and torque are damaged once per leg with each of NaN, +inf and -inf, so that each of the four lanes of
    a quad is the one that sees the value; the torque row is the actuator that drives that leg's joint (act_perm^-1)."""
    act_inv = np.argsort(np.asarray(act_perm))
    P = {}
    vals = (("nan", np.nan), ("inf", np.inf), ("ninf", -np.inf))
    for k, (nm, x) in enumerate(vals):
        P[nm + "_quat"] = (_set("q", k, x), "bad")
        P[nm + "_position"] = (_set("q", 4 + k, x), "bad")
        P[nm + "_base_rate"] = (_set("v", 2 * k, x), "bad")
        for leg in range(4):
            j = 3 * leg + (leg + k) % 3
            P["%s_joint_leg%d" % (nm, leg)] = (_set("q", 7 + j, x), "bad")
            P["%s_joint_rate_leg%d" % (nm, leg)] = (_set("v", 6 + j, x), "bad")
            # an infinite torque is also over any finite limit: the header's CLIP rule holds for it too
            P["%s_torque_leg%d" % (nm, leg)] = (_set("tau", int(act_inv[j]), x), "bad" if nm == "nan" else "clip_bad")
    if ground:
        P["nan_ext_wrench"] = (_set("ext_wrench", 4, np.nan), "bad")
        P["inf_ext_wrench"] = (_set("ext_wrench", 1, np.inf), "bad")
    for nm, x in (("nan", np.nan), ("inf", np.inf), ("negative", -0.7), ("zero", 0.0)):
        P[nm + "_mu"] = (_vec("mu", x), "bad")
    for nm, x in (("zero", 0.0), ("inf", np.inf), ("nan", np.nan)):
        P[nm + "_mass_scale"] = (_vec("mass_scale", x), "bad")
    P["zero_quat"] = (_scale_quat(0.0), "bad")
    P["tiny_quat"] = (_scale_quat(1e-170), "bad")             # |q|^2 underflows
    P["huge_rate"] = (_set("v", 0, 1e200), "bad")             # finite input, overflows inside
    P["nonunit_quat"] = (_scale_quat(3.7), "legal")
    for leg in range(4):                                      # the over-limit torque on one lane, the NaN on another
        other = 3 * ((leg + 1) % 4) + 1
        P["clip_with_bad_leg%d" % leg] = (_clip_and(_set("q", 7 + other, np.nan), int(act_inv[3 * leg + 2]), -over_limit), "clip_bad")
    P["clip_with_bad_mu"] = (_clip_and(_vec("mu", np.nan), int(act_inv[4]), over_limit), "clip_bad")
    return P


def slots_of(j, n=80):
    """The instances that kind number j damages in a batch of n = 80 (five wavefronts of 16 robots): robot slot s of a wavefront
    is damaged in wavefront (s + j) mod 5, so one launch puts the kind into each of the 16 slots once, next to clean quads."""
    assert n % 16 == 0
    nw = n // 16
    return np.array(sorted(16 * ((s + j) % nw) + s for s in range(16)))


def copy_batch(b):
    return {k: (np.array(x, copy=True) if isinstance(x, np.ndarray) else x) for k, x in b.items()}


def ground_batch(model, n, seed):
    t, q, v, tau, sp, we = go.draw_near_stance(model, n, seed)
    return t, dict(q=q, v=v, tau=tau, mu=np.random.default_rng(seed + 1).uniform(0.3, 1.0, n), mass_scale=sp, ext_wrench=we)


def rigid_batch(cfg, n, seed):
    from quadruped_drake_amd import load_model, workloads
    b = workloads.make_batch(cfg, n=n, seed=seed)
    rng = np.random.default_rng(seed + 7)
    return load_model(b["model"]), dict(q=b["q"].copy(), v=b["v"].copy(), tau=rng.uniform(-10.0, 10.0, (12, n)),
                                        mask=(np.arange(n) % 16).astype(np.uint8), mu=rng.uniform(0.3, 1.0, n),
                                        mass_scale=rng.uniform(0.8, 1.2, n))


# ---- the ground closed loop's start
def trot_ground_start(n, seed, model="mini_cheetah"):
    """Heterogeneous starts of a trot on the ground: joints +-0.02 rad about the nominal stance, the lowest foot 0.5 mm into the
    ground, trot phase in 0 .. 0.6 s.  -> (q0, v0, t0)"""
    from quadruped_drake_amd import load_model, workloads
    t = load_model(model)
    rng = np.random.default_rng(seed)
    q, v = workloads.nominal_state(model, n)
    q[7:] += rng.uniform(-0.02, 0.02, (12, n))
    for i in range(n):
        q[6, i] -= go._feet_z(t, q[:, i]).min() + 0.5e-3
    return q, v, rng.uniform(0.0, 0.6, n)


def substep_cases():
    """(S, dt) at the default max_substep of 62.5 us: one substep, an odd count, the default 16 at 1 kHz, and a period that the
    default substep does not divide (dt = 2.05 ms -> 33 substeps of 62.1 us)."""
    return [(1, 6e-5), (5, 3e-4), (16, 1e-3), (33, 2.05e-3)]


assert all(max(1, int(math.ceil(dt / 6.25e-5 * (1.0 - 1e-12)))) == s for s, dt in substep_cases())
