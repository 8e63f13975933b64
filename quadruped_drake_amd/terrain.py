"""Terrain profiles of the compliant-ground plant (include/wbc_ground.h): height fields that vary along one horizontal direction.

    H(x, y) = scale * h(s),   s = (x - x0) cos(yaw) + (y - y0) sin(yaw),

h piecewise linear through 1 .. 8 knots (s_k, h_k), s_k strictly increasing, h constant outside the knots.  A vertical riser is a
steep segment.  The constructors mirror the terrains the reference ships for its planner (FlatGround, Block, Stairs and Slope of
towr/include/towr/terrain/examples/height_map_examples.h); the numbers are this project's own.  `GroundContactPlant.set_terrain`
takes a list of up to 16 profiles; each instance picks one by `terrain_id` and scales it by `terrain_scale`.
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import WbcTerrainProfile   # wbc_terrain_profile of include/wbc_ground.h

MAX_KNOTS = 8
MAX_PROFILES = 16


class Profile:
    """Knots (s_k, h_k) of h, the direction `yaw` of s in the world's x-y plane and the origin (x0, y0) of s."""

    def __init__(self, s, h, yaw=0.0, x0=0.0, y0=0.0):
        self.s = [float(x) for x in np.atleast_1d(s)]
        self.h = [float(x) for x in np.atleast_1d(h)]
        self.yaw, self.x0, self.y0 = float(yaw), float(x0), float(y0)
        if len(self.s) != len(self.h) or not 1 <= len(self.s) <= MAX_KNOTS:
            raise ValueError("Profile: 1 .. %d knots, as many heights as positions" % MAX_KNOTS)
        if not all(math.isfinite(x) for x in self.s + self.h + [self.yaw, self.x0, self.y0]):
            raise ValueError("Profile: every number must be finite")
        if any(b <= a for a, b in zip(self.s, self.s[1:])):
            raise ValueError("Profile: knot positions must be strictly increasing")

    def __repr__(self):
        return "Profile(s=%r, h=%r, yaw=%r, x0=%r, y0=%r)" % (self.s, self.h, self.yaw, self.x0, self.y0)

    def rotated(self, angle, about=(0.0, 0.0)):
        """The same terrain after rotating the world by `angle` about the vertical through `about`."""
        c, s = math.cos(angle), math.sin(angle)
        dx, dy = self.x0 - about[0], self.y0 - about[1]
        return Profile(self.s, self.h, self.yaw + angle, about[0] + c * dx - s * dy, about[1] + s * dx + c * dy)

    def c_struct(self):
        p = WbcTerrainProfile()
        p.nk, p.x0, p.y0, p.yaw = len(self.s), self.x0, self.y0, self.yaw
        for k in range(len(self.s)):
            p.s[k], p.h[k] = self.s[k], self.h[k]
        return p


def c_array(profiles):
    """A ctypes array of wbc_terrain_profile from a list of Profile."""
    profiles = list(profiles)
    arr = (WbcTerrainProfile * len(profiles))()
    for i, p in enumerate(profiles):
        arr[i] = p.c_struct()
    return arr


def bind(profiles, terrain_id, terrain_scale, device, owner, hint=""):
    """What GroundContactPlant.set_terrain and GaitPlanner.set_terrain share: 1 .. 16 profiles, terrain_id (uint8 [N]) and terrain_scale
    (float64 [N]) on cuda:`device`, where `owner` lives, N read off whichever of the two is given.
    -> (wbc_terrain_profile array as void*, count, terrain_id's pointer, terrain_scale's, the tuple (profiles, terrain_id, terrain_scale, N)
    that the setter stores: it keeps the tensors alive and _check_terrain_n reads its N)"""
    import torch
    profiles = list(profiles) if profiles is not None else []
    if not profiles or not all(isinstance(p, Profile) for p in profiles):
        raise ValueError("set_terrain: profiles must be a non-empty list of terrain.Profile" + hint)
    n = None
    for a in (terrain_id, terrain_scale):
        if a is not None and isinstance(a, torch.Tensor) and a.dim() == 1:
            n = int(a.shape[0]) if n is None else n
    pid = _lib.dev_ptr(terrain_id, 0, n, "uint8", "terrain_id", device, owner, True)
    psc = _lib.dev_ptr(terrain_scale, 0, n, "float64", "terrain_scale", device, owner, True)
    return C.cast(c_array(profiles), C.c_void_p), len(profiles), pid, psc, (profiles, terrain_id, terrain_scale, n)


def _check_terrain_n(terrain, n, refuses, whose=""):
    """terrain: what a set_terrain stored, or None; refuses(held, n): the owner's rule, operator.lt for the plant, which takes a prefix of
    a longer terrain, operator.ne for the planner"""
    if terrain is not None and terrain[3] is not None and refuses(terrain[3], n):
        raise ValueError("%sterrain_id / terrain_scale hold %d instances, the call has %d" % (whose, terrain[3], n))


def flat(height=0.0, **kw):
    """Level ground at `height` (TOWR's FlatGround)."""
    return Profile([0.0], [height], **kw)


def slope(angle, start=0.0, length=100.0, **kw):
    """A plane rising at `angle` [rad] along s from s = start, level before it (the up-ramp of TOWR's Slope, without its end).
    `length` is the run after which the ground is level again; the default is far beyond any run of the plant."""
    return Profile([start, start + length], [0.0, math.tan(angle) * length], **kw)


def ramp_step(start, height, run=0.03, **kw):
    """A kerb of `height` at s = start whose riser is a ramp over `run` (TOWR's Block, which makes its riser over eps = 0.03 m)."""
    return Profile([start, start + run], [0.0, height], **kw)


def stairs(start, tread, rises, run=0.03, **kw):
    """Steps from s = start: rise k climbs rises[k] over `run`, followed by a level tread of `tread` (TOWR's Stairs; up to 4 rises)."""
    rises = [float(r) for r in np.atleast_1d(rises)]
    s, h = [], []
    at, top = float(start), 0.0
    for r in rises:
        s += [at, at + run]
        h += [top, top + r]
        at += run + tread
        top += r
    return Profile(s, h, **kw)


def ridge(start, up, down, height, **kw):
    """Up over `up` to `height`, straight down again over `down`, level after it (TOWR's Slope)."""
    return Profile([start, start + up, start + up + down], [0.0, height, 0.0], **kw)


def evaluate(profile, x, y, scale=1.0):
    """-> (H, n): height [...] and unit normal [..., 3] of the terrain at the world points (x, y), by the header's definition: the
    segment j whose half-open interval [s_j, s_j+1) holds s gives the slope g, and n = (-g cos yaw, -g sin yaw, 1) / sqrt(1 + g^2)."""
    x, y = np.broadcast_arrays(np.asarray(x, float), np.asarray(y, float))
    sk, hk = np.array(profile.s), np.array(profile.h)
    c, sn = math.cos(profile.yaw), math.sin(profile.yaw)
    s = (x - profile.x0) * c + (y - profile.y0) * sn
    j = np.searchsorted(sk, s, side="right")                    # knots at or below s
    inside = (j > 0) & (j < sk.size)
    a = np.clip(j - 1, 0, max(sk.size - 2, 0))
    if sk.size > 1:
        g = np.where(inside, (hk[a + 1] - hk[a]) / (sk[a + 1] - sk[a]), 0.0)
    else:
        g = np.zeros_like(s)
    base = np.where(j == 0, hk[0], hk[np.clip(j - 1, 0, sk.size - 1)])
    H = scale * (base + np.where(inside, g * (s - sk[a]), 0.0))
    g = scale * g
    r = np.sqrt(1.0 + g * g)
    return H, np.stack([-g * c / r, -g * sn / r, 1.0 / r], axis=-1)


SPECS = {"flat": "height [m], default 0", "slope": "angle [rad], default 0.1, rising along +x through the origin",
         "ramp_step": "height [m], default 0.05, 0.3 m ahead", "stairs": "rise [m] of each of three steps, default 0.04, 0.3 m ahead, treads 0.2 m",
         "ridge": "height [m], default 0.1, 0.3 m ahead, 0.5 m up and 0.5 m down"}


def from_spec(spec):
    """A Profile from the command line's NAME[:PARAM] (simulate.py --terrain, tools/ground_bench.py --terrain); SPECS lists them."""
    name, _, par = str(spec).partition(":")
    if name not in SPECS:
        raise ValueError("terrain %r: expected one of %s" % (spec, ", ".join(sorted(SPECS))))
    try:
        x = float(par) if par else None
    except ValueError:
        raise ValueError("terrain %r: the parameter must be a number" % (spec,))
    if name == "flat":
        return flat(0.0 if x is None else x)
    if name == "slope":
        rise = 50.0 * math.tan(0.1 if x is None else x)
        return Profile([-50.0, 50.0], [-rise, rise])
    if name == "ramp_step":
        return ramp_step(0.3, 0.05 if x is None else x)
    if name == "stairs":
        return stairs(0.3, 0.2, [0.04 if x is None else x] * 3)
    return ridge(0.3, 0.5, 0.5, 0.1 if x is None else x)


def pyramid_mu(mu_p, grade):
    """tan(atan(mu_p) - atan|grade|): the largest controller `mu` whose friction pyramid about world z keeps an along-slope edge
    force inside the plant's cone of friction mu_p about the normal of a slope of `grade` (the followed targets tilt the trunk,
    the pyramids stay about z).  <= 0 where the slope is steeper than the cone: no force along world z stays inside it."""
    return math.tan(math.atan(mu_p) - math.atan(abs(grade)))


def stance_pose(profile, x, y, height, scale=1.0):
    """Quaternion (w, x, y, z) and position of a trunk standing square on the terrain above the surface point under (x, y): its
    z axis along the local normal, its origin `height` along the normal above the surface."""
    H, n = evaluate(profile, x, y, scale)
    H, n = float(H), np.asarray(n, float)
    axis = np.array([-n[1], n[0], 0.0])
    sn = float(np.linalg.norm(axis))
    half = 0.5 * math.atan2(sn, n[2])
    quat = np.array([math.cos(half), 0.0, 0.0, 0.0])
    if sn > 0:
        quat[1:] = axis / sn * math.sin(half)
    return quat, np.array([x, y, H]) + height * n
