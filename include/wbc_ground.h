/*
 * wbc_ground.h -- C ABI of the batched compliant-ground plant (libwbc_hip.so, next to include/wbc.h and include/wbc_plant.h).
 *
 * The rigid-contact plant of wbc_plant.h holds every scheduled stance foot with a bilateral constraint and only reports where a real
 * ground would have let go.  This plant has a ground: the plane z = 0, a compliant half-space that touches each foot in a point.
 * The ground force is an explicit function of the state, so a foot that is lifted is free, a foot that lands is caught, a foot whose
 * tangential load exceeds the friction cone slides, and a robot that tips falls.  No contact schedule enters.
 *
 * The model (this project's definition; unpinned at Drake like every other number here).  For foot c with world position p_c and
 * velocity pd_c = J_c v:
 *   phi = foot_radius - p_c,z.   If phi <= 0:  f_c = 0, exactly.   Otherwise
 *   f_n = stiffness * phi * max(0, 1 - dissipation * pd_c,z)                       (Hunt-Crossley)
 *   v_t = (pd_x, pd_y),   f_t = -mu_p f_n v_t / max(|v_t|, v_stiction),   f_c = (f_t, f_n).
 * Below v_stiction the friction force is a viscous damper, so a loaded foot under a tangential load CREEPS, at up to v_stiction.
 * One substep of length h = dt / S, everything evaluated at the substep's start state:
 *   tau_a = clip(tau, -tau_max, +tau_max), held over the whole step, mapped to S' tau_a through act_perm / q_perm;
 *   M vd + Cv + tau_g = S' tau_a + w_ext + sum_c J_c' f_c,   the trunk mass and inertia scaled by s_p exactly as wbc_plant scales it;
 *   w_ext: an optional external wrench on the trunk, ext_wrench [6][ld], world frame, rows as v's base rows ([torque about the trunk
 *   origin; force]), held over the step (the push of a push-recovery test);
 *   then the arithmetic of wbc_integrate with step h.
 * S = ceil(dt / max_substep) is computed on the host (with 1e-12 relative slack, so that dt = 8 max_substep gives 8); all S substeps
 * of a step run inside one kernel launch with the state in registers.
 * Defaults (wbc_ground_params_default): stiffness = (the robot's weight at s_p = 1) / delta with delta = 1e-3 m, dissipation =
 * 1 / sqrt(g delta) -- the estimate Drake documents for its penetration allowance --, mu = 1.0 (the reference's ground,
 * simulate.py:43-46), v_stiction = 0.05 m/s, foot_radius = 0, tau_max = +inf, max_substep = 6.25e-5 s (16 substeps of a 1 ms period), fall_height = 0.
 * An explicit substep on a mode of stiffness k, damping c and effective mass m_e is stable iff 2 h c / m_e + h^2 k / m_e < 4; the
 * hardest mode is friction on the foot's own small effective mass (c = mu f_n / v_stiction), which is why neither a stiction speed
 * of 1e-3 m/s nor a substep of 1 ms can be used here (profiles/r08/ground.md has the sweep).
 *
 * Terrain (wbc_ground_set_terrain; this project's definition too).  A terrain is a height field that varies along ONE horizontal
 * direction: H(x, y) = scale * h(s) with s = (x - x0) cos(yaw) + (y - y0) sin(yaw), h piecewise linear through nk knots (s_k, h_k),
 * 1 <= nk <= 8, s_k strictly increasing, h constant outside the knots.  A vertical riser is a steep segment (TOWR's Block makes its
 * riser over 0.03 m).  A handle holds up to 16 profiles; instance i stands on profile terrain_id[i], scaled by terrain_scale[i].
 * For a foot at p with velocity pd let j be the segment whose half-open interval [s_j, s_j+1) holds the foot's s, with
 *   g = scale (h_j+1 - h_j) / (s_j+1 - s_j)   and   n = (-g cos(yaw), -g sin(yaw), 1) / sqrt(1 + g^2)
 * (g = 0, n = z before the first and from the last knot on).  The force law is the one above, written about n:
 *   phi = foot_radius - (p_z - H(p_x, p_y)) n_z            (the distance to the segment's plane).   If phi <= 0: f_c = 0, exactly.
 *   v_n = pd . n,   f_n = stiffness * phi * max(0, 1 - dissipation * v_n),   v_t = pd - v_n n,
 *   f_c = f_n n - mu_p f_n v_t / max(|v_t|, v_stiction)                          (world frame, as before).
 * SLIP is the same |v_t| > v_stiction on a loaded foot, FELL becomes "the trunk origin at or below H(q_x, q_y) + fall_height",
 * contact bit c is phi > 0.  With g = 0 and H = 0 this is the law of the plane.  The integrator, the substeps and the stability
 * condition are untouched: the stiffness along n is still `stiffness`.  The limits of the model: the contact is first order in the
 * local plane (a foot near a convex knot feels the plane of the segment under it, extended); the normal jumps at a knot; there are
 * no overhangs and no contact with a riser's face from the side beyond what the steep segment gives.
 *
 * Following the ground (wbc_ground_follow_targets, wbc_ground_set_follow; this project's definition).  The planners' 54 target rows
 * (layout: wbc.h) are about the plane z = 0.  The follow law rewrites an instance's rows for the terrain it stands on, from its
 * profile and its terrain_scale.  H(x, y) and g(x, y) are the scaled height and the scaled slope of the piece under (x, y), with the
 * half-open pieces above; s(x, y) = (x - x0) cos(yaw) + (y - y0) sin(yaw), and for a horizontal vector u, u_s = u_x cos(yaw) +
 * u_y sin(yaw).  Modes: WBC_FOLLOW_OFF (nothing), WBC_FOLLOW_LIFT (heights only), WBC_FOLLOW_FIT (heights and the trunk's attitude).
 *   Feet (LIFT and FIT).  Foot i with target position p_i, velocity pd_i, acceleration pdd_i, and H_i, g_i taken at (p_i,x, p_i,y):
 *     p_i,z += H_i,   pd_i,z += g_i (pd_i)_s,   pdd_i,z += g_i (pdd_i)_s;   x and y are untouched.
 *   A foot whose target x or y is not finite is left entirely as it is and takes no part in the fit (a contact foot's target rows
 *   may hold anything -- wbc.h -- and following must not turn such an instance into a status 2).
 *   The fit, over the usable feet: s_m and H_m are the means of s_i and H_i, and
 *     b = sum (s_i - s_m)(H_i - H_m) / sum (s_i - s_m)^2,
 *   b = 0 where fewer than two feet are usable or the denominator is below 1e-12 m^2; with no usable foot H_m = H and s_m = s at the
 *   body target's (x, y), and b = 0.
 *   Body position (LIFT and FIT):  p_z += H_m + b (s(p_x, p_y) - s_m),   pd_z += b (pd)_s,   pdd_z += b (pdd)_s,   b taken as
 *   constant in time.  On a plane this is the plane's height under the body; x and y are untouched, so the body stays over its feet.
 *   Body attitude (FIT only).  R_fit is the rotation about the horizontal axis (-sin(yaw), cos(yaw), 0) by -atan(b): it takes world
 *   z to the fitted plane's normal.  R' = R_fit Rz(yaw_b) Ry(pitch) Rx(roll), rpy' is read from R' (roll' = atan2(R'21, R'22),
 *   pitch' = atan2(-R'20, sqrt(R'00^2 + R'10^2)), yaw' = atan2(R'10, R'00)), and rpyd' = E(rpy')^-1 R_fit E(rpy) rpyd, likewise rpydd,
 *   where E(rpy) maps the rates of rpy to the angular velocity in the world; no E-dot term, as everywhere in this project.  Where
 *   b = 0 (R_fit is the identity) or |cos pitch'| < 1e-9 the nine attitude rows are left as they are.
 *   Untouched: an instance whose terrain_id >= count or whose terrain_scale is not finite keeps its targets bit for bit (the plant
 *   reports it BAD anyway).  Non-finite values in rows that are read flow through the arithmetic and reach the tick, which answers
 *   status 2 as it does today.
 *   The limits: b and the foot slopes jump when a foothold crosses a knot; the attitude follows the fit of the four PLANNED footholds,
 *   stance and swing alike; the follow law does not re-plan footholds for the terrain (the gait planner does, when it is given the
 *   terrain: wbc_gait_terrain.h, whose targets must not be followed again); and the controllers' friction pyramids stay about
 *   world z -- on a slope of grade gamma a controller mu of at most tan(atan(mu_p) - atan|gamma|) keeps an along-slope edge force
 *   inside the plant's cone about the normal (terrain.py: pyramid_mu).
 *
 * Flags, per instance and per step, an int32 bit field:
 *   WBC_GROUND_SLIP  in some substep a loaded foot (f_n > 0) had |v_t| > v_stiction;
 *   WBC_GROUND_FELL  the trunk origin is at or below fall_height at the end of the step (forward: in the given state);
 *   WBC_GROUND_CLIP  some |tau_k| > tau_max (1 + 1e-9) (clipping itself is always applied);
 *   WBC_GROUND_BAD   not answerable: a non-finite value in q, v, tau or ext_wrench, a mu_p or s_p that is not positive and finite, a
 *                    terrain_id beyond the table or a non-finite terrain_scale, or a non-finite result in any substep.  q and v are
 *                    left bit-for-bit untouched, force, vdot and contact are 0, and of the other bits only CLIP is reported.
 *
 * Conventions of wbc.h: SoA with the batch index fastest (row r of instance i at base[r*ld + i]); device pointers only; n <= WBC_MAX_LD,
 * ld >= n; every pointer not named as required may be NULL; 0 on success, < 0 on misuse or a HIP error with the message in
 * wbc_last_error(); nothing throws; every call leaves the calling thread's current HIP device as it found it.  Asynchronous on
 * `hip_stream` (NULL = the default stream).
 */
#ifndef WBC_GROUND_H
#define WBC_GROUND_H

#include <stdint.h>
#include "wbc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WBC_GROUND_SLIP 1
#define WBC_GROUND_FELL 2
#define WBC_GROUND_CLIP 4
#define WBC_GROUND_BAD 8

typedef struct {
  double stiffness;    /* k  [N/m] */
  double dissipation;  /* d  [s/m] */
  double mu;           /* mu_p where no per-instance value is given */
  double v_stiction;   /* v_s  [m/s] */
  double foot_radius;  /* [m] */
  double tau_max;      /* actuator limit [N m] */
  double max_substep;  /* longest explicit substep [s] */
  double fall_height;  /* FELL: trunk origin at or below this height [m] */
} wbc_ground_params;
typedef struct wbc_ground_s* wbc_ground;

/* The defaults for `model` (stiffness and dissipation depend on its weight and gravity). */
int wbc_ground_params_default(const wbc_model* model, wbc_ground_params* out);
/* params NULL = defaults.  The model's joint axes must follow the pattern wbc_create accepts. */
int wbc_ground_create(const wbc_model* model, const wbc_ground_params* params, int device, wbc_ground* out);
int wbc_ground_destroy(wbc_ground g);

/* One force evaluation, no state change.  Required: q [19][ld], v [18][ld], tau [12][ld] (actuator order, as wbc_step writes them).
 * Optional: mu [n] (default params.mu), mass_scale [n] (default 1.0), ext_wrench [6][ld] (default 0), and the outputs vdot [18][ld]
 * (rows in the order of v), force [12][ld] (world frame, ground on foot, row 3*foot + xyz, feet [LF RF LH RH]), contact [n] (bit c:
 * foot c has phi > 0) and flags [n]. */
int wbc_ground_forward(wbc_ground g, void* hip_stream, int n, int ld, const double* q, const double* v, const double* tau,
                       const double* mu, const double* mass_scale, const double* ext_wrench, double* vdot, double* force,
                       uint8_t* contact, int32_t* flags);
/* One control period dt > 0 in S substeps, in place on q and v; time [n] (optional) += dt.  force: the mean over the substeps
 * (impulse / dt); contact: of the last substep; counts [4][ld] (optional, zeroed by the caller): row b += 1 for every step that raises
 * flag bit b. */
int wbc_ground_step(wbc_ground g, void* hip_stream, int n, int ld, double dt, double* q, double* v, double* time, const double* tau,
                    const double* mu, const double* mass_scale, const double* ext_wrench, double* force, uint8_t* contact,
                    int32_t* flags, int32_t* counts);
/* Closed loop: `steps` x (wbc_traj_lookup -> wbc_step(h) -> wbc_ground_step), all on hip_stream (h is bound to it as wbc_set_stream
 * does).  WBC_DEVICE_PTRS handles only; h and g on the same device.  The controller gets the schedule's contact_mask; the ground
 * decides what actually touches.  mu / mass_scale go to the controller, ground_mu / ground_mass_scale / ext_wrench to the plant.
 * Required: q, v, time, targets [54][ld], contact_mask [n], tau [12][ld].  The controller's statistics accumulate in h as they do in
 * wbc_rollout; on return targets / contact_mask / tau / metrics / status / force / contact / flags hold the last tick's values.
 * After wbc_ground_set_follow, with a terrain set, the follow law runs on the targets between the lookup and the tick. */
int wbc_ground_rollout(wbc_handle h, wbc_ground g, wbc_traj traj, void* hip_stream, int steps, double dt, int n, int ld, double* q,
                       double* v, double* time, double* targets, uint8_t* contact_mask, const double* mu, const double* mass_scale,
                       const double* ground_mu, const double* ground_mass_scale, const double* ext_wrench, double* tau,
                       double* metrics, int32_t* status, double* force, uint8_t* contact, int32_t* flags, int32_t* counts);
/* Registers, scratch bytes per lane, LDS bytes and threads per block of the ground-step kernel. */
int wbc_ground_kernel_info(wbc_ground g, int* num_vgpr, int* scratch_bytes, int* lds_bytes, int* block_threads);

/* ---- Terrain (the model: the head of this file).  A profile: nk knots (s[k], h[k]), the direction yaw of s and its origin. */
typedef struct { int nk; double x0, y0, yaw; double s[8]; double h[8]; } wbc_terrain_profile;
#define WBC_GROUND_MAX_PROFILES 16
/* Host arithmetic only, no device call: < 0 with the message set when count is outside 1 .. 16, an nk outside 1 .. 8, knots that are
 * not strictly increasing, or any non-finite number. */
int wbc_terrain_check(const wbc_terrain_profile* profiles, int count);
/* Checks and copies the table to the handle's device (synchronising with it) and remembers the per-instance device pointers
 * terrain_id [n] (NULL: profile 0) and terrain_scale [n] (NULL: 1.0); both must be at least as long as the n of every later call and
 * stay alive in the caller's hands.  count = 0 or profiles = NULL switches the terrain off again.  wbc_ground_forward, wbc_ground_step
 * and wbc_ground_rollout of this handle then run on the terrain.  A terrain_id >= count or a non-finite terrain_scale makes the
 * instance WBC_GROUND_BAD; any finite scale is legal, 0 and negative ones included. */
int wbc_ground_set_terrain(wbc_ground g, const wbc_terrain_profile* profiles, int count, const uint8_t* terrain_id,
                           const double* terrain_scale);
/* wbc_ground_kernel_info of the step kernel that runs while a terrain is set. */
int wbc_ground_terrain_kernel_info(wbc_ground g, int* num_vgpr, int* scratch_bytes, int* lds_bytes, int* block_threads);

/* ---- Following the ground (the law: the head of this file). */
#define WBC_FOLLOW_OFF 0
#define WBC_FOLLOW_LIFT 1
#define WBC_FOLLOW_FIT 2
/* The follow law in place on targets [54][ld], for the terrain set on the handle (its table, terrain_id and terrain_scale); only the
 * rows the law changes are written: the z rows of every usable foot and of the body, in WBC_FOLLOW_FIT also the nine attitude rows.
 * mode = WBC_FOLLOW_OFF, n = 0, or no terrain set: success, and nothing is launched.  < 0 with the message set, before any device
 * call, for a null handle, a mode outside 0 .. 2, n < 0 or n > WBC_MAX_LD, ld < n or ld > WBC_MAX_LD, or null targets with n > 0. */
int wbc_ground_follow_targets(wbc_ground g, void* hip_stream, int n, int ld, int mode, double* targets);
/* What wbc_ground_rollout does between its lookup and its tick: with a mode other than WBC_FOLLOW_OFF (the default) and a terrain set,
 * every tick runs lookup -> follow -> wbc_step -> ground step, and on return targets holds the last tick's followed targets.  With
 * WBC_FOLLOW_OFF or no terrain set the rollout issues exactly the launches it issues without this call. */
int wbc_ground_set_follow(wbc_ground g, int mode);
/* wbc_ground_kernel_info of the follow kernel. */
int wbc_ground_follow_kernel_info(wbc_ground g, int* num_vgpr, int* scratch_bytes, int* lds_bytes, int* block_threads);

#ifdef __cplusplus
}
#endif
#endif
