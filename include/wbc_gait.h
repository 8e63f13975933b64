/*
 * wbc_gait.h -- C ABI of the gait planner (libwbc_hip.so): the controllers' 54 target rows and contact mask of a walking quadruped,
 * computed on the device, per instance, from a velocity command.  The conventions are those of wbc.h and wbc_ground.h.
 *
 * The law (this project's definition).  What a trajectory optimiser gives the controllers is a contact schedule, footholds, swing
 * splines and a base motion.  Here the schedule is a table, the base follows a commanded velocity along an exact arc, and the rest
 * has a closed form in the time alone: nothing is integrated, nothing is remembered between calls.
 *
 *   A stride is nphase phases, 1 <= nphase <= 8, phase j with a duration d_j (positive, finite) and a 4-bit contact mask, bit i = foot
 *   i of [LF RF LH RH] in contact.  B_0 = 0, B_j = B_j-1 + d_j-1 (summed in this order, in double); the stride repeats with period
 *   B_nphase.  Boundary j + m nphase (m any integer) is at B_j + m B_nphase.  A handle holds up to 16 strides.  Every foot is in
 *   contact in at least one phase of a stride.
 *
 *   Per-instance inputs (device arrays, wbc_gait_set_commands): cmd [3][ld] = (c_x, c_y, omega), a velocity in the heading frame
 *   [m/s] and a yaw rate [rad/s]; gait_id [n] (NULL: stride 0); stride_scale [n] = s (NULL: 1.0), the instance's durations are the
 *   table's times s; start [3][ld] = (x0, y0, psi0) (NULL: 0).  Handle parameters: stance[4][2], the nominal foot (x, y) in the heading
 *   frame, height, swing_height, ramp_time >= 0, wait_time.
 *
 *   Clock.  tau = time - wait_time.  For tau < 0 the instance gets the standing targets at its start pose -- body at (x0, y0, height)
 *   with rpy (0, 0, psi0), foot f at (x0, y0) + Rz(psi0) stance_f on z = 0, every rate zero -- and mask 0xF.  Otherwise, with
 *   T = s B_nphase and every operation rounded once (no fused multiply-add):
 *     k = floor(tau / T);   if k T > tau: k = k - 1;   if (k + 1) T <= tau: k = k + 1;   r = tau - k T.
 *   The phase is the number of j in 1 .. nphase-1 with r >= s B_j: the phase whose half-open interval [s B_j, s B_j+1) holds r.  The
 *   contact mask is that phase's.  A boundary of the stride in progress, given as B relative to the stride's start, is at the time
 *   k T + s B (a product, a product, a sum).
 *
 *   Path parameter theta(t), for t >= 0.  For t < ramp_time, with x = t / ramp_time:
 *     theta = ramp_time (2.5 x^4 - 3 x^5 + x^6),   theta' = 10 x^3 - 15 x^4 + 6 x^5,   theta'' = 30 x^2 (1 - x)^2 / ramp_time;
 *   from ramp_time on: theta = t - ramp_time / 2, theta' = 1, theta'' = 0 (so ramp_time = 0 gives theta = t).  The gait clock runs in
 *   tau, the body in theta: during the ramp the robot steps in place and accelerates smoothly.
 *
 *   Body at path parameter theta:  psi = psi0 + omega theta,
 *     p_xy = (x0, y0) + theta sinc(omega theta / 2) Rz(psi0 + omega theta / 2) c,   sinc(a) = sin a / a, and 1 - a^2 / 6 for |a| < 1e-4
 *   (the exact arc of a constant velocity c in the heading frame under a constant yaw rate),  p_z = height.  The body rows at tau
 *   are those at theta(tau):  pd_xy = theta' Rz(psi) c,   pdd_xy = theta'' Rz(psi) c + theta'^2 omega z x Rz(psi) c,
 *   rpy = (0, 0, psi), rpyd = (0, 0, omega theta'), rpydd = (0, 0, omega theta''); the z rows of pd and pdd are zero.
 *
 *   Runs.  For each foot, consecutive phases with the same contact bit merge into runs, cyclically across stride boundaries; a run
 *   [a, b) is given by its two boundaries' times.  A foot in contact in every phase has one stance run without beginning or end.
 *   Footholds.  The foothold of a stance run [a, b) is the nominal stance point under the body's pose at mid-stance t_m = (a + b) / 2:
 *     F = p_xy(theta(t_m)) + Rz(psi(theta(t_m))) stance_f;
 *   for a run with a <= 0 (and for the run without beginning) it is the stance point at the start pose, theta = 0.
 *   A stance foot's target is (F, 0) with zero velocity and acceleration.
 *   Swing.  In a swing run [a, b) with D = b - a and u = (tau - a) / D the foot goes from the foothold A of the stance run that ends at
 *   a to the foothold B of the one that begins at b:
 *     xy = A + (B - A) sigma(u),  sigma = 10 u^3 - 15 u^4 + 6 u^5;   z = swing_height 64 u^3 (1 - u)^3;
 *   velocity and acceleration are the analytic derivatives in time (sigma' / D, sigma'' / D^2, likewise z), so position, velocity and
 *   acceleration are continuous at lift-off and touch-down.  A swing run that is under way at tau = 0 (it wraps the stride's
 *   boundary, or phase 0 lifts the foot) starts from the start stance point in mid-air: only strides whose phase 0 has all feet down
 *   begin at rest.
 *
 *   Malformed instances -- a gait_id >= count, a stride_scale that is not positive and finite, a non-finite command, start or time --
 *   get all 54 rows NaN and mask 0xF; the tick then answers status 2 as it does for any NaN target.  Other instances are not touched
 *   by them.  An instance whose clock does not resolve in double is malformed as well: T = s B_nphase is zero or not finite (at any
 *   time); or, for tau >= 0, k T is not finite, or for some foot that has a run the run [a, b) of the phase in progress, a and b formed
 *   as the law forms them (k T + s B, in double), does not have b - a positive and finite.  A foot that is in contact in every phase
 *   has no run and decides nothing here.  (A stride scale of 1e-17, a time of 1e300 s: both ends of a run round to one double.)  So no
 *   instance is answered half in NaN.
 *
 *   The limits.  Without a terrain set on the handle (wbc_gait_terrain.h) the swing knows no terrain: over a
 *   knot the follow law (wbc_ground.h) lifts a swing target by the height under it, and the target jumps at a riser; and footholds
 *   are not moved away from edges.  With one set, the footholds keep clear of the steep pieces and the swing clears what lies between
 *   them: that header has the law and its own limits.  The law is a function of the time and the command
 *   arrays alone: a caller may rewrite cmd, gait_id, stride_scale or start between calls, and the body pose and the footholds then
 *   jump.  A command that changes along the way, with a blended transition and inside a rollout too, is a schedule
 *   (include/wbc_gait_schedule.h: up to seven switches per instance, joined by smooth turns); the stride and its scale
 *   still hold for the whole run.  wbc_gait_targets takes nothing from the measured state; footholds that react to the measured
 *   trunk are a pass after it (include/wbc_gait_feedback.h: wbc_gait_targets_measured, on the plane only).  The
 *   persistent wbc_rollout (wbc.h) takes no gait: its lookup is part of the tick kernels.
 *
 * Rollouts.  While a gait is set on a plant handle (wbc_ground_set_gait, wbc_plant_set_gait), wbc_ground_rollout / wbc_plant_rollout
 * take every tick's targets and contact_mask from wbc_gait_targets instead of wbc_traj_lookup, and `traj` may be NULL: the order is
 * gait -> follow (if set) -> wbc_step -> plant step.  With no gait set a rollout issues exactly the launches it issues without this
 * header.
 */
#ifndef WBC_GAIT_H
#define WBC_GAIT_H

#include <stdint.h>
#include "wbc_plant.h"
#include "wbc_ground.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WBC_GAIT_MAX_PHASES 8
#define WBC_GAIT_MAX_STRIDES 16

typedef struct { int nphase; double duration[8]; uint8_t contact[8]; } wbc_gait_stride;
typedef struct { double stance[4][2], height, swing_height, ramp_time, wait_time; } wbc_gait_params;
typedef struct wbc_gait_s* wbc_gait;

/* Host arithmetic only, no device call: < 0 with the message set for null arguments, count outside 1 .. 16, a non-finite parameter or
 * ramp_time < 0, an nphase outside 1 .. 8, a duration that is not positive and finite, a contact mask above 0xF, or a foot that is
 * in contact in no phase of a stride. */
int wbc_gait_check(const wbc_gait_params* params, const wbc_gait_stride* strides, int count);
/* wbc_gait_check, then a handle for `device`.  Host work only: the packed table goes to the device with wbc_gait_set_commands. */
int wbc_gait_create(const wbc_gait_params* params, const wbc_gait_stride* strides, int count, int device, wbc_gait* out);
int wbc_gait_destroy(wbc_gait g);
/* Remembers the per-instance device pointers cmd [3][ld] (required), gait_id [n], stride_scale [n] and start [3][ld] (each optional);
 * ld is that of the later wbc_gait_targets calls, every array must be as long as their n asks and stay alive in the caller's hands.
 * The first call uploads the table (synchronising with the device). */
int wbc_gait_set_commands(wbc_gait g, const double* cmd, const uint8_t* gait_id, const double* stride_scale, const double* start);
/* targets [54][ld] (layout: wbc.h) and contact_mask [n] of the instances at time [n]; all 54 rows and the mask of every instance are
 * written, columns n .. ld are not touched.  n = 0: success, nothing is launched.  < 0 with the message set, before any device call,
 * for a null handle, n < 0 or n > WBC_MAX_LD, ld < n or ld > WBC_MAX_LD, null time, targets or contact_mask with n > 0, or a handle
 * that has had no wbc_gait_set_commands. */
int wbc_gait_targets(wbc_gait g, void* hip_stream, int n, int ld, const double* time, double* targets, uint8_t* contact_mask);
/* Registers, scratch bytes per lane, LDS bytes and threads per block of the gait kernel. */
int wbc_gait_kernel_info(wbc_gait g, int* num_vgpr, int* scratch_bytes, int* lds_bytes, int* block_threads);
/* The target source of this plant handle's rollout (above); gait NULL: the trajectory again.  < 0 with the message set, before any
 * device call, for a null plant handle or a gait handle created for another device than the plant's.  The gait handle must outlive
 * its use. */
int wbc_ground_set_gait(wbc_ground g, wbc_gait gait);
int wbc_plant_set_gait(wbc_plant p, wbc_gait gait);

#ifdef __cplusplus
}
#endif
#endif
