/*
 * wbc_gait_terrain.h -- C ABI of the gait planner's terrain (libwbc_hip.so): while a terrain is set on a gait handle, the 54 rows
 * of wbc_gait_targets are the finished targets ON that terrain -- footholds on the surface and off the risers, swings that clear what
 * lies between their two footholds, a body that follows the feet -- and no follow pass (wbc_ground.h) runs after
 * them.  With no terrain set every entry point of wbc_gait.h does what it does without this header and launches the
 * kernel it launches without it.
 *
 * The law (this project's definition).  Every quantity that is not named here is wbc_gait.h's: the clock, the runs, theta, the body's
 * arc, the flat law's footholds, u, D, sigma(u) = 10 u^3 - 15 u^4 + 6 u^5.  b(u) = 64 u^3 (1 - u)^3.
 *
 *   Terrain.  Up to 16 wbc_terrain_profile of include/wbc_ground.h, as wbc_terrain_check accepts them.  Instance i walks on profile
 *   terrain_id[i] (NULL: profile 0) scaled by terrain_scale[i] (NULL: 1.0).  With d = (cos yaw, sin yaw) and s(x, y) = (x - x0) d_x +
 *   (y - y0) d_y the height is H(x, y) = scale h(s), h piecewise linear through the knots (s_k, h_k), pieces half open [s_k, s_k+1),
 *   h constant before the first and from the last knot on: wbc_ground.h's definition.  Piece j, 0 <= j <= nk - 2, lies between knots
 *   j and j + 1 and has the slope (h_j+1 - h_j) / (s_j+1 - s_j).
 *
 *   Handle parameters (wbc_gait_terrain_params): body_mode, WBC_GAIT_BODY_LIFT or WBC_GAIT_BODY_FIT; max_grade > 0; edge_margin >= 0;
 *   apex_max >= the gait's swing_height.
 *
 *   Footholds.  F_xy is the flat law's foothold of a stance run and s_F = s(F_xy).  Piece j is steep if |scale slope_j| > max_grade.
 *   Take the pieces in increasing j; for the FIRST steep piece whose open interval (s_j - edge_margin, s_j+1 + edge_margin) holds s_F
 *   the foothold moves along d to the nearer end e of that interval, to the upper end at equal distances (upper - s_F <= s_F - lower
 *   picks the upper end):  F_xy += (e - s_F) d, and the foothold's s is e itself.  One pass, no second look.  A foothold that is not
 *   moved keeps its s_F.  The foothold's height is F_z = scale h(s) at the foothold's s, by the half-open pieces.  The start-pose
 *   footholds -- those of a run with a <= 0, of the run without a beginning, and every foothold while tau < 0 -- are not moved: the
 *   robot stands there; their height is H under them all the same.  A stance foot's target is (F_xy, F_z) with zero velocity and
 *   acceleration.
 *
 *   Swing from the foothold A (s_A, z_A) to the foothold B (s_B, z_B):  xy = A_xy + (B_xy - A_xy) sigma(u) as in wbc_gait.h, and
 *     z = z_A + (z_B - z_A) sigma(u) + a b(u),
 *   velocity and acceleration its analytic derivatives in time.  The apex a: for every knot k of the instance's profile with s_k
 *   strictly between s_A and s_B (in either order) let
 *     lambda_k = (s_k - s_A) / (s_B - s_A),    e_k = scale h_k - (z_A + lambda_k (z_B - z_A)),
 *     a = min(apex_max, swing_height + max(0, max_k e_k / (4 lambda_k (1 - lambda_k)))).
 *   Why this is enough, with no root to find: the foot's s is s_A + (s_B - s_A) sigma, so the terrain under the swing is piecewise
 *   linear in sigma with its kinks at sigma = lambda_k; b >= 4 sigma (1 - sigma) for every u (the ratio is
 *   64 / ((10 - 15 u + 6 u^2)(1 + 3 u + 6 u^2)), between 4 and 6.4); and b is concave as a function of sigma (db / dsigma =
 *   6.4 (1 - 2 u)).  So z - H - swing_height b is concave in sigma between kinks and non-negative at every kink and at both ends:
 *   wherever the cap apex_max does not bite,  z(u) - H(xy(u)) >= swing_height b(u)  for the whole swing -- the foot clears the real
 *   terrain by at least the flat ground's swing profile.  On flat terrain at height 0 the foot rows are wbc_gait.h's, bit for bit.
 *
 *   Body.  Foot f has a ground height g_f(t): F_z in stance, z_A + (z_B - z_A) sigma(u) in swing, with rates (z_B - z_A) sigma' / D
 *   and (z_B - z_A) sigma'' / D^2; it is continuous to the acceleration across lift-off and touch-down.
 *     p_z = height + mean_f g_f, pd_z and pdd_z the means of the rates (every sum over the feet here is taken as (f_0 + f_1) + (f_2 + f_3),
 *   so four equal heights have exactly that mean and a symmetric stance on level ground exactly no tilt); the x and y rows of the
 *   body are wbc_gait.h's.  LIFT leaves rpy = (0, 0, psi).  FIT has fixed lever arms, the handle's stance coordinates centred
 *   on their means, xt_f = stance_f,x - mean_f stance_f,x and yt_f likewise:
 *     P = sum_f xt_f g_f / sum_f xt_f^2,  pitch = -atan P;      Q = sum_f yt_f g_f / sum_f yt_f^2,  roll = +atan Q;
 *     rpy = (roll, pitch, psi), and rpyd, rpydd carry the analytic first and second time derivatives: for pitch
 *     -P' / (1 + P^2) and -(P'' (1 + P^2) - 2 P P'^2) / (1 + P^2)^2 with P', P'' the same sums over the rates of g_f; for roll their
 *     negatives in Q.  A stance with sum xt^2 = 0 or sum yt^2 = 0 is refused with FIT.  The yaw rows are wbc_gait.h's.
 *
 *   Malformed instances.  In addition to wbc_gait.h's (a clock that does not resolve in double among them): a terrain_id >= count or a terrain_scale that is not finite gives 54 NaN rows
 *   and mask 0xF; its neighbours are not touched.
 *
 *   The limits.  The profile varies along one direction only.  The cap apex_max may bite, and then the clearance above is not
 *   guaranteed.  One pass over the steep pieces: where a level tread between two steep pieces is shorter than 2 edge_margin, a moved
 *   foothold may come to lie inside the next steep piece's margin.  e_k / (lambda_k (1 - lambda_k)) loses digits when a knot lies
 *   within rounding of a foothold.  The controllers' friction pyramids stay about world z (wbc_ground.h: pyramid_mu).  The follow law
 *   (include/wbc_ground.h) must not run after a terrain gait: it would lift everything a second time; a rollout of a plant
 *   handle with a follow mode set and a terrain gait does exactly that, and plant.closed_loop refuses the pair.  As in wbc_gait.h, a
 *   caller who rewrites the per-instance arrays between calls makes the footholds jump.
 *
 * Rollouts.  wbc_gait_targets, wbc_ground_set_gait, wbc_plant_set_gait and the rollouts keep their prototypes: a gait handle with a
 * terrain set launches wbc_gait_terrain_targets_kernel wherever it launched wbc_gait_targets_kernel.
 */
#ifndef WBC_GAIT_TERRAIN_H
#define WBC_GAIT_TERRAIN_H

#include <stdint.h>
#include "wbc_ground.h"
#include "wbc_gait.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WBC_GAIT_BODY_LIFT 0
#define WBC_GAIT_BODY_FIT 1

typedef struct { int body_mode; double max_grade, edge_margin, apex_max; } wbc_gait_terrain_params;

/* Host arithmetic only, no device call: < 0 with the message set for null params or profiles, what wbc_terrain_check refuses, a
 * body_mode other than LIFT and FIT, a max_grade that is not positive and finite, an edge_margin that is not non-negative and finite,
 * an apex_max that is not finite.  (What depends on the gait handle -- apex_max >= swing_height, the lever arms of FIT -- is checked
 * by wbc_gait_set_terrain.) */
int wbc_gait_terrain_check(const wbc_gait_terrain_params* params, const wbc_terrain_profile* profiles, int count);
/* Sets the terrain of this gait handle: wbc_gait_terrain_check, apex_max >= the handle's swing_height, with FIT the lever arms; then
 * the packed table goes to the handle's device (synchronising with it, like wbc_ground_set_terrain).  terrain_id [n] and
 * terrain_scale [n] are device arrays (each optional) as long as the n of every later call, and stay alive in the caller's hands.
 * profiles NULL or count 0: the handle is the plain gait again (params is not read, no device call).  Misuse returns < 0 with the
 * message set before any device call, and leaves the handle as it was. */
int wbc_gait_set_terrain(wbc_gait g, const wbc_gait_terrain_params* params, const wbc_terrain_profile* profiles, int count,
                         const uint8_t* terrain_id, const double* terrain_scale);
/* Registers, scratch bytes per lane, LDS bytes and threads per block of the kernel that runs while a terrain is set. */
int wbc_gait_terrain_kernel_info(wbc_gait g, int* num_vgpr, int* scratch_bytes, int* lds_bytes, int* block_threads);

#ifdef __cplusplus
}
#endif
#endif
