/*
 * wbc_gait_feedback.h -- C ABI of the gait planner's foot-placement feedback (libwbc_hip.so): a pass that runs after the gait's target
 * kernel and shifts the footholds by what the measured trunk asks for (Raibert's heuristic; with the default gain, the capture
 * point).  The conventions are those of wbc_gait.h.
 *
 * The law (this project's definition).  The pass reads the 54 target rows and the contact mask that wbc_gait_targets just wrote, the
 * time, and the measured q and v (layout: wbc.h).  It keeps a small state per instance, in a buffer the gait handle owns, and it
 * adds an (x, y) offset to the foot rows.  It does not care which of the gait's kernels wrote the rows: a command schedule
 * (include/wbc_gait_schedule.h) composes with no further code.
 *
 *   Parameters.  k_v [s]: velocity gain;  k_p: position gain;  d_max [m] > 0: the largest offset;  u_hold in [0, 1]: the swing
 *   fraction up to which a swing's landing offset still follows the measurement.  All four finite and non-negative.
 *
 *   State.  Per instance and foot three world-frame offsets in (x, y): cur, of the foothold the foot stands on; from and to, of the
 *   swing in progress.  Per instance the contact mask of the previous call.  wbc_gait_set_feedback zeroes the offsets and sets the
 *   previous mask to 0xF.
 *
 *   Per call, per instance.  With p = target rows 0 .. 1, pd = rows 3 .. 4 (the body's planned position and velocity):
 *     e_p = q[4:6] - p,   e_v = v[3:5] - pd,   d_raw = k_v e_v + k_p e_p   (two products and a sum per component),
 *     |d_raw| = sqrt(d_raw_x^2 + d_raw_y^2),   d = d_raw min(1, d_max / |d_raw|),   d = 0 when |d_raw| = 0.
 *   Every operation of the pass is rounded once: nothing is contracted into a fused multiply-add, as in wbc_gait.h's clock.
 *   An instance is left exactly as it is -- rows, state and previous mask -- when one of those eight numbers, one of its 54 target
 *   rows (the gait's NaN answer to a malformed instance, wbc_gait.h's unresolved clock included) or its time is not finite; `offsets` gets NaN for it.  Its neighbours are
 *   not touched by it.
 *
 *   Per foot f.  The clock is wbc_gait.h's.  With e the six numbers of the packed stride for (foot, phase), a = k T + s e[0] and
 *   b = k T + s e[1] (the run the foot is in, as the gait computes it),  D = b - a,  u = (tau - a) / D,
 *     sigma = 10 u^3 - 15 u^4 + 6 u^5,   sigma' = 30 u^2 (1 - u)^2,   sigma'' = 60 u (1 - u) (1 - 2 u)   (wbc_gait.h, "Swing").
 *   Foot in the air (mask bit clear):
 *     previous bit set -- lift-off:  from = cur,  to = d;     otherwise, if u <= u_hold:  to = d;
 *     rows:  p_xy += from + (to - from) sigma,   pd_xy += (to - from) sigma' / D,   pdd_xy += (to - from) sigma'' / D^2.
 *     The rates treat `to` as a constant: while u <= u_hold the landing offset moves with the measurement, and the target's
 *     velocity and acceleration do not carry that motion.
 *   Foot down (mask bit set):
 *     previous bit clear -- touch-down:  cur = to;     rows:  p_xy += cur.
 *   Then the previous mask becomes the current one.  The z rows, the body rows and the mask are not written.  Before wait_time the
 *   mask is 0xF and the law adds what the feet stand on: zero on a fresh state.
 *
 *   Exact relations.  k_v = k_p = 0, or a measurement equal to the plan, gives offsets of exactly zero: every row equals
 *   wbc_gait_targets'.  Position, velocity and acceleration of a foot stay continuous across lift-off and touch-down while the
 *   measurement's error is constant.
 *
 *   The limits.  With a terrain on the handle (wbc_gait_set_terrain) wbc_gait_targets_measured is an error: a shifted foothold would
 *   need its height and its riser clearance evaluated again, which is the step after this one.  Only footholds react: the body rows
 *   and the clock take nothing from the measurement, and the stride and its scale hold for the whole run.  The state is advanced
 *   once per call: call it once per tick, with times that do not run backwards.  The persistent wbc_rollout (wbc.h) takes no gait.
 *
 * Rollouts.  While feedback is set on the gait handle that a plant handle carries (wbc_ground_set_gait, wbc_plant_set_gait),
 * wbc_ground_rollout and wbc_plant_rollout take their targets from wbc_gait_targets_measured, fed with the rollout's own q and v: the
 * order is gait -> feedback -> follow (if set) -> wbc_step -> plant step, one more launch per tick.  The state carries over from one
 * rollout call to the next.  With no feedback set a rollout issues exactly the launches it issues without this header.
 */
#ifndef WBC_GAIT_FEEDBACK_H
#define WBC_GAIT_FEEDBACK_H

#include <stdint.h>
#include "wbc_gait.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct { double k_v, k_p, d_max, u_hold; } wbc_gait_feedback_params;

/* Host arithmetic only, no device call: < 0 with the message set for null params, a parameter that is negative or not finite,
 * d_max = 0 or u_hold > 1. */
int wbc_gait_feedback_check(const wbc_gait_feedback_params* params);
/* out <- k_v = sqrt(height / 9.81) (the capture point's gain for the gait's body height), k_p = 0, d_max = 0.10, u_hold = 0.5.
 * Host arithmetic only; < 0 for a null argument or a height that is not positive and finite. */
int wbc_gait_feedback_params_default(const wbc_gait_params* gait_params, wbc_gait_feedback_params* out);
/* Allocates and zeroes the state of n instances on the handle's device (synchronising with it); on a handle that has feedback
 * already: resets it.  wbc_gait_targets is not changed by it.  < 0 with the message set, before any device call, for a null handle,
 * what wbc_gait_feedback_check refuses, or n outside 1 .. WBC_MAX_LD. */
int wbc_gait_set_feedback(wbc_gait g, const wbc_gait_feedback_params* params, int n);
/* Frees the state (synchronising with the device when there was one): the handle is what it was before wbc_gait_set_feedback. */
int wbc_gait_clear_feedback(wbc_gait g);
/* wbc_gait_targets(g, hip_stream, n, ld, time, targets, contact_mask), unchanged, then the pass on the same stream with the device
 * arrays q [19][ld] and v [18][ld].  offsets (optional) [8][ld]: rows 2 f, 2 f + 1 <- the (x, y) offset added to foot f's position --
 * cur in stance, from + (to - from) sigma in swing; columns n .. ld of targets and offsets are not touched.  n = 0: success, nothing
 * is launched.  < 0 with the message set, before any device call, for a null handle, n or ld outside the ranges wbc_gait_targets
 * checks, null time, q, v, targets or contact_mask with n > 0, a handle without wbc_gait_set_commands, without
 * wbc_gait_set_feedback or with a terrain set, or n larger than wbc_gait_set_feedback's. */
int wbc_gait_targets_measured(wbc_gait g, void* hip_stream, int n, int ld, const double* time, const double* q, const double* v,
                              double* targets, uint8_t* contact_mask, double* offsets);
/* Registers, scratch bytes per lane, LDS bytes and threads per block of the pass's kernel. */
int wbc_gait_feedback_kernel_info(wbc_gait g, int* num_vgpr, int* scratch_bytes, int* lds_bytes, int* block_threads);

#ifdef __cplusplus
}
#endif
#endif
