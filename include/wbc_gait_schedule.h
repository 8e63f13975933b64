/*
 * wbc_gait_schedule.h -- C ABI of the gait planner's command schedules (libwbc_hip.so): every instance walks a sequence of commands
 * (vx, vy, yaw rate) joined by smooth turns, instead of one arc for the whole run.  The conventions are those of wbc_gait.h.
 *
 * The law (this project's definition).  Everything stays a closed form in the time: nothing is integrated, nothing is remembered
 * between ticks, and the body's pose is needed at three path parameters per foot only -- now and the two mid-stances.
 *
 *   Inputs.  Per instance there are m switches, 0 <= m <= 7 (WBC_GAIT_MAX_SWITCHES).  Switch j (1 <= j <= m) has a path parameter
 *   Theta_j and a command c_j = (cx_j, cy_j, omega_j).  c_0 is the instance's cmd and S_0 = (x0, y0, psi0) its start, both from
 *   wbc_gait_set_commands.  One blend length beta >= 0 per call of wbc_gait_set_schedule, in path-parameter units.  The instance is
 *   valid when every number is finite, Theta_1 >= 0 and Theta_j+1 >= Theta_j + beta.
 *
 *   What stays as it is.  The clock, phases, runs, swing splines, masks, theta(t), the `a <= 0` rule for the first footholds
 *   (wbc_gait.h) and the terrain law (wbc_gait_terrain.h) are untouched.  Only the body's pose function P(theta) = (x, y, psi) changes;
 *   it is used for the body rows and for the two mid-stance footholds, F = P_xy(theta(t_m)) + Rz(psi(theta(t_m))) stance_f.
 *
 *   Segment 0 is the arc of c_0 from S_0 at theta = 0 (wbc_gait.h, "Body at path parameter theta").
 *
 *   Segments j >= 1.  Let E_j = (p_E, psi_E) be the pose of segment j-1's arc at Theta_j.  Then
 *     psi_S = psi_E + beta (omega_j-1 + omega_j) / 2,
 *     p_S   = p_E + (beta / 2) (Rz(psi_E) c_j-1 + Rz(psi_S) c_j),
 *   and segment j's arc is the arc formula of wbc_gait.h with command c_j, from S_j = (p_S, psi_S) at theta = Theta_j + beta, with
 *   the arc parameter theta - Theta_j - beta.
 *
 *   Blend window Theta_j <= theta < Theta_j + beta (empty when beta = 0).  With u = (theta - Theta_j) / beta each of x, y and psi is
 *   the quintic that matches value, first and second theta-derivative at both ends.  The first derivative at an end is Rz(psi) c for
 *   the position and omega for the yaw, the second omega z x Rz(psi) c for the position and 0 for the yaw, taken with (c_j-1, psi_E)
 *   at u = 0 and with (c_j, psi_S) at u = 1.  With V = beta (first derivative), A = beta^2 (second derivative),
 *   D = q1 - q0 - V0 - A0 / 2, DV = V1 - V0 - A0 and DA = A1 - A0:
 *     q(u) = q0 + V0 u + A0 u^2 / 2 + k3 u^3 + k4 u^4 + k5 u^5,
 *     k3 = 10 D - 4 DV + DA / 2,   k4 = -15 D + 7 DV - DA,   k5 = 6 D - 3 DV + DA / 2.
 *   For the yaw this gives psi' = omega_j-1 + (omega_j - omega_j-1) (3 u^2 - 2 u^3).
 *
 *   Body rows, from P by the chain rule at theta(tau):  p = P,  pd = theta' P',  pdd = theta'' P' + theta'^2 P'',  likewise rpy_z,
 *   rpyd_z and rpydd_z.  On an arc these are wbc_gait.h's expressions; P is continuous to the second derivative everywhere when
 *   beta > 0 (beta = 0: the pose is continuous, the velocity jumps at Theta_j).
 *
 *   Malformed instances.  An invalid schedule (m > 7 included) gets 54 NaN rows and mask 0xF, like every other malformed instance;
 *   its neighbours keep their bits.  wbc_gait.h's list holds under a schedule as it stands, a clock that does not resolve in double
 *   included.
 *
 *   Exact relation.  An instance with m = 0 gets the bits of the law without a schedule, and so does any instance while all three
 *   of its pose evaluations lie before Theta_1.
 *
 *   The limits.  The stride and the stride scale do not change along the schedule; the schedule itself is a plan: it takes nothing
 *   from the measured state.  What reacts to the measured trunk is a pass after it that shifts the footholds
 *   (include/wbc_gait_feedback.h), with or without a schedule.  The persistent wbc_rollout (wbc.h) takes no gait.
 *
 * Rollouts take the gait handle as their target source (wbc_gait.h), so a schedule set on it steers wbc_ground_rollout and
 * wbc_plant_rollout with no further call.
 */
#ifndef WBC_GAIT_SCHEDULE_H
#define WBC_GAIT_SCHEDULE_H

#include <stdint.h>
#include "wbc_gait.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WBC_GAIT_MAX_SWITCHES 7

/* Resolves the schedules of instances 0 .. n-1 into a buffer the handle owns (one small kernel on hip_stream, one thread per
 * instance, then a wait for that stream): per switch E_j, S_j and the blend's coefficients, which the target kernels then only read.
 * Device arrays: nswitch [n] = m; when [7][ld], row j-1 = Theta_j; cmds [21][ld], rows 3 (j-1) .. 3 (j-1) + 2 = c_j; rows from m on
 * are not read; ld is also the leading dimension of wbc_gait_set_commands' cmd and start.  Everything needed is copied: the three arrays may be freed after the call.  It needs a prior wbc_gait_set_commands,
 * whose cmd and start it reads: call it again after they are rewritten.  From then on wbc_gait_targets follows the schedule; a
 * wbc_gait_targets with a larger n than this call's is an error.  < 0 with the message set, before any device call, for a null
 * handle or array, a negative or non-finite blend, n < 1 or n > WBC_MAX_LD, ld < n or ld > WBC_MAX_LD, or a handle that has had no
 * wbc_gait_set_commands. */
int wbc_gait_set_schedule(wbc_gait g, void* hip_stream, int n, int ld, double blend, const uint8_t* nswitch, const double* when,
                          const double* cmds);
/* The handle walks its one command again: wbc_gait_targets launches the kernels it launches on a handle that never had a schedule. */
int wbc_gait_clear_schedule(wbc_gait g);
/* Registers, scratch bytes per lane, LDS bytes and threads per block of the kernel that runs while a schedule is set: terrain 0 the
 * one without a terrain, otherwise the one with. */
int wbc_gait_schedule_kernel_info(wbc_gait g, int terrain, int* num_vgpr, int* scratch_bytes, int* lds_bytes, int* block_threads);

#ifdef __cplusplus
}
#endif
#endif
