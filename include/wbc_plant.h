/*
 * wbc_plant.h -- C ABI of the batched rigid-contact plant step (libwbc_hip.so, next to include/wbc.h).
 *
 * wbc_integrate / wbc_rollout advance the state with the accelerations the controller's own QP planned, so the "robot" is always
 * exactly the controller's model.  A plant step instead applies the controller's torques to a robot of its own: forward dynamics
 * under the applied torques with the stance feet held by rigid (bilateral) contacts, then the semi-implicit Euler step of
 * wbc_integrate.  Per instance i with state q, v, torques tau (actuator order, as wbc_step writes them), contact mask m (bits 0..3,
 * feet [LF RF LH RH]), plant friction mu_p and plant trunk scale s_p:
 *
 *   tau_a = clip(tau, -tau_max, +tau_max), mapped to generalized forces S' tau_a through the model's act_perm / q_perm;
 *   the model of the handle with the trunk mass and inertia scaled by s_p (the meaning of wbc_step's mass_scale);
 *   M vd + Cv + tau_g = S' tau_a + sum_{c in m} J_c' f_c   and   J_c vd + Jdot_c v = -Kd_contact J_c v  for every c in m
 *   (the stance rows of the controllers' QPs); v+ = v + dt vd, then the quaternion, position and joint update of wbc_integrate.
 *
 * Not modelled: ground geometry, unilateral contact, lift-off, slip, impacts.  The plant only REPORTS where a real ground would have
 * let go, per instance and per step in an int32 bit field:
 *   WBC_PLANT_PULL  a stance foot's normal force f_z < -tol (the ground would have had to pull);
 *   WBC_PLANT_CONE  |f_x| or |f_y| > mu_p f_z + tol (outside the plant's friction pyramid);
 *   WBC_PLANT_CLIP  some |tau_k| > tau_max (1 + 1e-9) (clipping itself is always applied);
 *   WBC_PLANT_BAD   not answerable: a non-finite value in q, v or tau, a mu_p or s_p that is not positive and finite, a contact
 *                   system whose Cholesky pivot falls below 1e-12 of its largest pivot, or a non-finite result.  vd = 0, f = 0,
 *                   and q and v are left bit-for-bit untouched;
 *   tol = 1e-9 (sum_{c in m} (|f_x| + |f_y| + |f_z|) + the plant robot's weight): rounding level of the instance's forces, so that
 *   neither a QP force on the boundary of its own cone nor a foot the QP leaves at exactly zero force (where the plant returns
 *   rounding noise) is flagged.
 * With the plant equal to the controller (s_p = mass_scale, no clipping, the same Kd_contact) vd and f are the QP's.
 *
 * Conventions of wbc.h: SoA with the batch index fastest (row r of instance i at base[r*ld + i]); device pointers only; n <= WBC_MAX_LD,
 * ld >= n; every pointer not named as required may be NULL; 0 on success, < 0 on misuse or a HIP error with the message in
 * wbc_last_error(); nothing throws; every call leaves the calling thread's current HIP device as it found it.  Asynchronous on
 * `hip_stream` (NULL = the default stream).
 */
#ifndef WBC_PLANT_H
#define WBC_PLANT_H

#include <stdint.h>
#include "wbc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WBC_PLANT_PULL 1
#define WBC_PLANT_CONE 2
#define WBC_PLANT_CLIP 4
#define WBC_PLANT_BAD 8

/* defaults: Kd_contact = 100 (the controllers' stance-row gain), tau_max = +inf (no clipping), mu = 1.0 (the reference's ground,
 * simulate.py:43-46; not the controllers' 0.7) */
typedef struct {
  double Kd_contact, tau_max, mu;
} wbc_plant_params;
typedef struct wbc_plant_s* wbc_plant;

int wbc_plant_params_default(wbc_plant_params* out);
/* params NULL = defaults.  The model's joint axes must follow the pattern wbc_create accepts. */
int wbc_plant_create(const wbc_model* model, const wbc_plant_params* params, int device, wbc_plant* out);
int wbc_plant_destroy(wbc_plant p);

/* Required: q [19][ld], v [18][ld], tau [12][ld], contact_mask [n].  Optional: mu [n] (default params.mu), mass_scale [n] (default
 * 1.0), and the outputs vd [18][ld] (rows in the order of v), force [12][ld] (world frame, ground on foot, row 3*foot + xyz, 0 for
 * swing feet) and flags [n].  No state change. */
int wbc_plant_forward(wbc_plant p, void* hip_stream, int n, int ld, const double* q, const double* v, const double* tau,
                      const uint8_t* contact_mask, const double* mu, const double* mass_scale, double* vdot, double* force,
                      int32_t* flags);
/* wbc_plant_forward, then the semi-implicit Euler step in place on q and v; time [n] (optional) += dt.  counts [4][ld] (optional,
 * zeroed by the caller): row b += 1 for every step that raises flag bit b. */
int wbc_plant_step(wbc_plant p, void* hip_stream, int n, int ld, double dt, double* q, double* v, double* time, const double* tau,
                   const uint8_t* contact_mask, const double* mu, const double* mass_scale, double* vdot, double* force,
                   int32_t* flags, int32_t* counts);
/* Closed loop: `steps` x (wbc_traj_lookup -> wbc_step(h) -> wbc_plant_step), all on hip_stream (h is bound to it as wbc_set_stream
 * does).  WBC_DEVICE_PTRS handles only; h and p on the same device.  mu / mass_scale go to the controller, plant_mu /
 * plant_mass_scale to the plant.  Required: q, v, time, targets [54][ld], contact_mask [n], tau [12][ld].  The controller's
 * statistics accumulate in h as they do in wbc_rollout; on return targets / contact_mask / tau / metrics / status / force / flags
 * hold the last tick's values. */
int wbc_plant_rollout(wbc_handle h, wbc_plant p, wbc_traj traj, void* hip_stream, int steps, double dt, int n, int ld, double* q,
                      double* v, double* time, double* targets, uint8_t* contact_mask, const double* mu, const double* mass_scale,
                      const double* plant_mu, const double* plant_mass_scale, double* tau, double* metrics, int32_t* status,
                      double* force, int32_t* flags, int32_t* counts);
/* Registers, scratch bytes per lane, LDS bytes and threads per block of the plant-step kernel. */
int wbc_plant_kernel_info(wbc_plant p, int* num_vgpr, int* scratch_bytes, int* lds_bytes, int* block_threads);

#ifdef __cplusplus
}
#endif
#endif
