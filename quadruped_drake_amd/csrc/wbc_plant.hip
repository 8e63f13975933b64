// wbc_plant.hip -- the rigid-contact plant step (include/wbc_plant.h): kernel and C ABI.
//
// Mapping: a quad of lanes per robot, one lane per leg (16 robots per wavefront; 256 wavefronts at N = 4096).  Each lane computes
// its own leg's kinematics, CRBA, RNEA, D^-1, Y / Z columns and joint accelerations (wbc_plant.hpp); the base Schur complement
// and the base right-hand side are summed over the quad; the 6x6 and <= 12x12 Cholesky factorisations are replicated on the quad
// (the same instructions on the same bits: every lane holds the same values).  Cross-lane moves are quad_perm DPP builtins, so
// the compiler's hazard recogniser sees every one of them.  double throughout, SoA I/O with the batch index fastest, and every
// load issued before the first store (q and v are updated in place through run-time strides).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/wbc.h"
#include "../../include/wbc_plant.h"
#include "../../include/wbc_gait.h"
#include "../../include/wbc_gait_feedback.h"
#include "wbc_model.hpp"
#include "wbc_tick.hpp"
#include "wbc_plant.hpp"
#include "wbc_quad.hpp"
#include "wbc_plant_host.hpp"
#include "wbc_gait_handle.hpp"   // host only: the device of a gait handle, and whether feedback is set on it

namespace {

struct PlantArgs {
  int n, ld;
  double dt;
  double* q;
  double* v;
  double* time;
  const double* tau;
  const uint8_t* mask;
  const double* mu;
  const double* ms;
  double* vdot;
  double* force;
  int32_t* flags;
  int32_t* counts;
  double Kd, tau_max, mu0;
};

// Lambda^-1 assembly on every lane: lane c holds its row blocks blk[d] = Z_c' Z_d (+ G_c on the diagonal); block (c, d), d <= c,
// is broadcast from lane c into the packed lower triangle.
template <int C> __device__ __forceinline__ void gather_rows(const double (&blk)[4][9], const double* e, double* A, double* eall) {
#pragma unroll
  for (int d = 0; d <= C; d++)
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++)
        if (d < C || j <= i) A[wbc::sp(3 * C + i, 3 * d + j)] = wbc::qmove<wbc::qp_bcast<C>()>(blk[d][3 * i + j]);
#pragma unroll
  for (int i = 0; i < 3; i++) eall[3 * C + i] = wbc::qmove<wbc::qp_bcast<C>()>(e[i]);
}

template <bool STEP>
__device__ __forceinline__ void plant_body(const wbc::ModelC* __restrict__ mp, const PlantArgs& a) {
  using namespace wbc;
  const int t = blockIdx.x * QUAD_BLOCK + threadIdx.x;
  const int l = t & 3;
  const int r = t >> 2;
  const bool live = r < a.n;
  const int i = live ? r : a.n - 1;   // quads past the batch compute on its last robot and store nothing
  const size_t ld = (size_t)a.ld;
  const ModelC& m = *mp;
  // ---------------- every load first
  double qb[7], vb[6], th[3], qd[3], tq[3];
  int qrow[3];
#pragma unroll
  for (int k = 0; k < 7; k++) qb[k] = a.q[k * ld + i];
#pragma unroll
  for (int k = 0; k < 6; k++) vb[k] = a.v[k * ld + i];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    qrow[k] = m.q_perm[3 * l + k];
    th[k] = a.q[(7 + qrow[k]) * ld + i];
    qd[k] = a.v[(6 + qrow[k]) * ld + i];
    tq[k] = a.tau[m.act_inv[3 * l + k] * ld + i];
  }
  const unsigned mask = a.mask[i] & 15u;
  const double mu = a.mu ? a.mu[i] : a.mu0;
  const double s_p = a.ms ? a.ms[i] : 1.0;
  double t0 = 0.0;
  int cnt = 0;
  if (STEP && a.time) t0 = a.time[i];
  if (STEP && a.counts) cnt = a.counts[l * ld + i];
  // ---------------- input checks (own joint rows here, OR over the quad)
  int bits = 0;
  {
    bool nf = false, clip = false;
#pragma unroll
    for (int k = 0; k < 7; k++) nf |= not_finite(qb[k]);
#pragma unroll
    for (int k = 0; k < 6; k++) nf |= not_finite(vb[k]);
#pragma unroll
    for (int k = 0; k < 3; k++) {
      nf |= not_finite(th[k]) | not_finite(qd[k]) | not_finite(tq[k]);
      clip |= fabs(tq[k]) > a.tau_max * (1.0 + PLANT_CLIP_TOL);
    }
    nf |= !(mu > 0.0) | not_finite(mu) | !(s_p > 0.0) | not_finite(s_p);
    bits = qor((nf ? PLANT_BAD : 0) | (clip ? PLANT_CLIP : 0));
  }
  double tau_a[3];
#pragma unroll
  for (int k = 0; k < 3; k++) tau_a[k] = fmin(fmax(tq[k], -a.tau_max), a.tau_max);
  // ---------------- phase 1: own leg; base share replicated
  double R0[9];
  plant_rotation(qb, R0);
  const double w0[3] = {vb[0], vb[1], vb[2]}, v0[3] = {vb[3], vb[4], vb[5]};
  const bool stance = (mask >> l) & 1u;
  PlantLeg<double> L;
  plant_leg_phase1(m, l, R0, w0, v0, th, qd, tau_a, stance, a.Kd, L);
  double S[27];
  plant_base_share(m, R0, w0, s_p, S);
#pragma unroll
  for (int k = 0; k < 27; k++) S[k] = S[k] + qsum(L.s[k]);
  // ---------------- base solve: S = Lb Lb', a0_b = S^-1 rho
  double rinvb[6], pivb[6], a0b[6];
  plant_chol<double, 6>(S, rinvb, pivb);
#pragma unroll
  for (int k = 0; k < 6; k++) a0b[k] = S[21 + k];
  plant_fwd<double, 6>(S, rinvb, a0b);
  plant_bwd<double, 6>(S, rinvb, a0b);
  // ---------------- phase 2: own leg's Z, G, e; the contact system on every lane
  double Z[18], G[9], e[3], a0l[3];
  plant_leg_phase2(L, S, rinvb, a0b, stance, Z, G, e, a0l);
  double blk[4][9];
  {
    double Zd[18];
#pragma unroll
    for (int k = 0; k < 18; k++) Zd[k] = qmove<qp_bcast<0>()>(Z[k]);
    plant_lambda_block(Z, Zd, G, l == 0, blk[0]);
#pragma unroll
    for (int k = 0; k < 18; k++) Zd[k] = qmove<qp_bcast<1>()>(Z[k]);
    plant_lambda_block(Z, Zd, G, l == 1, blk[1]);
#pragma unroll
    for (int k = 0; k < 18; k++) Zd[k] = qmove<qp_bcast<2>()>(Z[k]);
    plant_lambda_block(Z, Zd, G, l == 2, blk[2]);
#pragma unroll
    for (int k = 0; k < 18; k++) Zd[k] = qmove<qp_bcast<3>()>(Z[k]);
    plant_lambda_block(Z, Zd, G, l == 3, blk[3]);
  }
  double A[78], eall[12], f[12];
  gather_rows<0>(blk, e, A, eall);
  gather_rows<1>(blk, e, A, eall);
  gather_rows<2>(blk, e, A, eall);
  gather_rows<3>(blk, e, A, eall);
  const bool pivots_ok = plant_contact_solve(A, eall, mask, f);
  // ---------------- accelerations: x_b = a0_b + Lb'^-1 sum_c Z_c f_c, then the own leg
  double fo[3];
#pragma unroll
  for (int k = 0; k < 3; k++) fo[k] = (l == 0) ? f[k] : (l == 1) ? f[3 + k] : (l == 2) ? f[6 + k] : f[9 + k];
  double vdb[6], vdl[3];
#pragma unroll
  for (int k = 0; k < 6; k++) vdb[k] = qsum(Z[3 * k] * fo[0] + Z[3 * k + 1] * fo[1] + Z[3 * k + 2] * fo[2]);
  plant_bwd<double, 6>(S, rinvb, vdb);
#pragma unroll
  for (int k = 0; k < 6; k++) vdb[k] = a0b[k] + vdb[k];
  plant_leg_final(L, vdb, fo, vdl);
  {
    bool nf = !pivots_ok;
#pragma unroll
    for (int k = 0; k < 6; k++) nf |= not_finite(vdb[k]);
#pragma unroll
    for (int k = 0; k < 3; k++) nf |= not_finite(vdl[k]) | not_finite(fo[k]);
    bits |= qor(nf ? PLANT_BAD : 0);
  }
  const bool bad = bits & PLANT_BAD;
  bits |= bad ? 0 : plant_force_flags(f, mask, mu, plant_weight(m, s_p));
#pragma unroll
  for (int k = 0; k < 6; k++) vdb[k] = bad ? 0.0 : vdb[k];
#pragma unroll
  for (int k = 0; k < 3; k++) { vdl[k] = bad ? 0.0 : vdl[k]; fo[k] = (bad || !stance) ? 0.0 : fo[k]; }
  // ---------------- integration (registers only)
  double qn[3], vn[3];
  if (STEP) {
    plant_integrate_base(a.dt, vdb, qb, vb);
#pragma unroll
    for (int k = 0; k < 3; k++) { qn[k] = th[k]; vn[k] = qd[k]; plant_integrate_joint(a.dt, vdl[k], qn[k], vn[k]); }
  }
  // ---------------- stores
  if (!live) return;
  if (l == 0 && a.flags) a.flags[i] = bits;
  if (a.vdot) {
    if (l == 0) {
#pragma unroll
      for (int k = 0; k < 6; k++) a.vdot[k * ld + i] = vdb[k];
    }
#pragma unroll
    for (int k = 0; k < 3; k++) a.vdot[(6 + qrow[k]) * ld + i] = vdl[k];
  }
  if (a.force) {
#pragma unroll
    for (int k = 0; k < 3; k++) a.force[(3 * l + k) * ld + i] = fo[k];
  }
  if (STEP) {
    if (!bad) {
      if (l == 0) {
#pragma unroll
        for (int k = 0; k < 6; k++) a.v[k * ld + i] = vb[k];
#pragma unroll
        for (int k = 0; k < 7; k++) a.q[k * ld + i] = qb[k];
      }
#pragma unroll
      for (int k = 0; k < 3; k++) { a.v[(6 + qrow[k]) * ld + i] = vn[k]; a.q[(7 + qrow[k]) * ld + i] = qn[k]; }
    }
    if (l == 0 && a.time) a.time[i] = t0 + a.dt;
    if (a.counts && ((bits >> l) & 1)) a.counts[l * ld + i] = cnt + 1;
  }
}

}  // namespace

// stable kernel names (rocprofv3 --kernel-trace)
__global__ void __launch_bounds__(wbc::QUAD_BLOCK) wbc_plant_step_kernel(const wbc::ModelC* __restrict__ m, PlantArgs a) {
  plant_body<true>(m, a);
}
__global__ void __launch_bounds__(wbc::QUAD_BLOCK) wbc_plant_forward_kernel(const wbc::ModelC* __restrict__ m, PlantArgs a) {
  plant_body<false>(m, a);
}

struct wbc_plant_s {
  int device;
  wbc_plant_params params;
  wbc::ModelC* d_model;
  wbc_gait gait;   // not null: wbc_plant_rollout takes its targets from it, not from the trajectory
};

namespace {

int check_plant_args(const char* fn, wbc_plant p, int n, int ld, const void* q, const void* v, const void* tau, const void* mask) {
  return wbc::plant_check_batch(fn, p, "plant", n, ld, q && v && tau && mask, "q, v, tau and contact_mask");
}

int launch_plant(wbc_plant p, hipStream_t s, bool step, const PlantArgs& a) {
  const dim3 grid = wbc::plant_grid(a.n), block(wbc::QUAD_BLOCK);
  if (step)
    hipLaunchKernelGGL(wbc_plant_step_kernel, grid, block, 0, s, p->d_model, a);
  else
    hipLaunchKernelGGL(wbc_plant_forward_kernel, grid, block, 0, s, p->d_model, a);
  HIP_TRY(hipGetLastError());
  return 0;
}

PlantArgs make_args(wbc_plant p, int n, int ld, double dt, double* q, double* v, double* time, const double* tau, const uint8_t* mask,
                    const double* mu, const double* ms, double* vdot, double* force, int32_t* flags, int32_t* counts) {
  PlantArgs a;
  a.n = n; a.ld = ld; a.dt = dt; a.q = q; a.v = v; a.time = time; a.tau = tau; a.mask = mask; a.mu = mu; a.ms = ms;
  a.vdot = vdot; a.force = force; a.flags = flags; a.counts = counts;
  a.Kd = p->params.Kd_contact; a.tau_max = p->params.tau_max; a.mu0 = p->params.mu;
  return a;
}

}  // namespace

extern "C" {

int wbc_plant_params_default(wbc_plant_params* out) {
  if (!out) return wbc::misuse("wbc_plant_params_default: null argument");
  out->Kd_contact = 100.0;
  out->tau_max = INFINITY;
  out->mu = 1.0;
  return 0;
}

int wbc_plant_create(const wbc_model* model, const wbc_plant_params* params, int device, wbc_plant* out) {
  if (!model || !out) return wbc::misuse("wbc_plant_create: null argument");
  wbc::ModelC m;
  int rc = wbc::model_checked("wbc_plant_create", model, &m);
  if (rc) return rc;
  wbc_plant_params P;
  wbc_plant_params_default(&P);
  if (params) P = *params;
  if (!(P.mu > 0) || !(P.tau_max > 0) || !(P.Kd_contact >= 0) || P.mu == INFINITY || P.Kd_contact == INFINITY)
    return wbc::misuse("wbc_plant_create: mu must be positive and finite, tau_max positive, Kd_contact non-negative and finite");
  wbc::ModelC* d = nullptr;
  rc = wbc::plant_model_upload(device, m, &d);
  if (rc) return rc;
  wbc_plant p = new wbc_plant_s();
  p->device = device;
  p->params = P;
  p->d_model = d;
  p->gait = nullptr;
  *out = p;
  return 0;
}

int wbc_plant_destroy(wbc_plant p) {
  if (!p) return 0;
  wbc::DeviceGuard device_guard_(p->device);
  (void)hipDeviceSynchronize();   // a launch still reading the model
  if (p->d_model) (void)hipFree(p->d_model);
  delete p;
  return 0;
}

int wbc_plant_forward(wbc_plant p, void* hip_stream, int n, int ld, const double* q, const double* v, const double* tau,
                      const uint8_t* contact_mask, const double* mu, const double* mass_scale, double* vdot, double* force,
                      int32_t* flags) {
  const int rc = check_plant_args("wbc_plant_forward", p, n, ld, q, v, tau, contact_mask);
  if (rc) return rc;
  if (n == 0) return 0;
  WBC_ON_DEVICE(p->device, wbc::fail);
  // the forward kernel never writes q or v
  return launch_plant(p, (hipStream_t)hip_stream, false,
                      make_args(p, n, ld, 0.0, const_cast<double*>(q), const_cast<double*>(v), nullptr, tau, contact_mask, mu,
                                mass_scale, vdot, force, flags, nullptr));
}

int wbc_plant_step(wbc_plant p, void* hip_stream, int n, int ld, double dt, double* q, double* v, double* time, const double* tau,
                   const uint8_t* contact_mask, const double* mu, const double* mass_scale, double* vdot, double* force,
                   int32_t* flags, int32_t* counts) {
  const int rc = check_plant_args("wbc_plant_step", p, n, ld, q, v, tau, contact_mask);
  if (rc) return rc;
  if (n == 0) return 0;
  WBC_ON_DEVICE(p->device, wbc::fail);
  return launch_plant(p, (hipStream_t)hip_stream, true,
                      make_args(p, n, ld, dt, q, v, time, tau, contact_mask, mu, mass_scale, vdot, force, flags, counts));
}

int wbc_plant_rollout(wbc_handle h, wbc_plant p, wbc_traj traj, void* hip_stream, int steps, double dt, int n, int ld, double* q,
                      double* v, double* time, double* targets, uint8_t* contact_mask, const double* mu, const double* mass_scale,
                      const double* plant_mu, const double* plant_mass_scale, double* tau, double* metrics, int32_t* status,
                      double* force, int32_t* flags, int32_t* counts) {
  const int rc = check_plant_args("wbc_plant_rollout", p, n, ld, q, v, tau, contact_mask);
  if (rc) return rc;
  if (!h || (!traj && !p->gait)) return wbc::misuse("wbc_plant_rollout: null controller or trajectory handle");
  if (steps < 0) return wbc::misuse("wbc_plant_rollout: steps must be >= 0");
  if (n > 0 && (!time || !targets)) return wbc::misuse("wbc_plant_rollout: time and targets are required");
  const PlantArgs a = make_args(p, n, ld, dt, q, v, time, tau, contact_mask, plant_mu, plant_mass_scale, nullptr, force, flags, counts);
  // the tick's targets: the gait's while one is set, else the lookup in `traj` -- the launch a rollout without a gait issues.  A
  // gait with feedback set (wbc_gait_feedback.h) reads the rollout's own q and v: one more launch per tick.
  const bool measured = p->gait && wbc::gait_feedback_on(*p->gait);
  auto source = [&](wbc_traj tr, void* s, int n_, int ld_, const double* t, double* tg, uint8_t* m) {
    if (measured) return wbc_gait_targets_measured(p->gait, s, n_, ld_, t, q, v, tg, m, nullptr);
    return p->gait ? wbc_gait_targets(p->gait, s, n_, ld_, t, tg, m) : wbc_traj_lookup(tr, s, n_, ld_, t, tg, m);
  };
  return wbc::plant_rollout("wbc_plant_rollout", h, traj, p->device, hip_stream, steps, n, ld, q, v, time, targets, contact_mask, mu,
                            mass_scale, tau, metrics, status, [&] { return launch_plant(p, (hipStream_t)hip_stream, true, a); },
                            wbc::NoRolloutHook(), source);
}

int wbc_plant_set_gait(wbc_plant p, wbc_gait gait) {
  if (!p) return wbc::misuse("wbc_plant_set_gait: null plant handle");
  if (gait && gait->device != p->device) return wbc::misuse("wbc_plant_set_gait: the gait handle lives on another device than the plant");
  p->gait = gait;
  return 0;
}

int wbc_plant_kernel_info(wbc_plant p, int* num_vgpr, int* scratch_bytes, int* lds_bytes, int* block_threads) {
  if (!p) return wbc::misuse("wbc_plant_kernel_info: null plant handle");
  return WBC_PLANT_KERNEL_INFO(p->device, wbc_plant_step_kernel, num_vgpr, scratch_bytes, lds_bytes, block_threads);
}

}  // extern "C"
