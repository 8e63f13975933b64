// wbc_ground.hip -- the compliant-ground plant (include/wbc_ground.h): kernel and C ABI.
//
// Mapping of wbc_plant.hip: a quad of lanes per robot, one lane per leg (16 robots per wavefront).  Each lane computes its own
// leg's kinematics, CRBA, RNEA, D^-1, ground force and joint accelerations (wbc_ground.hpp); the base Schur complement and the
// base right-hand side are summed over the quad with quad_perm DPP builtins; the 6x6 Cholesky solve and the base integration are
// replicated on the quad (the same instructions on the same bits: every lane holds the same base state).  The explicit substeps
// of a control period all run inside ONE launch: q and v are loaded once, live in registers over the substep loop (which is not
// unrolled) and are stored once; nothing goes to memory between substeps.  double throughout, SoA I/O with the batch index fastest.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/wbc.h"
#include "../../include/wbc_ground.h"
#include "../../include/wbc_gait.h"
#include "../../include/wbc_gait_feedback.h"
#include "wbc_model.hpp"
#include "wbc_tick.hpp"
#include "wbc_ground.hpp"
#include "wbc_ground_follow.hpp"
#include "wbc_quad.hpp"
#include "wbc_plant_host.hpp"
#include "wbc_gait_handle.hpp"   // host only: the device of a gait handle, and whether feedback is set on it

namespace {

struct GroundArgs {
  int n, ld, substeps;
  double dt, h;
  double* q;
  double* v;
  double* time;
  const double* tau;
  const double* mu;
  const double* ms;
  const double* wext;
  double* vdot;
  double* force;
  uint8_t* contact;
  int32_t* flags;
  int32_t* counts;
  double k, d, vs, radius, tau_max, mu0, fall_height;
};
// The terrain kernels' own argument: the packed table (wbc::terrain_pack, count x TERRAIN_STRIDE doubles, device memory) and the
// per-instance choice.  GroundArgs stays as the flat kernels take it.
struct TerrainArgs {
  const double* table;
  const uint8_t* id;
  const double* scale;
  int count;
};
constexpr int TERRAIN_LDS_DOUBLES = wbc::TERRAIN_MAX_PROFILES * wbc::TERRAIN_STRIDE;   // 5 KB

// One force evaluation at the state in registers: base accelerations (replicated), the own leg's joint accelerations and foot
// force.  Returns ground_foot_force's bits of the own foot.
template <bool TERRAIN>
__device__ __forceinline__ int ground_eval(const wbc::ModelC& m, int l, const wbc::GroundLaw<double>& law, double mu, double s_p,
                                           const double* we, const double* qb, const double* vb, const double* th, const double* qd,
                                           const double* tau_a, double* vdb, double* vdl, double* f, const double* tab, double tscale) {
  using namespace wbc;
  double R0[9];
  plant_rotation(qb, R0);
  const double w0[3] = {vb[0], vb[1], vb[2]}, v0[3] = {vb[3], vb[4], vb[5]};
  PlantLeg<double> L;
  const int fb = ground_leg_phase<TERRAIN>(m, l, R0, w0, v0, qb[6], th, qd, tau_a, law, mu, L, f, qb[4], qb[5], tab, tscale);
  double S[27];
  plant_base_share(m, R0, w0, s_p, S);
#pragma unroll
  for (int k = 0; k < 27; k++) S[k] = S[k] + qsum(L.s[k]);
#pragma unroll
  for (int k = 0; k < 6; k++) S[21 + k] = S[21 + k] + we[k];
  ground_base_solve(S, vdb);
  plant_leg_final(L, vdb, f, vdl);
  return fb;
}

// TERRAIN: `lds` is the block's TERRAIN_LDS_DOUBLES of LDS; the table is staged into it once, before anything else, and every foot
// of every substep reads its profile from there (a lane carries the address of its profile and its scale through the loop, no
// knot).  Without TERRAIN, ta and lds are not touched.
template <bool STEP, bool TERRAIN>
__device__ __forceinline__ void ground_body(const wbc::ModelC* __restrict__ mp, const GroundArgs& a, const TerrainArgs& ta, double* lds) {
  using namespace wbc;
  if (TERRAIN) {
    const int words = ta.count * TERRAIN_STRIDE;   // count <= TERRAIN_MAX_PROFILES: checked by wbc_ground_set_terrain
    for (int k = threadIdx.x; k < words; k += QUAD_BLOCK) lds[k] = ta.table[k];
    __syncthreads();
  }
  const int t = blockIdx.x * QUAD_BLOCK + threadIdx.x;
  const int l = t & 3;
  const int r = t >> 2;
  const bool live = r < a.n;
  const int i = live ? r : a.n - 1;   // quads past the batch compute on its last robot and store nothing
  const size_t ld = (size_t)a.ld;
  const ModelC& m = *mp;
  // ---------------- every load first
  double qb[7], vb[6], th[3], qd[3], tq[3], we[6];
  int qrow[3];
#pragma unroll
  for (int k = 0; k < 7; k++) qb[k] = a.q[k * ld + i];
#pragma unroll
  for (int k = 0; k < 6; k++) vb[k] = a.v[k * ld + i];
#pragma unroll
  for (int k = 0; k < 6; k++) we[k] = a.wext ? a.wext[k * ld + i] : 0.0;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    qrow[k] = m.q_perm[3 * l + k];
    th[k] = a.q[(7 + qrow[k]) * ld + i];
    qd[k] = a.v[(6 + qrow[k]) * ld + i];
    tq[k] = a.tau[m.act_inv[3 * l + k] * ld + i];
  }
  const double mu = a.mu ? a.mu[i] : a.mu0;
  const double s_p = a.ms ? a.ms[i] : 1.0;
  double t0 = 0.0;
  int cnt = 0;
  if (STEP && a.time) t0 = a.time[i];
  if (STEP && a.counts) cnt = a.counts[l * ld + i];
  // ---------------- input checks (own joint rows here, OR over the quad at the end)
  bool nf = false, clip = false;
#pragma unroll
  for (int k = 0; k < 7; k++) nf |= not_finite(qb[k]);
#pragma unroll
  for (int k = 0; k < 6; k++) nf |= not_finite(vb[k]) | not_finite(we[k]);
#pragma unroll
  for (int k = 0; k < 3; k++) {
    nf |= not_finite(th[k]) | not_finite(qd[k]) | not_finite(tq[k]);
    clip |= fabs(tq[k]) > a.tau_max * (1.0 + PLANT_CLIP_TOL);
  }
  nf |= !(mu > 0.0) | not_finite(mu) | !(s_p > 0.0) | not_finite(s_p);
  const double* tab = nullptr;
  double tscale = 1.0;
  if (TERRAIN) {
    const int id = ta.id ? (int)ta.id[i] : 0;
    tscale = ta.scale ? ta.scale[i] : 1.0;
    const bool tbad = (id >= ta.count) | not_finite(tscale);
    nf |= tbad;
    tab = lds + (tbad ? 0 : id) * TERRAIN_STRIDE;   // a bad instance computes on profile 0 and stores nothing of it
  }
  double tau_a[3];
#pragma unroll
  for (int k = 0; k < 3; k++) tau_a[k] = fmin(fmax(tq[k], -a.tau_max), a.tau_max);
  GroundLaw<double> law;
  law.k = a.k; law.d = a.d; law.vs = a.vs; law.radius = a.radius;
  // ---------------- the substeps (registers only)
  double vdb[6], vdl[3], f[3], fsum[3] = {0.0, 0.0, 0.0};
  int fb = 0, slip = 0;
  if (STEP) {
    const double h = a.h;
#pragma unroll 1
    for (int s = 0; s < a.substeps; s++) {
      fb = ground_eval<TERRAIN>(m, l, law, mu, s_p, we, qb, vb, th, qd, tau_a, vdb, vdl, f, tab, tscale);
      slip |= fb;
#pragma unroll
      for (int k = 0; k < 6; k++) nf |= not_finite(vdb[k]);
#pragma unroll
      for (int k = 0; k < 3; k++) { nf |= not_finite(vdl[k]) | not_finite(f[k]); fsum[k] += f[k]; }
      plant_integrate_base(h, vdb, qb, vb);
#pragma unroll
      for (int k = 0; k < 3; k++) plant_integrate_joint(h, vdl[k], th[k], qd[k]);
    }
    const double inv = 1.0 / (double)a.substeps;
#pragma unroll
    for (int k = 0; k < 3; k++) fsum[k] = fsum[k] * inv;
#pragma unroll
    for (int k = 0; k < 7; k++) nf |= not_finite(qb[k]);
  } else {
    fb = ground_eval<TERRAIN>(m, l, law, mu, s_p, we, qb, vb, th, qd, tau_a, vdb, vdl, f, tab, tscale);
    slip = fb;
#pragma unroll
    for (int k = 0; k < 6; k++) nf |= not_finite(vdb[k]);
#pragma unroll
    for (int k = 0; k < 3; k++) { nf |= not_finite(vdl[k]) | not_finite(f[k]); fsum[k] = f[k]; }
  }
  // ---------------- flags: one OR over the quad of [bad, clip, slip, touch bit of the own foot]
  const int mine = (nf ? 1 : 0) | (clip ? 2 : 0) | ((slip & GROUND_FOOT_SLIP) ? 4 : 0) | ((fb & GROUND_FOOT_TOUCH) ? (16 << l) : 0);
  const int all = qor(mine);
  const bool bad = all & 1;
  int bits = (bad ? GROUND_BAD : 0) | ((all & 2) ? GROUND_CLIP : 0);
  if (!bad) bits |= ((all & 4) ? GROUND_SLIP : 0) | (ground_fell<TERRAIN>(qb, a.fall_height, tab, tscale) ? GROUND_FELL : 0);
  // ---------------- stores.  The store addresses are formed afresh from an index the compiler cannot tie to the loads': otherwise
  // it keeps the ~20 row addresses of the loads alive over the substep loop, and they spill.
  if (!live) return;
  int is = i;
  if (STEP) asm volatile("" : "+v"(is));
  if (l == 0 && a.flags) a.flags[is] = bits;
  if (l == 0 && a.contact) a.contact[is] = bad ? (uint8_t)0 : (uint8_t)((all >> 4) & 15);
  if (!STEP && a.vdot) {
    if (l == 0) {
#pragma unroll
      for (int k = 0; k < 6; k++) a.vdot[k * ld + is] = bad ? 0.0 : vdb[k];
    }
#pragma unroll
    for (int k = 0; k < 3; k++) a.vdot[(6 + qrow[k]) * ld + is] = bad ? 0.0 : vdl[k];
  }
  if (a.force) {
#pragma unroll
    for (int k = 0; k < 3; k++) a.force[(3 * l + k) * ld + is] = bad ? 0.0 : fsum[k];
  }
  if (STEP) {
    if (!bad) {
      if (l == 0) {
#pragma unroll
        for (int k = 0; k < 6; k++) a.v[k * ld + is] = vb[k];
#pragma unroll
        for (int k = 0; k < 7; k++) a.q[k * ld + is] = qb[k];
      }
#pragma unroll
      for (int k = 0; k < 3; k++) { a.v[(6 + qrow[k]) * ld + is] = qd[k]; a.q[(7 + qrow[k]) * ld + is] = th[k]; }
    }
    if (l == 0 && a.time) a.time[is] = t0 + a.dt;
    if (a.counts && ((bits >> l) & 1)) a.counts[l * ld + is] = cnt + 1;
  }
}

}  // namespace

// stable kernel names (rocprofv3 --kernel-trace)
__global__ void __launch_bounds__(wbc::QUAD_BLOCK) wbc_ground_step_kernel(const wbc::ModelC* __restrict__ m, GroundArgs a) {
  ground_body<true, false>(m, a, TerrainArgs{}, nullptr);
}
__global__ void __launch_bounds__(wbc::QUAD_BLOCK) wbc_ground_forward_kernel(const wbc::ModelC* __restrict__ m, GroundArgs a) {
  ground_body<false, false>(m, a, TerrainArgs{}, nullptr);
}
__global__ void __launch_bounds__(wbc::QUAD_BLOCK) wbc_ground_terrain_step_kernel(const wbc::ModelC* __restrict__ m, GroundArgs a, TerrainArgs ta) {
  __shared__ double lds[TERRAIN_LDS_DOUBLES];
  ground_body<true, true>(m, a, ta, lds);
}
__global__ void __launch_bounds__(wbc::QUAD_BLOCK) wbc_ground_terrain_forward_kernel(const wbc::ModelC* __restrict__ m, GroundArgs a, TerrainArgs ta) {
  __shared__ double lds[TERRAIN_LDS_DOUBLES];
  ground_body<false, true>(m, a, ta, lds);
}

// Targets that follow the terrain (wbc_ground_follow.hpp): one thread per robot, in place on targets [54][ld], the instance's rows
// and its profile in registers before the first store.
__global__ void __launch_bounds__(wbc::QUAD_BLOCK) wbc_ground_follow_kernel(int n, int ld, int mode, double* targets, TerrainArgs ta) {
  const int i = blockIdx.x * wbc::QUAD_BLOCK + threadIdx.x;
  if (i >= n) return;
  wbc::follow_instance(mode, ta.table, ta.count, ta.id, ta.scale, targets, (size_t)ld, (size_t)i);
}

struct wbc_ground_s {
  int device;
  wbc_ground_params params;
  wbc::ModelC* d_model;
  double* d_terrain;           // the packed table, TERRAIN_LDS_DOUBLES doubles, allocated by the first wbc_ground_set_terrain
  TerrainArgs terrain;         // count == 0: no terrain
  int follow;                  // WBC_FOLLOW_*: what wbc_ground_rollout does to the targets between lookup and tick
  wbc_gait gait;               // not null: wbc_ground_rollout takes its targets from it, not from the trajectory
};

namespace {

int check_ground_args(const char* fn, wbc_ground g, int n, int ld, const void* q, const void* v, const void* tau) {
  return wbc::plant_check_batch(fn, g, "ground", n, ld, q && v && tau, "q, v and tau");
}

// the substeps of a period dt; < 0 with the message set when dt is not a positive finite time or needs more than 2^20 substeps
int substeps_for(const char* fn, wbc_ground g, double dt) {
  if (!(dt > 0.0) || dt == INFINITY) return wbc::misuse(fn, "dt must be positive and finite");
  const int s = wbc::ground_substeps(dt, g->params.max_substep);
  if (s <= 0) return wbc::misuse(fn, "dt / max_substep exceeds 2^20 substeps");
  return s;
}

int launch_ground(wbc_ground g, hipStream_t s, bool step, const GroundArgs& a) {
  const dim3 grid = wbc::plant_grid(a.n), block(wbc::QUAD_BLOCK);
  if (g->terrain.count > 0) {
    if (step)
      hipLaunchKernelGGL(wbc_ground_terrain_step_kernel, grid, block, 0, s, g->d_model, a, g->terrain);
    else
      hipLaunchKernelGGL(wbc_ground_terrain_forward_kernel, grid, block, 0, s, g->d_model, a, g->terrain);
  } else if (step)
    hipLaunchKernelGGL(wbc_ground_step_kernel, grid, block, 0, s, g->d_model, a);
  else
    hipLaunchKernelGGL(wbc_ground_forward_kernel, grid, block, 0, s, g->d_model, a);
  HIP_TRY(hipGetLastError());
  return 0;
}

GroundArgs make_args(wbc_ground g, int n, int ld, int substeps, double dt, double* q, double* v, double* time, const double* tau,
                     const double* mu, const double* ms, const double* wext, double* vdot, double* force, uint8_t* contact,
                     int32_t* flags, int32_t* counts) {
  GroundArgs a;
  a.n = n; a.ld = ld; a.substeps = substeps; a.dt = dt; a.h = dt / (double)substeps;
  a.q = q; a.v = v; a.time = time; a.tau = tau; a.mu = mu; a.ms = ms; a.wext = wext;
  a.vdot = vdot; a.force = force; a.contact = contact; a.flags = flags; a.counts = counts;
  const wbc_ground_params& P = g->params;
  a.k = P.stiffness; a.d = P.dissipation; a.vs = P.v_stiction; a.radius = P.foot_radius; a.tau_max = P.tau_max; a.mu0 = P.mu;
  a.fall_height = P.fall_height;
  return a;
}

// the follow kernel on targets [54][ld]; the caller has checked the arguments and that a terrain is set
int launch_follow(wbc_ground g, hipStream_t s, int n, int ld, int mode, double* targets) {
  hipLaunchKernelGGL(wbc_ground_follow_kernel, dim3((unsigned)((n + wbc::QUAD_BLOCK - 1) / wbc::QUAD_BLOCK)), dim3(wbc::QUAD_BLOCK), 0, s, n,
                     ld, mode, targets, g->terrain);
  HIP_TRY(hipGetLastError());
  return 0;
}

bool follow_mode_ok(int mode) { return mode == WBC_FOLLOW_OFF || mode == WBC_FOLLOW_LIFT || mode == WBC_FOLLOW_FIT; }

void default_params(const wbc::ModelC& m, wbc_ground_params* out) {
  wbc::ground_default_law(m, &out->stiffness, &out->dissipation);
  out->mu = 1.0;
  out->v_stiction = wbc::GROUND_V_STICTION;
  out->foot_radius = 0.0;
  out->tau_max = INFINITY;
  out->max_substep = wbc::GROUND_MAX_SUBSTEP;
  out->fall_height = 0.0;
}

}  // namespace

extern "C" {

int wbc_ground_params_default(const wbc_model* model, wbc_ground_params* out) {
  if (!model || !out) return wbc::misuse("wbc_ground_params_default: null argument");
  wbc::ModelC m;
  const int rc = wbc::model_axes("wbc_ground_params_default", model, &m);
  if (rc) return rc;
  default_params(m, out);
  return 0;
}

int wbc_ground_create(const wbc_model* model, const wbc_ground_params* params, int device, wbc_ground* out) {
  if (!model || !out) return wbc::misuse("wbc_ground_create: null argument");
  wbc::ModelC m;
  int rc = wbc::model_checked("wbc_ground_create", model, &m);
  if (rc) return rc;
  wbc_ground_params P;
  default_params(m, &P);
  if (params) P = *params;
  const bool fin = P.stiffness < INFINITY && P.dissipation < INFINITY && P.mu < INFINITY && P.v_stiction < INFINITY &&
                   fabs(P.foot_radius) < INFINITY && P.max_substep < INFINITY && fabs(P.fall_height) < INFINITY;
  if (!fin || !(P.stiffness > 0) || !(P.dissipation >= 0) || !(P.mu > 0) || !(P.v_stiction > 0) || !(P.tau_max > 0) || !(P.max_substep > 0))
    return wbc::misuse("wbc_ground_create: stiffness, mu, v_stiction, tau_max and max_substep must be positive, dissipation "
                             "non-negative, and all but tau_max finite");
  wbc::ModelC* d = nullptr;
  rc = wbc::plant_model_upload(device, m, &d);
  if (rc) return rc;
  wbc_ground g = new wbc_ground_s();
  g->device = device;
  g->params = P;
  g->d_model = d;
  g->d_terrain = nullptr;
  g->terrain = TerrainArgs{};
  g->follow = WBC_FOLLOW_OFF;
  g->gait = nullptr;
  *out = g;
  return 0;
}

int wbc_ground_destroy(wbc_ground g) {
  if (!g) return 0;
  wbc::DeviceGuard device_guard_(g->device);
  (void)hipDeviceSynchronize();   // a launch still reading the model
  if (g->d_model) (void)hipFree(g->d_model);
  if (g->d_terrain) (void)hipFree(g->d_terrain);
  delete g;
  return 0;
}

int wbc_ground_forward(wbc_ground g, void* hip_stream, int n, int ld, const double* q, const double* v, const double* tau,
                       const double* mu, const double* mass_scale, const double* ext_wrench, double* vdot, double* force,
                       uint8_t* contact, int32_t* flags) {
  const int rc = check_ground_args("wbc_ground_forward", g, n, ld, q, v, tau);
  if (rc) return rc;
  if (n == 0) return 0;
  WBC_ON_DEVICE(g->device, wbc::fail);
  // the forward kernel never writes q or v
  return launch_ground(g, (hipStream_t)hip_stream, false,
                       make_args(g, n, ld, 1, 0.0, const_cast<double*>(q), const_cast<double*>(v), nullptr, tau, mu, mass_scale,
                                 ext_wrench, vdot, force, contact, flags, nullptr));
}

int wbc_ground_step(wbc_ground g, void* hip_stream, int n, int ld, double dt, double* q, double* v, double* time, const double* tau,
                    const double* mu, const double* mass_scale, const double* ext_wrench, double* force, uint8_t* contact,
                    int32_t* flags, int32_t* counts) {
  const int rc = check_ground_args("wbc_ground_step", g, n, ld, q, v, tau);
  if (rc) return rc;
  const int sub = substeps_for("wbc_ground_step", g, dt);
  if (sub < 0) return sub;
  if (n == 0) return 0;
  WBC_ON_DEVICE(g->device, wbc::fail);
  return launch_ground(g, (hipStream_t)hip_stream, true,
                       make_args(g, n, ld, sub, dt, q, v, time, tau, mu, mass_scale, ext_wrench, nullptr, force, contact, flags, counts));
}

int wbc_ground_rollout(wbc_handle h, wbc_ground g, wbc_traj traj, void* hip_stream, int steps, double dt, int n, int ld, double* q,
                       double* v, double* time, double* targets, uint8_t* contact_mask, const double* mu, const double* mass_scale,
                       const double* ground_mu, const double* ground_mass_scale, const double* ext_wrench, double* tau,
                       double* metrics, int32_t* status, double* force, uint8_t* contact, int32_t* flags, int32_t* counts) {
  const int rc = check_ground_args("wbc_ground_rollout", g, n, ld, q, v, tau);
  if (rc) return rc;
  if (!h || (!traj && !g->gait)) return wbc::misuse("wbc_ground_rollout: null controller or trajectory handle");
  if (steps < 0) return wbc::misuse("wbc_ground_rollout: steps must be >= 0");
  if (n > 0 && (!time || !targets || !contact_mask)) return wbc::misuse("wbc_ground_rollout: time, targets and contact_mask are required");
  const int sub = substeps_for("wbc_ground_rollout", g, dt);
  if (sub < 0) return sub;
  const GroundArgs a = make_args(g, n, ld, sub, dt, q, v, time, tau, ground_mu, ground_mass_scale, ext_wrench, nullptr, force, contact,
                                 flags, counts);
  const bool follow = g->follow != WBC_FOLLOW_OFF && g->terrain.count > 0;   // otherwise: the launches of a rollout without it
  // the tick's targets: the gait's while one is set, else the lookup in `traj` -- the launch a rollout without a gait issues.  A
  // gait with feedback set (wbc_gait_feedback.h) reads the rollout's own q and v: one more launch per tick.
  const bool measured = g->gait && wbc::gait_feedback_on(*g->gait);
  auto source = [&](wbc_traj tr, void* s, int n_, int ld_, const double* t, double* tg, uint8_t* m) {
    if (measured) return wbc_gait_targets_measured(g->gait, s, n_, ld_, t, q, v, tg, m, nullptr);
    return g->gait ? wbc_gait_targets(g->gait, s, n_, ld_, t, tg, m) : wbc_traj_lookup(tr, s, n_, ld_, t, tg, m);
  };
  return wbc::plant_rollout("wbc_ground_rollout", h, traj, g->device, hip_stream, steps, n, ld, q, v, time, targets, contact_mask, mu,
                            mass_scale, tau, metrics, status, [&] { return launch_ground(g, (hipStream_t)hip_stream, true, a); },
                            [&] { return follow ? launch_follow(g, (hipStream_t)hip_stream, n, ld, g->follow, targets) : 0; }, source);
}

int wbc_ground_set_gait(wbc_ground g, wbc_gait gait) {
  if (!g) return wbc::misuse("wbc_ground_set_gait: null ground handle");
  if (gait && gait->device != g->device) return wbc::misuse("wbc_ground_set_gait: the gait handle lives on another device than the plant");
  g->gait = gait;
  return 0;
}

int wbc_ground_follow_targets(wbc_ground g, void* hip_stream, int n, int ld, int mode, double* targets) {
  const int rc = wbc::plant_check_batch("wbc_ground_follow_targets", g, "ground", n, ld, targets != nullptr, "targets");
  if (rc) return rc;
  if (ld < n) return wbc::misuse("wbc_ground_follow_targets", "ld must be >= n");
  if (!follow_mode_ok(mode)) return wbc::misuse("wbc_ground_follow_targets", "mode must be WBC_FOLLOW_OFF, WBC_FOLLOW_LIFT or WBC_FOLLOW_FIT");
  if (n == 0 || mode == WBC_FOLLOW_OFF || g->terrain.count == 0) return 0;
  WBC_ON_DEVICE(g->device, wbc::fail);
  return launch_follow(g, (hipStream_t)hip_stream, n, ld, mode, targets);
}

int wbc_ground_set_follow(wbc_ground g, int mode) {
  if (!g) return wbc::misuse("wbc_ground_set_follow: null ground handle");
  if (!follow_mode_ok(mode)) return wbc::misuse("wbc_ground_set_follow", "mode must be WBC_FOLLOW_OFF, WBC_FOLLOW_LIFT or WBC_FOLLOW_FIT");
  g->follow = mode;
  return 0;
}

int wbc_ground_follow_kernel_info(wbc_ground g, int* num_vgpr, int* scratch_bytes, int* lds_bytes, int* block_threads) {
  if (!g) return wbc::misuse("wbc_ground_follow_kernel_info: null ground handle");
  return WBC_PLANT_KERNEL_INFO(g->device, wbc_ground_follow_kernel, num_vgpr, scratch_bytes, lds_bytes, block_threads);
}

int wbc_ground_kernel_info(wbc_ground g, int* num_vgpr, int* scratch_bytes, int* lds_bytes, int* block_threads) {
  if (!g) return wbc::misuse("wbc_ground_kernel_info: null ground handle");
  return WBC_PLANT_KERNEL_INFO(g->device, wbc_ground_step_kernel, num_vgpr, scratch_bytes, lds_bytes, block_threads);
}

int wbc_terrain_check(const wbc_terrain_profile* profiles, int count) {
  char b[256];
  if (!profiles) return wbc::misuse("wbc_terrain_check: null profiles");
  if (count < 1 || count > WBC_GROUND_MAX_PROFILES) return wbc::misuse("wbc_terrain_check: count must be 1 .. WBC_GROUND_MAX_PROFILES (16)");
  for (int p = 0; p < count; p++) {
    const wbc_terrain_profile& t = profiles[p];
    const char* what = wbc::terrain_profile_error(t.nk, t.x0, t.y0, t.yaw, t.s, t.h);
    if (what) { snprintf(b, sizeof b, "wbc_terrain_check: profile %d: %s", p, what); return wbc::misuse(b); }
  }
  return 0;
}

int wbc_ground_set_terrain(wbc_ground g, const wbc_terrain_profile* profiles, int count, const uint8_t* terrain_id,
                           const double* terrain_scale) {
  if (!g) return wbc::misuse("wbc_ground_set_terrain: null ground handle");
  if (!profiles || count == 0) {
    g->terrain = TerrainArgs{};
    return 0;
  }
  const int rc = wbc_terrain_check(profiles, count);
  if (rc) return rc;
  static_assert(WBC_GROUND_MAX_PROFILES == wbc::TERRAIN_MAX_PROFILES, "the header's limit is the table's");
  double table[TERRAIN_LDS_DOUBLES];
  for (int p = 0; p < count; p++) {
    const wbc_terrain_profile& t = profiles[p];
    wbc::terrain_pack(t.nk, t.x0, t.y0, t.yaw, t.s, t.h, table + p * wbc::TERRAIN_STRIDE);
  }
  WBC_ON_DEVICE(g->device, wbc::fail);
  if (!g->d_terrain) HIP_TRY(hipMalloc(&g->d_terrain, sizeof table));
  HIP_TRY(hipDeviceSynchronize());   // a launch still reading the previous table
  g->terrain = TerrainArgs{};
  HIP_TRY(hipMemcpy(g->d_terrain, table, (size_t)count * wbc::TERRAIN_STRIDE * sizeof(double), hipMemcpyHostToDevice));
  g->terrain.table = g->d_terrain;
  g->terrain.id = terrain_id;
  g->terrain.scale = terrain_scale;
  g->terrain.count = count;
  return 0;
}

int wbc_ground_terrain_kernel_info(wbc_ground g, int* num_vgpr, int* scratch_bytes, int* lds_bytes, int* block_threads) {
  if (!g) return wbc::misuse("wbc_ground_terrain_kernel_info: null ground handle");
  return WBC_PLANT_KERNEL_INFO(g->device, wbc_ground_terrain_step_kernel, num_vgpr, scratch_bytes, lds_bytes, block_threads);
}

}  // extern "C"
