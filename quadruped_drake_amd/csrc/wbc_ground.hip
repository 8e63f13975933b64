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
#include "wbc_model.hpp"
#include "wbc_tick.hpp"
#include "wbc_ground.hpp"
#include "wbc_device_guard.hpp"

extern "C" void wbc_set_error_(const char* msg);   // wbc_kernels.hip: the buffer wbc_last_error() returns

namespace {

int gfail(const char* what, hipError_t e) {
  char b[512];
  snprintf(b, sizeof b, "%s: %s", what, hipGetErrorString(e));
  wbc_set_error_(b);
  return -2;
}
int gmisuse(const char* what) { wbc_set_error_(what); return -1; }
#define GROUND_TRY(x)                               \
  do {                                              \
    hipError_t e_ = (x);                            \
    if (e_ != hipSuccess) return gfail(#x, e_);     \
  } while (0)

constexpr int GROUND_BLOCK = 64;   // one wavefront per workgroup: 16 robots

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

// quad_perm DPP move of a double: CTRL = p0 | p1 << 2 | p2 << 4 | p3 << 6 (lane j of the quad reads lane p_j)
template <int CTRL> __device__ __forceinline__ double qmove(double x) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), CTRL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), CTRL, 0xF, 0xF, false);
  return __hiloint2double(hi, lo);
}
template <int CTRL> __device__ __forceinline__ int qmove_i(int x) { return __builtin_amdgcn_update_dpp(0, x, CTRL, 0xF, 0xF, false); }
constexpr int QP_XOR1 = 0xB1, QP_XOR2 = 0x4E;                 // [1 0 3 2], [2 3 0 1]
// sum over the quad, the same bits on every lane: (x0 + x1) + (x2 + x3)
__device__ __forceinline__ double qsum(double x) {
  const double a = x + qmove<QP_XOR1>(x);
  return a + qmove<QP_XOR2>(a);
}
__device__ __forceinline__ int qor(int x) {
  const int a = x | qmove_i<QP_XOR1>(x);
  return a | qmove_i<QP_XOR2>(a);
}

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
    for (int k = threadIdx.x; k < words; k += GROUND_BLOCK) lds[k] = ta.table[k];
    __syncthreads();
  }
  const int t = blockIdx.x * GROUND_BLOCK + threadIdx.x;
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
__global__ void __launch_bounds__(GROUND_BLOCK) wbc_ground_step_kernel(const wbc::ModelC* __restrict__ m, GroundArgs a) {
  ground_body<true, false>(m, a, TerrainArgs{}, nullptr);
}
__global__ void __launch_bounds__(GROUND_BLOCK) wbc_ground_forward_kernel(const wbc::ModelC* __restrict__ m, GroundArgs a) {
  ground_body<false, false>(m, a, TerrainArgs{}, nullptr);
}
__global__ void __launch_bounds__(GROUND_BLOCK) wbc_ground_terrain_step_kernel(const wbc::ModelC* __restrict__ m, GroundArgs a, TerrainArgs ta) {
  __shared__ double lds[TERRAIN_LDS_DOUBLES];
  ground_body<true, true>(m, a, ta, lds);
}
__global__ void __launch_bounds__(GROUND_BLOCK) wbc_ground_terrain_forward_kernel(const wbc::ModelC* __restrict__ m, GroundArgs a, TerrainArgs ta) {
  __shared__ double lds[TERRAIN_LDS_DOUBLES];
  ground_body<false, true>(m, a, ta, lds);
}

struct wbc_ground_s {
  int device;
  wbc_ground_params params;
  wbc::ModelC* d_model;
  double* d_terrain;           // the packed table, TERRAIN_LDS_DOUBLES doubles, allocated by the first wbc_ground_set_terrain
  TerrainArgs terrain;         // count == 0: no terrain
};

namespace {

int check_ground_args(const char* fn, wbc_ground g, int n, int ld, const void* q, const void* v, const void* tau) {
  char b[256];
  if (n < 0 || n > WBC_MAX_LD) { snprintf(b, sizeof b, "%s: n out of range (0 .. WBC_MAX_LD)", fn); return gmisuse(b); }
  if (ld > WBC_MAX_LD) { snprintf(b, sizeof b, "%s: ld exceeds WBC_MAX_LD", fn); return gmisuse(b); }
  if (n > 0 && ld < n) { snprintf(b, sizeof b, "%s: ld must be >= n", fn); return gmisuse(b); }
  if (!g) { snprintf(b, sizeof b, "%s: null ground handle", fn); return gmisuse(b); }
  if (n > 0 && (!q || !v || !tau)) { snprintf(b, sizeof b, "%s: q, v and tau are required", fn); return gmisuse(b); }
  return 0;
}

// the substeps of a period dt; < 0 with the message set when dt is not a positive finite time or needs more than 2^20 substeps
int substeps_for(const char* fn, wbc_ground g, double dt) {
  char b[256];
  if (!(dt > 0.0) || dt == INFINITY) { snprintf(b, sizeof b, "%s: dt must be positive and finite", fn); return gmisuse(b); }
  const int s = wbc::ground_substeps(dt, g->params.max_substep);
  if (s <= 0) { snprintf(b, sizeof b, "%s: dt / max_substep exceeds 2^20 substeps", fn); return gmisuse(b); }
  return s;
}

int launch_ground(wbc_ground g, hipStream_t s, bool step, const GroundArgs& a) {
  const dim3 grid((unsigned)(((size_t)a.n * 4 + GROUND_BLOCK - 1) / GROUND_BLOCK));
  if (g->terrain.count > 0) {
    if (step)
      hipLaunchKernelGGL(wbc_ground_terrain_step_kernel, grid, dim3(GROUND_BLOCK), 0, s, g->d_model, a, g->terrain);
    else
      hipLaunchKernelGGL(wbc_ground_terrain_forward_kernel, grid, dim3(GROUND_BLOCK), 0, s, g->d_model, a, g->terrain);
  } else if (step)
    hipLaunchKernelGGL(wbc_ground_step_kernel, grid, dim3(GROUND_BLOCK), 0, s, g->d_model, a);
  else
    hipLaunchKernelGGL(wbc_ground_forward_kernel, grid, dim3(GROUND_BLOCK), 0, s, g->d_model, a);
  GROUND_TRY(hipGetLastError());
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

int model_of(const char* fn, const wbc_model* model, wbc::ModelC* m) {
  char b[384];
  if (wbc::model_from_flat(model->flat, m)) { snprintf(b, sizeof b, "%s: joint axes must be axis-aligned", fn); return gmisuse(b); }
  if (!wbc::model_axes_are_xyy(m)) {
    snprintf(b, sizeof b, "%s: unsupported kinematic tree -- legs with the abduction joint about +-x and the hip and knee joints "
                          "about +-y (Mini Cheetah, ANYmal)", fn);
    return gmisuse(b);
  }
  return 0;
}

}  // namespace

extern "C" {

int wbc_ground_params_default(const wbc_model* model, wbc_ground_params* out) {
  if (!model || !out) return gmisuse("wbc_ground_params_default: null argument");
  wbc::ModelC m;
  const int rc = model_of("wbc_ground_params_default", model, &m);
  if (rc) return rc;
  wbc::ground_default_law(m, &out->stiffness, &out->dissipation);
  out->mu = 1.0;
  out->v_stiction = wbc::GROUND_V_STICTION;
  out->foot_radius = 0.0;
  out->tau_max = INFINITY;
  out->max_substep = wbc::GROUND_MAX_SUBSTEP;
  out->fall_height = 0.0;
  return 0;
}

int wbc_ground_create(const wbc_model* model, const wbc_ground_params* params, int device, wbc_ground* out) {
  if (!model || !out) return gmisuse("wbc_ground_create: null argument");
  wbc::ModelC m;
  int rc = model_of("wbc_ground_create", model, &m);
  if (rc) return rc;
  bool seen_q[12] = {0}, seen_a[12] = {0};
  int qp[12], ap[12];
  for (int i = 0; i < 12; i++) {
    qp[i] = model->q_perm[i]; ap[i] = model->act_perm[i];
    if (qp[i] < 0 || qp[i] >= 12 || ap[i] < 0 || ap[i] >= 12 || seen_q[qp[i]] || seen_a[ap[i]])
      return gmisuse("wbc_ground_create: q_perm/act_perm must be permutations of 0..11");
    seen_q[qp[i]] = seen_a[ap[i]] = true;
  }
  wbc::model_set_perms(&m, qp, ap);
  wbc_ground_params P;
  wbc_ground_params_default(model, &P);
  if (params) P = *params;
  const bool fin = P.stiffness < INFINITY && P.dissipation < INFINITY && P.mu < INFINITY && P.v_stiction < INFINITY &&
                   fabs(P.foot_radius) < INFINITY && P.max_substep < INFINITY && fabs(P.fall_height) < INFINITY;
  if (!fin || !(P.stiffness > 0) || !(P.dissipation >= 0) || !(P.mu > 0) || !(P.v_stiction > 0) || !(P.tau_max > 0) || !(P.max_substep > 0))
    return gmisuse("wbc_ground_create: stiffness, mu, v_stiction, tau_max and max_substep must be positive, dissipation non-negative, "
                   "and all but tau_max finite");
  WBC_ON_DEVICE(device, gfail);
  wbc::ModelC* d = nullptr;
  GROUND_TRY(hipMalloc(&d, sizeof m));
  const hipError_t e = hipMemcpy(d, &m, sizeof m, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(d);
    return gfail("hipMemcpy(model)", e);
  }
  wbc_ground g = new wbc_ground_s();
  g->device = device;
  g->params = P;
  g->d_model = d;
  g->d_terrain = nullptr;
  g->terrain = TerrainArgs{};
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
  WBC_ON_DEVICE(g->device, gfail);
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
  WBC_ON_DEVICE(g->device, gfail);
  return launch_ground(g, (hipStream_t)hip_stream, true,
                       make_args(g, n, ld, sub, dt, q, v, time, tau, mu, mass_scale, ext_wrench, nullptr, force, contact, flags, counts));
}

int wbc_ground_rollout(wbc_handle h, wbc_ground g, wbc_traj traj, void* hip_stream, int steps, double dt, int n, int ld, double* q,
                       double* v, double* time, double* targets, uint8_t* contact_mask, const double* mu, const double* mass_scale,
                       const double* ground_mu, const double* ground_mass_scale, const double* ext_wrench, double* tau,
                       double* metrics, int32_t* status, double* force, uint8_t* contact, int32_t* flags, int32_t* counts) {
  int rc = check_ground_args("wbc_ground_rollout", g, n, ld, q, v, tau);
  if (rc) return rc;
  if (!h || !traj) return gmisuse("wbc_ground_rollout: null controller or trajectory handle");
  if (steps < 0) return gmisuse("wbc_ground_rollout: steps must be >= 0");
  if (n > 0 && (!time || !targets || !contact_mask)) return gmisuse("wbc_ground_rollout: time, targets and contact_mask are required");
  const int sub = substeps_for("wbc_ground_rollout", g, dt);
  if (sub < 0) return sub;
  // a host-pointer handle is refused by wbc_integrate before anything is launched (n = 0: an argument check only)
  if (wbc_integrate(h, 0, 0, 0.0, nullptr, nullptr, nullptr)) return gmisuse("wbc_ground_rollout: needs a WBC_DEVICE_PTRS controller handle");
  if (steps == 0 || n == 0) return 0;
  rc = wbc_set_stream(h, hip_stream);
  if (rc) return rc;
  WBC_ON_DEVICE(g->device, gfail);
  const GroundArgs a = make_args(g, n, ld, sub, dt, q, v, time, tau, ground_mu, ground_mass_scale, ext_wrench, nullptr, force, contact,
                                 flags, counts);
  for (int s = 0; s < steps; s++) {
    rc = wbc_traj_lookup(traj, hip_stream, n, ld, time, targets, contact_mask);
    if (rc) return rc;
    rc = wbc_step(h, n, ld, q, v, targets, contact_mask, mu, mass_scale, tau, metrics, status);
    if (rc) return rc;
    rc = launch_ground(g, (hipStream_t)hip_stream, true, a);
    if (rc) return rc;
  }
  return 0;
}

int wbc_ground_kernel_info(wbc_ground g, int* num_vgpr, int* scratch_bytes, int* lds_bytes, int* block_threads) {
  if (!g) return gmisuse("wbc_ground_kernel_info: null ground handle");
  WBC_ON_DEVICE(g->device, gfail);
  hipFuncAttributes fa;
  GROUND_TRY(hipFuncGetAttributes(&fa, (const void*)wbc_ground_step_kernel));
  if (num_vgpr) *num_vgpr = fa.numRegs;
  if (scratch_bytes) *scratch_bytes = (int)fa.localSizeBytes;
  if (lds_bytes) *lds_bytes = (int)fa.sharedSizeBytes;
  if (block_threads) *block_threads = GROUND_BLOCK;
  return 0;
}

int wbc_terrain_check(const wbc_terrain_profile* profiles, int count) {
  char b[256];
  if (!profiles) return gmisuse("wbc_terrain_check: null profiles");
  if (count < 1 || count > WBC_GROUND_MAX_PROFILES) return gmisuse("wbc_terrain_check: count must be 1 .. WBC_GROUND_MAX_PROFILES (16)");
  for (int p = 0; p < count; p++) {
    const wbc_terrain_profile& t = profiles[p];
    const char* what = wbc::terrain_profile_error(t.nk, t.x0, t.y0, t.yaw, t.s, t.h);
    if (what) { snprintf(b, sizeof b, "wbc_terrain_check: profile %d: %s", p, what); return gmisuse(b); }
  }
  return 0;
}

int wbc_ground_set_terrain(wbc_ground g, const wbc_terrain_profile* profiles, int count, const uint8_t* terrain_id,
                           const double* terrain_scale) {
  if (!g) return gmisuse("wbc_ground_set_terrain: null ground handle");
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
  WBC_ON_DEVICE(g->device, gfail);
  if (!g->d_terrain) GROUND_TRY(hipMalloc(&g->d_terrain, sizeof table));
  GROUND_TRY(hipDeviceSynchronize());   // a launch still reading the previous table
  g->terrain = TerrainArgs{};
  GROUND_TRY(hipMemcpy(g->d_terrain, table, (size_t)count * wbc::TERRAIN_STRIDE * sizeof(double), hipMemcpyHostToDevice));
  g->terrain.table = g->d_terrain;
  g->terrain.id = terrain_id;
  g->terrain.scale = terrain_scale;
  g->terrain.count = count;
  return 0;
}

int wbc_ground_terrain_kernel_info(wbc_ground g, int* num_vgpr, int* scratch_bytes, int* lds_bytes, int* block_threads) {
  if (!g) return gmisuse("wbc_ground_terrain_kernel_info: null ground handle");
  WBC_ON_DEVICE(g->device, gfail);
  hipFuncAttributes fa;
  GROUND_TRY(hipFuncGetAttributes(&fa, (const void*)wbc_ground_terrain_step_kernel));
  if (num_vgpr) *num_vgpr = fa.numRegs;
  if (scratch_bytes) *scratch_bytes = (int)fa.localSizeBytes;
  if (lds_bytes) *lds_bytes = (int)fa.sharedSizeBytes;
  if (block_threads) *block_threads = GROUND_BLOCK;
  return 0;
}

}  // extern "C"
