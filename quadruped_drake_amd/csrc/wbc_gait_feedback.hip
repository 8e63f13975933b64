// wbc_gait_feedback.hip -- the gait planner's foot-placement feedback (include/wbc_gait_feedback.h): kernel and C ABI.
//
// wbc_gait_feedback_kernel runs after whichever gait kernel wrote the targets, on the same stream, in the gait's mapping: a quad of
// lanes per robot, one foot per lane, 16 robots per wavefront, the packed stride table staged in LDS.  Every lane loads its foot's
// nine rows, its six state words (lane t reads word t of each state row: contiguous), and the robot's eight trunk numbers, time, mask
// and previous mask -- the same addresses on the four lanes of a quad, one request each, which the ISA shows cheaper than a load on
// one lane and two DPP moves per word.  The 18 body rows are only looked at for a NaN: lane l takes rows l, l + 4, .. and the verdict
// goes round the quad by one OR.  Every load is issued before the first store.  The clock is replicated on the quad as in
// wbc_gait_targets_kernel.  No private array is indexed by a run-time value: no scratch.
//
// A translation unit of its own, like the schedules': the device code of wbc_gait.hip and wbc_gait_schedule.hip stays what it is.
// The state lives in the gait handle (wbc_gait_handle.hpp).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/wbc.h"
#include "../../include/wbc_gait_feedback.h"
#include "wbc_gait_feedback.hpp"
#include "wbc_gait_handle.hpp"
#include "wbc_quad.hpp"
#include "wbc_plant_host.hpp"

namespace {

struct FeedbackArgs {
  int n, ld, count;
  size_t row;            // doubles per state row: 4 x the instances of wbc_gait_set_feedback
  const double* table;   // GAIT_HEAD + count * GAIT_STRIDE doubles
  const double* time;
  const uint8_t* gait_id;
  const double* scale;
  const double* q;
  const double* v;
  double* targets;
  const uint8_t* mask;
  double* offsets;       // may be null
  double* state;
  uint8_t* prev;
  wbc_gait_feedback_params par;
};

}  // namespace

// stable kernel name (rocprofv3 --kernel-trace)
__global__ void __launch_bounds__(wbc::QUAD_BLOCK) wbc_gait_feedback_kernel(FeedbackArgs a) {
  using namespace wbc;
  __shared__ double lds[GAIT_TABLE_DOUBLES];
  const int words = GAIT_HEAD + a.count * GAIT_STRIDE;   // count <= WBC_GAIT_MAX_STRIDES: checked by wbc_gait_create
  for (int k = threadIdx.x; k < words; k += QUAD_BLOCK) lds[k] = a.table[k];
  const int t = blockIdx.x * QUAD_BLOCK + threadIdx.x;
  const int l = t & 3;
  const int r = t >> 2;
  const bool live = r < a.n;
  const size_t i = (size_t)(live ? r : a.n - 1);   // quads past the batch compute on its last robot and store nothing
  const size_t ld = (size_t)a.ld;
  const size_t w = 4 * i + (size_t)l;              // the lane's word of a state row; i < n <= row / 4
  const double time = a.time[i];
  const int id = a.gait_id ? (int)a.gait_id[i] : 0;
  const double s = a.scale ? a.scale[i] : 1.0;
  double* const out = a.targets + i;
  const double px = out[0], py = out[ld], pdx = out[3 * ld], pdy = out[4 * ld];
  const double qx = a.q[4 * ld + i], qy = a.q[5 * ld + i], vx = a.v[3 * ld + i], vy = a.v[4 * ld + i];
  double f[9], body[5];
#pragma unroll
  for (int k = 0; k < 9; k++) f[k] = out[(size_t)(18 + 9 * l + k) * ld];
#pragma unroll
  for (int j = 0; j < 5; j++) {
    const int k = l + 4 * j;
    body[j] = out[(size_t)(k < 18 ? k : 17) * ld];   // rows l, l + 4, .. of the 18; past them row 17 again
  }
  const unsigned mask = a.mask[i], was = a.prev[i];
  double cur[2], from[2], to[2];
#pragma unroll
  for (int k = 0; k < 2; k++) {
    cur[k] = a.state[(size_t)k * a.row + w];
    from[k] = a.state[(size_t)(2 + k) * a.row + w];
    to[k] = a.state[(size_t)(4 + k) * a.row + w];
  }
  __syncthreads();
  const GaitClock c = gait_feedback_clock(lds, a.count, time, id, s);
  double dx, dy, add[6];
  bool bad = !gait_feedback_offset(a.par, qx, qy, vx, vy, px, py, pdx, pdy, dx, dy) | not_finite(time);
#pragma unroll
  for (int k = 0; k < 9; k++) bad |= not_finite(f[k]);
#pragma unroll
  for (int j = 0; j < 5; j++) bad |= not_finite(body[j]);
  bad = qor(bad ? 1 : 0) != 0;
  gait_feedback_foot(a.par, c, l, (mask >> l) & 1u, (was >> l) & 1u, dx, dy, cur, from, to, add);
  if (!live) return;
  if (!bad) {
    double* const o = out + (size_t)(18 + 9 * l) * ld;
#pragma unroll
    for (int k = 0; k < 2; k++) {
      o[(size_t)k * ld] = f[k] + add[k];
      o[(size_t)(3 + k) * ld] = f[3 + k] + add[2 + k];
      o[(size_t)(6 + k) * ld] = f[6 + k] + add[4 + k];
      a.state[(size_t)k * a.row + w] = cur[k];
      a.state[(size_t)(2 + k) * a.row + w] = from[k];
      a.state[(size_t)(4 + k) * a.row + w] = to[k];
    }
    if (l == 0) a.prev[i] = (uint8_t)mask;
  }
  if (a.offsets) {
    const double nan = __builtin_nan("");
    a.offsets[(size_t)(2 * l) * ld + i] = bad ? nan : add[0];
    a.offsets[(size_t)(2 * l + 1) * ld + i] = bad ? nan : add[1];
  }
}

namespace {

size_t state_doubles(int n) { return (size_t)wbc::GAIT_FEEDBACK_ROWS * 4 * (size_t)n; }

}  // namespace

extern "C" {

int wbc_gait_feedback_check(const wbc_gait_feedback_params* params) {
  const char* what = wbc::gait_feedback_error(params);
  return what ? wbc::misuse("wbc_gait_feedback_check", what) : 0;
}

int wbc_gait_feedback_params_default(const wbc_gait_params* gait_params, wbc_gait_feedback_params* out) {
  if (!gait_params || !out) return wbc::misuse("wbc_gait_feedback_params_default: null argument");
  if (!(gait_params->height > 0.0) || wbc::not_finite(gait_params->height))
    return wbc::misuse("wbc_gait_feedback_params_default: the gait's height must be positive and finite");
  out->k_v = sqrt(gait_params->height / 9.81);
  out->k_p = 0.0;
  out->d_max = 0.10;
  out->u_hold = 0.5;
  return 0;
}

int wbc_gait_set_feedback(wbc_gait g, const wbc_gait_feedback_params* params, int n) {
  if (!g) return wbc::misuse("wbc_gait_set_feedback: null gait handle");
  const char* what = wbc::gait_feedback_error(params);
  if (what) return wbc::misuse("wbc_gait_set_feedback", what);
  if (n < 1 || n > WBC_MAX_LD) return wbc::misuse("wbc_gait_set_feedback: n out of range (1 .. WBC_MAX_LD)");
  WBC_ON_DEVICE(g->device, wbc::fail);
  HIP_TRY(hipDeviceSynchronize());   // a launch still working on the state
  const int had = g->feedback_n;
  g->feedback_n = 0;
  if (g->d_feedback && had != n) {
    (void)hipFree(g->d_feedback);
    g->d_feedback = nullptr;
  }
  const size_t bytes = state_doubles(n) * sizeof(double);
  if (!g->d_feedback) HIP_TRY(hipMalloc(&g->d_feedback, bytes + (size_t)n));
  HIP_TRY(hipMemset(g->d_feedback, 0, bytes));
  HIP_TRY(hipMemset(g->d_feedback + state_doubles(n), 0x0F, (size_t)n));
  HIP_TRY(hipDeviceSynchronize());
  g->feedback = *params;
  g->feedback_n = n;
  return 0;
}

int wbc_gait_clear_feedback(wbc_gait g) {
  if (!g) return wbc::misuse("wbc_gait_clear_feedback: null gait handle");
  g->feedback_n = 0;
  if (!g->d_feedback) return 0;
  WBC_ON_DEVICE(g->device, wbc::fail);
  (void)hipDeviceSynchronize();   // a launch still working on the state
  (void)hipFree(g->d_feedback);
  g->d_feedback = nullptr;
  return 0;
}

int wbc_gait_targets_measured(wbc_gait g, void* hip_stream, int n, int ld, const double* time, const double* q, const double* v,
                              double* targets, uint8_t* contact_mask, double* offsets) {
  const int rc = wbc::plant_check_batch("wbc_gait_targets_measured", g, "gait", n, ld, time && q && v && targets && contact_mask,
                                        "time, q, v, targets and contact_mask");
  if (rc) return rc;
  if (!g->cmd || !g->d_table) return wbc::misuse("wbc_gait_targets_measured: wbc_gait_set_commands has not been called on this handle");
  if (g->terrain.count > 0)
    return wbc::misuse("wbc_gait_targets_measured: the handle has a terrain set: the feedback knows no terrain (wbc_gait_feedback.h, limits)");
  if (!wbc::gait_feedback_on(*g)) return wbc::misuse("wbc_gait_targets_measured: wbc_gait_set_feedback has not been called on this handle");
  if (n > g->feedback_n) return wbc::misuse("wbc_gait_targets_measured: n is larger than the n of the handle's wbc_gait_set_feedback");
  const int rg = wbc_gait_targets(g, hip_stream, n, ld, time, targets, contact_mask);
  if (rg || n == 0) return rg;
  WBC_ON_DEVICE(g->device, wbc::fail);
  FeedbackArgs a;
  a.n = n; a.ld = ld; a.count = g->count; a.row = 4 * (size_t)g->feedback_n; a.table = g->d_table; a.time = time; a.gait_id = g->gait_id;
  a.scale = g->scale; a.q = q; a.v = v; a.targets = targets; a.mask = contact_mask; a.offsets = offsets; a.state = g->d_feedback;
  a.prev = (uint8_t*)(g->d_feedback + state_doubles(g->feedback_n)); a.par = g->feedback;
  hipLaunchKernelGGL(wbc_gait_feedback_kernel, wbc::plant_grid(n), dim3(wbc::QUAD_BLOCK), 0, (hipStream_t)hip_stream, a);
  HIP_TRY(hipGetLastError());
  return 0;
}

int wbc_gait_feedback_kernel_info(wbc_gait g, int* num_vgpr, int* scratch_bytes, int* lds_bytes, int* block_threads) {
  if (!g) return wbc::misuse("wbc_gait_feedback_kernel_info: null gait handle");
  return WBC_PLANT_KERNEL_INFO(g->device, wbc_gait_feedback_kernel, num_vgpr, scratch_bytes, lds_bytes, block_threads);
}

// internal (not in the header; the tests' read-back): the state of instances 0 .. n-1 to host memory, state [6][4 n] in the layout of
// wbc_gait_feedback.hpp with n as its capacity, prev [n].  Synchronises the device.
int wbc_gait_feedback_state_(wbc_gait g, int n, double* state, uint8_t* prev) {
  if (!g || !state || !prev) return wbc::misuse("wbc_gait_feedback_state_: null argument");
  const int cap = g->feedback_n;
  if (!wbc::gait_feedback_on(*g) || n < 1 || n > cap) return wbc::misuse("wbc_gait_feedback_state_: no feedback set, or n out of range");
  WBC_ON_DEVICE(g->device, wbc::fail);
  HIP_TRY(hipDeviceSynchronize());
  for (int r = 0; r < wbc::GAIT_FEEDBACK_ROWS; r++)
    HIP_TRY(hipMemcpy(state + (size_t)r * 4 * n, g->d_feedback + (size_t)r * 4 * cap, (size_t)4 * n * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(prev, g->d_feedback + state_doubles(cap), (size_t)n, hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"
