// wbc_gait.hip -- the gait planner (include/wbc_gait.h): kernel and C ABI.
//
// Mapping of the plant kernels (wbc_quad.hpp): a quad of lanes per robot, one foot per lane, 16 robots per wavefront.  Every lane
// loads its robot's nine inputs, the clock (stride, phase, mask) is replicated on the quad -- the same instructions on the same bits
// -- and each lane evaluates its own foot's two footholds and the body's pose: three pose evaluations, two sincos each, which is the
// kernel's latency chain.  Lane l stores its foot's nine rows; lane 0 also the 18 body rows and the mask.  The packed table
// (wbc_gait.hpp) is staged in LDS once per block; every load is issued before the first store; nothing is read twice.
//
// wbc_gait_terrain_targets_kernel (include/wbc_gait_terrain.h) is the same mapping with the TERRAIN instantiations of
// the law: the terrain table is staged in LDS beside the stride table, each lane puts its foot's two footholds on the terrain and
// raises its swing over the knots between them, and the ground height under each foot and its two rates go round the quad by
// wbc_quad.hpp's broadcasts for the body rows.  A handle with no terrain launches wbc_gait_targets_kernel, whose code is untouched.
//
// Command schedules (include/wbc_gait_schedule.h) live in wbc_gait_schedule.hip and the foot-placement feedback
// (include/wbc_gait_feedback.h) in wbc_gait_feedback.hip, kernels and entry points: translation units of their own, so that this
// one's device code stays what it was.  The three share the handle (wbc_gait_handle.hpp); wbc_gait_targets hands a launch over to the
// schedules' file while a schedule is set and knows nothing of the feedback.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/wbc.h"
#include "../../include/wbc_gait.h"
#include "../../include/wbc_gait_terrain.h"
#include "wbc_gait.hpp"
#include "wbc_gait_handle.hpp"
#include "wbc_quad.hpp"
#include "wbc_plant_host.hpp"

using wbc::GaitArgs;
using wbc::GaitTerrainArgs;

// stable kernel name (rocprofv3 --kernel-trace)
__global__ void __launch_bounds__(wbc::QUAD_BLOCK) wbc_gait_targets_kernel(GaitArgs a) {
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
  const GaitIn in = gait_load(a.time, a.cmd, a.gait_id, a.scale, a.start, ld, i);
  __syncthreads();
  const GaitClock c = gait_clock(lds, a.count, in);
  double b[18], f[9];
  gait_foot(lds, in, c, l, f);
  gait_body(lds, in, c, b);
  if (!live) return;
  double* out = a.targets + i;
#pragma unroll
  for (int k = 0; k < 9; k++) out[(size_t)(18 + 9 * l + k) * ld] = f[k];
  if (l == 0) {
#pragma unroll
    for (int k = 0; k < 18; k++) out[(size_t)k * ld] = b[k];
    a.mask[i] = (uint8_t)c.mask;
  }
}

// dst[0 .. words) <- src[0 .. words) by the block's 64 lanes, eight loads in flight per lane before the first of their stores: a
// loop of one load and one store per trip pays the memory latency once per trip, and this kernel stages three times the plain one's words
__device__ __forceinline__ void gait_stage(double* dst, const double* src, int words) {
  constexpr int DEPTH = 8;
  for (int base = threadIdx.x; base < words; base += DEPTH * wbc::QUAD_BLOCK) {
    double x[DEPTH];
#pragma unroll
    for (int r = 0; r < DEPTH; r++) {
      const int k = base + r * wbc::QUAD_BLOCK;
      x[r] = k < words ? src[k] : 0.0;
    }
#pragma unroll
    for (int r = 0; r < DEPTH; r++) {
      const int k = base + r * wbc::QUAD_BLOCK;
      if (k < words) dst[k] = x[r];
    }
  }
}

__global__ void __launch_bounds__(wbc::QUAD_BLOCK) wbc_gait_terrain_targets_kernel(GaitArgs a, GaitTerrainArgs ta) {
  using namespace wbc;
  __shared__ double lds[GAIT_TABLE_DOUBLES + GAIT_TERRAIN_DOUBLES];
  double* const ter = lds + GAIT_TABLE_DOUBLES;
  const int words = GAIT_HEAD + a.count * GAIT_STRIDE;                 // count <= WBC_GAIT_MAX_STRIDES: checked by wbc_gait_create
  const int twords = GAIT_TERRAIN_HEAD + ta.count * TERRAIN_STRIDE;   // count <= TERRAIN_MAX_PROFILES: checked by wbc_gait_set_terrain
  gait_stage(lds, a.table, words);
  gait_stage(ter, ta.table, twords);
  const int t = blockIdx.x * QUAD_BLOCK + threadIdx.x;
  const int l = t & 3;
  const int r = t >> 2;
  const bool live = r < a.n;
  const size_t i = (size_t)(live ? r : a.n - 1);   // quads past the batch compute on its last robot and store nothing
  const size_t ld = (size_t)a.ld;
  const GaitIn in = gait_load(a.time, a.cmd, a.gait_id, a.scale, a.start, ld, i);
  const int tid = ta.id ? (int)ta.id[i] : 0;
  const double tsc = ta.scale ? ta.scale[i] : 1.0;
  __syncthreads();
  const GaitGround G = gait_ground(ter, ta.count, tid, tsc);
  GaitClock c = gait_clock(lds, a.count, in);
  gait_clock_spoil(c, G.bad);
  double b[18], f[9], own[3], gr[12];
  gait_foot<true>(lds, in, c, l, f, nullptr, ter, &G, own);
#pragma unroll
  for (int d = 0; d < 3; d++) {
    gr[d] = qmove<qp_bcast<0>()>(own[d]);
    gr[3 + d] = qmove<qp_bcast<1>()>(own[d]);
    gr[6 + d] = qmove<qp_bcast<2>()>(own[d]);
    gr[9 + d] = qmove<qp_bcast<3>()>(own[d]);
  }
  gait_body<true>(lds, in, c, b, ter, gr);
  if (!live) return;
  double* out = a.targets + i;
#pragma unroll
  for (int k = 0; k < 9; k++) out[(size_t)(18 + 9 * l + k) * ld] = f[k];
  if (l == 0) {
#pragma unroll
    for (int k = 0; k < 18; k++) out[(size_t)k * ld] = b[k];
    a.mask[i] = (uint8_t)c.mask;
  }
}

extern "C" {

int wbc_gait_check(const wbc_gait_params* params, const wbc_gait_stride* strides, int count) {
  const char* what = wbc::gait_error(params, strides, count);
  return what ? wbc::misuse("wbc_gait_check", what) : 0;
}

int wbc_gait_create(const wbc_gait_params* params, const wbc_gait_stride* strides, int count, int device, wbc_gait* out) {
  static_assert(WBC_GAIT_MAX_PHASES == 8 && WBC_GAIT_MAX_STRIDES == 16, "the packed table's layout");
  if (!out) return wbc::misuse("wbc_gait_create: null argument");
  const char* what = wbc::gait_error(params, strides, count);
  if (what) return wbc::misuse("wbc_gait_create", what);
  if (device < 0) return wbc::misuse("wbc_gait_create: device must be >= 0");
  wbc_gait g = new wbc_gait_s();   // no commands, no terrain, no schedule, no feedback: all null and 0
  g->device = device;
  g->count = count;
  wbc::gait_pack(params, strides, count, g->table);
  *out = g;
  return 0;
}

int wbc_gait_destroy(wbc_gait g) {
  if (!g) return 0;
  if (g->d_table || g->d_terrain || g->d_knots || g->d_feedback) {
    wbc::DeviceGuard device_guard_(g->device);
    (void)hipDeviceSynchronize();   // a launch still reading the tables
    if (g->d_table) (void)hipFree(g->d_table);
    if (g->d_terrain) (void)hipFree(g->d_terrain);
    if (g->d_knots) (void)hipFree(g->d_knots);
    if (g->d_feedback) (void)hipFree(g->d_feedback);
  }
  delete g;
  return 0;
}

int wbc_gait_set_commands(wbc_gait g, const double* cmd, const uint8_t* gait_id, const double* stride_scale, const double* start) {
  if (!g) return wbc::misuse("wbc_gait_set_commands: null gait handle");
  if (!cmd) return wbc::misuse("wbc_gait_set_commands: cmd is required");
  if (!g->d_table) {
    WBC_ON_DEVICE(g->device, wbc::fail);
    const size_t bytes = (size_t)(wbc::GAIT_HEAD + g->count * wbc::GAIT_STRIDE) * sizeof(double);
    double* d = nullptr;
    HIP_TRY(hipMalloc(&d, bytes));
    const hipError_t e = hipMemcpy(d, g->table, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipFree(d);
      return wbc::fail("hipMemcpy(gait table)", e);
    }
    g->d_table = d;
  }
  g->cmd = cmd; g->gait_id = gait_id; g->scale = stride_scale; g->start = start;
  return 0;
}

int wbc_gait_targets(wbc_gait g, void* hip_stream, int n, int ld, const double* time, double* targets, uint8_t* contact_mask) {
  const int rc = wbc::plant_check_batch("wbc_gait_targets", g, "gait", n, ld, time && targets && contact_mask, "time, targets and contact_mask");
  if (rc) return rc;
  if (!g->cmd || !g->d_table) return wbc::misuse("wbc_gait_targets: wbc_gait_set_commands has not been called on this handle");
  if (wbc::gait_schedule_on(*g) && n > g->schedule.n)
    return wbc::misuse("wbc_gait_targets: n is larger than the n of the handle's wbc_gait_set_schedule");
  if (n == 0) return 0;
  WBC_ON_DEVICE(g->device, wbc::fail);
  GaitArgs a;
  a.n = n; a.ld = ld; a.count = g->count; a.table = g->d_table; a.time = time; a.cmd = g->cmd; a.gait_id = g->gait_id;
  a.scale = g->scale; a.start = g->start; a.targets = targets; a.mask = contact_mask;
  if (wbc::gait_schedule_on(*g)) return wbc::gait_schedule_launch(*g, hip_stream, a);
  if (g->terrain.count > 0)
    hipLaunchKernelGGL(wbc_gait_terrain_targets_kernel, wbc::plant_grid(n), dim3(wbc::QUAD_BLOCK), 0, (hipStream_t)hip_stream, a, g->terrain);
  else
    hipLaunchKernelGGL(wbc_gait_targets_kernel, wbc::plant_grid(n), dim3(wbc::QUAD_BLOCK), 0, (hipStream_t)hip_stream, a);
  HIP_TRY(hipGetLastError());
  return 0;
}

int wbc_gait_kernel_info(wbc_gait g, int* num_vgpr, int* scratch_bytes, int* lds_bytes, int* block_threads) {
  if (!g) return wbc::misuse("wbc_gait_kernel_info: null gait handle");
  return WBC_PLANT_KERNEL_INFO(g->device, wbc_gait_targets_kernel, num_vgpr, scratch_bytes, lds_bytes, block_threads);
}

int wbc_gait_terrain_check(const wbc_gait_terrain_params* params, const wbc_terrain_profile* profiles, int count) {
  const char* what = wbc::gait_terrain_error(params);
  if (what) return wbc::misuse("wbc_gait_terrain_check", what);
  return wbc_terrain_check(profiles, count);
}

int wbc_gait_set_terrain(wbc_gait g, const wbc_gait_terrain_params* params, const wbc_terrain_profile* profiles, int count,
                         const uint8_t* terrain_id, const double* terrain_scale) {
  if (!g) return wbc::misuse("wbc_gait_set_terrain: null gait handle");
  if (!profiles || count == 0) {
    g->terrain = GaitTerrainArgs{};
    return 0;
  }
  const char* what = wbc::gait_terrain_error(params);
  if (what) return wbc::misuse("wbc_gait_set_terrain", what);
  const int rc = wbc_terrain_check(profiles, count);
  if (rc) return rc;
  what = wbc::gait_terrain_fit_error(params, g->table);
  if (what) return wbc::misuse("wbc_gait_set_terrain", what);
  static_assert(WBC_GROUND_MAX_PROFILES == wbc::TERRAIN_MAX_PROFILES, "the header's limit is the table's");
  double table[wbc::GAIT_TERRAIN_DOUBLES];
  wbc::gait_terrain_pack(params, g->table, profiles, count, table);
  WBC_ON_DEVICE(g->device, wbc::fail);
  if (!g->d_terrain) HIP_TRY(hipMalloc(&g->d_terrain, sizeof table));
  HIP_TRY(hipDeviceSynchronize());   // a launch still reading the previous table
  g->terrain = GaitTerrainArgs{};
  HIP_TRY(hipMemcpy(g->d_terrain, table, (size_t)(wbc::GAIT_TERRAIN_HEAD + count * wbc::TERRAIN_STRIDE) * sizeof(double), hipMemcpyHostToDevice));
  g->terrain.table = g->d_terrain;
  g->terrain.id = terrain_id;
  g->terrain.scale = terrain_scale;
  g->terrain.count = count;
  return 0;
}

int wbc_gait_terrain_kernel_info(wbc_gait g, int* num_vgpr, int* scratch_bytes, int* lds_bytes, int* block_threads) {
  if (!g) return wbc::misuse("wbc_gait_terrain_kernel_info: null gait handle");
  return WBC_PLANT_KERNEL_INFO(g->device, wbc_gait_terrain_targets_kernel, num_vgpr, scratch_bytes, lds_bytes, block_threads);
}

}  // extern "C"
