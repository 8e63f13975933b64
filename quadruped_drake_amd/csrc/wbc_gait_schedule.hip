// wbc_gait_schedule.hip -- the gait planner's command schedules (include/wbc_gait_schedule.h): kernels and C ABI.
//
// wbc_gait_schedule_resolve_kernel, one thread per robot, turns a robot's switches into its rows of the handle's buffer once per
// wbc_gait_set_schedule (wbc_gait.hpp: gait_schedule_resolve): per switch its Theta, S_j, c_j and the blend's three quintics.
// wbc_gait_schedule_targets_kernel and wbc_gait_schedule_terrain_targets_kernel are the mapping of wbc_gait.hip's two kernels -- a
// quad of lanes per robot, one foot per lane, the tables staged in LDS -- with the SCHEDULE instantiations of the law: every lane
// loads its robot's seven Thetas with its other inputs, and each of its three pose evaluations picks its segment by seven compares
// and reads that segment's rows of the buffer from global memory, seven for an arc and eighteen more inside a blend window.  The
// body's evaluation reads the same addresses on the four lanes of a quad, the footholds' neighbouring ones.  No private array is
// indexed by a run-time value: no scratch.
//
// This is a translation unit of its own so that the device code of wbc_gait.hip stays what it is: a handle without a schedule
// launches that file's kernels, and this file's are reached through gait_schedule_launch (wbc_gait_handle.hpp) only while a schedule
// is set.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/wbc.h"
#include "../../include/wbc_gait_schedule.h"
#include "wbc_gait.hpp"
#include "wbc_quad.hpp"
#include "wbc_plant_host.hpp"
#include "wbc_gait_handle.hpp"

namespace {

// dst[0 .. words) <- src[0 .. words) by the block's 64 lanes
__device__ __forceinline__ void stage(double* dst, const double* src, int words) {
#pragma unroll 8
  for (int k = threadIdx.x; k < words; k += wbc::QUAD_BLOCK) dst[k] = src[k];
}

// lane l's nine foot rows, and from lane 0 the body rows and the mask
__device__ __forceinline__ void store(const wbc::GaitArgs& a, size_t i, int l, const double* f, const double* b, unsigned mask) {
  const size_t ld = (size_t)a.ld;
  double* out = a.targets + i;
#pragma unroll
  for (int k = 0; k < 9; k++) out[(size_t)(18 + 9 * l + k) * ld] = f[k];
  if (l == 0) {
#pragma unroll
    for (int k = 0; k < 18; k++) out[(size_t)k * ld] = b[k];
    a.mask[i] = (uint8_t)mask;
  }
}

}  // namespace

// both target kernels take the launch, the handle's terrain and its schedule; this one, on the plane, does not read the terrain
__global__ void __launch_bounds__(wbc::QUAD_BLOCK) wbc_gait_schedule_targets_kernel(wbc::GaitArgs a, wbc::GaitTerrainArgs, wbc::GaitScheduleArgs sa) {
  using namespace wbc;
  __shared__ double lds[GAIT_TABLE_DOUBLES];
  stage(lds, a.table, GAIT_HEAD + a.count * GAIT_STRIDE);   // count <= WBC_GAIT_MAX_STRIDES: checked by wbc_gait_create
  const int t = blockIdx.x * QUAD_BLOCK + threadIdx.x;
  const int l = t & 3;
  const int r = t >> 2;
  const bool live = r < a.n;
  const size_t i = (size_t)(live ? r : a.n - 1);   // quads past the batch compute on its last robot and store nothing; a.n <= sa.n
  const GaitIn in = gait_load(a.time, a.cmd, a.gait_id, a.scale, a.start, (size_t)a.ld, i);
  const GaitSchedule S = gait_schedule_load(sa.knots, (size_t)sa.ld, i, sa.beta);
  __syncthreads();
  GaitClock c = gait_clock(lds, a.count, in);
  gait_clock_spoil(c, S.bad);
  double b[18], f[9];
  gait_foot<false, true>(lds, in, c, l, f, nullptr, nullptr, nullptr, nullptr, &S);
  gait_body<false, true>(lds, in, c, b, nullptr, nullptr, &S);
  if (live) store(a, i, l, f, b, c.mask);
}

__global__ void __launch_bounds__(wbc::QUAD_BLOCK) wbc_gait_schedule_terrain_targets_kernel(wbc::GaitArgs a, wbc::GaitTerrainArgs ta, wbc::GaitScheduleArgs sa) {
  using namespace wbc;
  __shared__ double lds[GAIT_TABLE_DOUBLES + GAIT_TERRAIN_DOUBLES];
  double* const ter = lds + GAIT_TABLE_DOUBLES;
  stage(lds, a.table, GAIT_HEAD + a.count * GAIT_STRIDE);                // count <= WBC_GAIT_MAX_STRIDES: checked by wbc_gait_create
  stage(ter, ta.table, GAIT_TERRAIN_HEAD + ta.count * TERRAIN_STRIDE);   // count <= TERRAIN_MAX_PROFILES: checked by wbc_gait_set_terrain
  const int t = blockIdx.x * QUAD_BLOCK + threadIdx.x;
  const int l = t & 3;
  const int r = t >> 2;
  const bool live = r < a.n;
  const size_t i = (size_t)(live ? r : a.n - 1);   // quads past the batch compute on its last robot and store nothing; a.n <= sa.n
  const GaitIn in = gait_load(a.time, a.cmd, a.gait_id, a.scale, a.start, (size_t)a.ld, i);
  const int tid = ta.id ? (int)ta.id[i] : 0;
  const double tsc = ta.scale ? ta.scale[i] : 1.0;
  const GaitSchedule S = gait_schedule_load(sa.knots, (size_t)sa.ld, i, sa.beta);
  __syncthreads();
  const GaitGround G = gait_ground(ter, ta.count, tid, tsc);
  GaitClock c = gait_clock(lds, a.count, in);
  gait_clock_spoil(c, G.bad | S.bad);
  double b[18], f[9], own[3], gr[12];
  gait_foot<true, true>(lds, in, c, l, f, nullptr, ter, &G, own, &S);
#pragma unroll
  for (int d = 0; d < 3; d++) {
    gr[d] = qmove<qp_bcast<0>()>(own[d]);
    gr[3 + d] = qmove<qp_bcast<1>()>(own[d]);
    gr[6 + d] = qmove<qp_bcast<2>()>(own[d]);
    gr[9 + d] = qmove<qp_bcast<3>()>(own[d]);
  }
  gait_body<true, true>(lds, in, c, b, ter, gr, &S);
  if (live) store(a, i, l, f, b, c.mask);
}

// knots [GAIT_SCHEDULE_ROWS][ld] <- the schedules of robots 0 .. n-1; cmd, start: wbc_gait_set_commands' (start may be null)
__global__ void __launch_bounds__(wbc::QUAD_BLOCK) wbc_gait_schedule_resolve_kernel(int n, int ld, double beta, const double* cmd, const double* start,
                                                                                     const uint8_t* nswitch, const double* when, const double* cmds,
                                                                                     double* knots) {
  using namespace wbc;
  const int r = blockIdx.x * QUAD_BLOCK + threadIdx.x;
  if (r >= n) return;
  const size_t i = (size_t)r, l = (size_t)ld;
  GaitIn in;
  in.time = 0.0; in.id = 0; in.s = 1.0;
  in.cx = cmd[i]; in.cy = cmd[l + i]; in.w = cmd[2 * l + i];
  in.x0 = start ? start[i] : 0.0; in.y0 = start ? start[l + i] : 0.0; in.psi0 = start ? start[2 * l + i] : 0.0;
  gait_schedule_resolve(in, beta, (int)nswitch[i], when + i, cmds + i, l, knots + i, l);
}

namespace wbc {

int gait_schedule_launch(const wbc_gait_s& g, void* hip_stream, const GaitArgs& a) {
  if (g.terrain.count > 0)
    hipLaunchKernelGGL(wbc_gait_schedule_terrain_targets_kernel, plant_grid(a.n), dim3(QUAD_BLOCK), 0, (hipStream_t)hip_stream, a, g.terrain, g.schedule);
  else
    hipLaunchKernelGGL(wbc_gait_schedule_targets_kernel, plant_grid(a.n), dim3(QUAD_BLOCK), 0, (hipStream_t)hip_stream, a, g.terrain, g.schedule);
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace wbc

extern "C" {

int wbc_gait_set_schedule(wbc_gait g, void* hip_stream, int n, int ld, double blend, const uint8_t* nswitch, const double* when,
                          const double* cmds) {
  static_assert(WBC_GAIT_MAX_SWITCHES == wbc::GAIT_MAX_SWITCHES, "the header's limit is the buffer's");
  if (!g) return wbc::misuse("wbc_gait_set_schedule: null gait handle");
  if (!nswitch || !when || !cmds) return wbc::misuse("wbc_gait_set_schedule: nswitch, when and cmds are required");
  if (!(blend >= 0.0) || wbc::not_finite(blend)) return wbc::misuse("wbc_gait_set_schedule: blend must be non-negative and finite");
  if (n < 1 || n > WBC_MAX_LD) return wbc::misuse("wbc_gait_set_schedule: n out of range (1 .. WBC_MAX_LD)");
  if (ld > WBC_MAX_LD) return wbc::misuse("wbc_gait_set_schedule: ld exceeds WBC_MAX_LD");
  if (ld < n) return wbc::misuse("wbc_gait_set_schedule: ld must be >= n");
  if (!g->cmd || !g->d_table) return wbc::misuse("wbc_gait_set_schedule: wbc_gait_set_commands has not been called on this handle");
  WBC_ON_DEVICE(g->device, wbc::fail);
  g->schedule = wbc::GaitScheduleArgs{};
  if (g->knots_capacity < ld) {
    HIP_TRY(hipDeviceSynchronize());   // a launch still reading the previous buffer
    if (g->d_knots) (void)hipFree(g->d_knots);
    g->d_knots = nullptr;
    g->knots_capacity = 0;
    HIP_TRY(hipMalloc(&g->d_knots, (size_t)wbc::GAIT_SCHEDULE_ROWS * (size_t)ld * sizeof(double)));
    g->knots_capacity = ld;
  }
  const unsigned blocks = (unsigned)((n + wbc::QUAD_BLOCK - 1) / wbc::QUAD_BLOCK);
  hipLaunchKernelGGL(wbc_gait_schedule_resolve_kernel, dim3(blocks), dim3(wbc::QUAD_BLOCK), 0, (hipStream_t)hip_stream, n, ld, blend, g->cmd,
                     g->start, nswitch, when, cmds, g->d_knots);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize((hipStream_t)hip_stream));   // the caller may free its arrays
  g->schedule.n = n; g->schedule.ld = ld; g->schedule.beta = blend; g->schedule.knots = g->d_knots;
  return 0;
}

int wbc_gait_clear_schedule(wbc_gait g) {
  if (!g) return wbc::misuse("wbc_gait_clear_schedule: null gait handle");
  g->schedule = wbc::GaitScheduleArgs{};   // the buffer stays for the next wbc_gait_set_schedule
  return 0;
}

int wbc_gait_schedule_kernel_info(wbc_gait g, int terrain, int* num_vgpr, int* scratch_bytes, int* lds_bytes, int* block_threads) {
  if (!g) return wbc::misuse("wbc_gait_schedule_kernel_info: null gait handle");
  if (terrain) return WBC_PLANT_KERNEL_INFO(g->device, wbc_gait_schedule_terrain_targets_kernel, num_vgpr, scratch_bytes, lds_bytes, block_threads);
  return WBC_PLANT_KERNEL_INFO(g->device, wbc_gait_schedule_targets_kernel, num_vgpr, scratch_bytes, lds_bytes, block_threads);
}

}  // extern "C"
