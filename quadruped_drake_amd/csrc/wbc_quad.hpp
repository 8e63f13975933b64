// wbc_quad.hpp -- the quad-of-lanes mapping the plant kernels share (wbc_plant.hip, wbc_ground.hip): a quad of lanes per robot,
// one lane per leg, and the cross-lane moves inside a quad.  The moves are quad_perm DPP builtins, so the compiler's hazard
// recogniser sees every one of them.
#pragma once
#include <hip/hip_runtime.h>

namespace wbc {

constexpr int QUAD_BLOCK = 64;   // one wavefront per workgroup: 16 robots

// quad_perm DPP move of a double: CTRL = p0 | p1 << 2 | p2 << 4 | p3 << 6 (lane j of the quad reads lane p_j)
template <int CTRL> __device__ __forceinline__ double qmove(double x) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), CTRL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), CTRL, 0xF, 0xF, false);
  return __hiloint2double(hi, lo);
}
template <int CTRL> __device__ __forceinline__ int qmove_i(int x) { return __builtin_amdgcn_update_dpp(0, x, CTRL, 0xF, 0xF, false); }
constexpr int QP_XOR1 = 0xB1, QP_XOR2 = 0x4E;                 // [1 0 3 2], [2 3 0 1]
template <int K> constexpr int qp_bcast() { return K * 0x55; }  // [K K K K]
// sum over the quad, the same bits on every lane: (x0 + x1) + (x2 + x3)
__device__ __forceinline__ double qsum(double x) {
  const double a = x + qmove<QP_XOR1>(x);
  return a + qmove<QP_XOR2>(a);
}
__device__ __forceinline__ int qor(int x) {
  const int a = x | qmove_i<QP_XOR1>(x);
  return a | qmove_i<QP_XOR2>(a);
}

}  // namespace wbc
