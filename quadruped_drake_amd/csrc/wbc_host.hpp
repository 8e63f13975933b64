// wbc_host.hpp -- the host side that the five translation units of the C ABI share (wbc_kernels.hip, wbc_traj.hip, wbc_plant.hip,
// wbc_ground.hip, wbc_gait.hip; internal, not installed): error reporting, the checks of a caller's model table and joint numbering, and the
// answer of a *_kernel_info entry point.  Host code only: nothing here decides a device instruction.
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>

#include "../../include/wbc.h"
#include "wbc_model.hpp"
#include "wbc_device_guard.hpp"

extern "C" void wbc_set_error_(const char* msg);   // wbc_kernels.hip: the thread-local buffer wbc_last_error() returns

namespace wbc {

// ---- error reporting: the message goes behind wbc_last_error(), the return value is the entry point's
inline int fail(const char* what, hipError_t e) {
  char b[512];
  snprintf(b, sizeof b, "%s: %s", what, hipGetErrorString(e));
  wbc_set_error_(b);
  return -2;
}
inline int misuse(const char* what) { wbc_set_error_(what); return -1; }
inline int misuse(const char* fn, const char* what) {   // "<entry point>: <what>"
  char b[512];
  snprintf(b, sizeof b, "%s: %s", fn, what);
  return misuse(b);
}
#define HIP_TRY(x)                                   \
  do {                                               \
    hipError_t e_ = (x);                             \
    if (e_ != hipSuccess) return wbc::fail(#x, e_);  \
  } while (0)

// ---- the caller's model
// The table as the kernels take it: axis-aligned joints in the x-y-y tree.  The permutations stay the identity.
inline int model_axes(const char* fn, const wbc_model* model, ModelC* m) {
  if (model_from_flat(model->flat, m)) return misuse(fn, "joint axes must be axis-aligned");
  if (!model_axes_are_xyy(m))
    return misuse(fn, "unsupported kinematic tree -- the kernels are specialised to legs with the abduction joint "
                      "about +-x and the hip and knee joints about +-y (Mini Cheetah, ANYmal)");
  return 0;
}

// model_axes, then the caller's joint and actuator numbering
inline int model_checked(const char* fn, const wbc_model* model, ModelC* m) {
  const int rc = model_axes(fn, model, m);
  if (rc) return rc;
  bool seen_q[12] = {0}, seen_a[12] = {0};
  int qp[12], ap[12];
  for (int i = 0; i < 12; i++) {
    qp[i] = model->q_perm[i]; ap[i] = model->act_perm[i];
    if (qp[i] < 0 || qp[i] >= 12 || ap[i] < 0 || ap[i] >= 12 || seen_q[qp[i]] || seen_a[ap[i]])
      return misuse(fn, "q_perm/act_perm must be permutations of 0..11");
    seen_q[qp[i]] = seen_a[ap[i]] = true;
  }
  model_set_perms(m, qp, ap);
  return 0;
}

// Actuator k drives canonical joint act_perm[k], which is joint q_perm[act_perm[k]] of the plant's order (a null permutation is
// the identity): jd[k] <- that plant joint, checked to be a permutation.
inline int actuator_joints(const char* fn, const int* q_perm, const int* act_perm, int* jd) {
  bool seen[12] = {false};
  for (int k = 0; k < 12; k++) {
    const int j = act_perm ? act_perm[k] : k;
    if (j < 0 || j >= 12) return misuse(fn, "act_perm must be a permutation of 0..11");
    jd[k] = q_perm ? q_perm[j] : j;
    if (jd[k] < 0 || jd[k] >= 12 || seen[jd[k]]) return misuse(fn, "q_perm / act_perm must be permutations of 0..11");
    seen[jd[k]] = true;
  }
  return 0;
}

// ---- the answer of a *_kernel_info entry point; `what` is the failing call as wbc_last_error() reports it
inline int kernel_info(int device, const void* kernel, const char* what, int threads, int* num_vgpr, int* scratch_bytes,
                       int* lds_bytes, int* block_threads) {
  WBC_ON_DEVICE(device, fail);
  hipFuncAttributes fa;
  const hipError_t e = hipFuncGetAttributes(&fa, kernel);
  if (e != hipSuccess) return fail(what, e);
  if (num_vgpr) *num_vgpr = fa.numRegs;
  if (scratch_bytes) *scratch_bytes = (int)fa.localSizeBytes;
  if (lds_bytes) *lds_bytes = (int)fa.sharedSizeBytes;
  if (block_threads) *block_threads = threads;
  return 0;
}

}  // namespace wbc
