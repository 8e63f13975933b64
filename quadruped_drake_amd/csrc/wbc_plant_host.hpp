// wbc_plant_host.hpp -- the host side that the C ABIs of the two plants share (wbc_plant.hip, wbc_ground.hip; internal, not
// installed): error reporting, the model a plant is created from and its upload, the argument checks of a batch, the launch
// grid, the kernel_info answer and the controller-to-plant rollout loop.  Every message carries the calling entry point's
// name, which each function takes as `fn`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/wbc.h"
#include "wbc_model.hpp"
#include "wbc_quad.hpp"
#include "wbc_device_guard.hpp"

extern "C" void wbc_set_error_(const char* msg);   // wbc_kernels.hip: the buffer wbc_last_error() returns

namespace wbc {

inline int plant_fail(const char* what, hipError_t e) {
  char b[512];
  snprintf(b, sizeof b, "%s: %s", what, hipGetErrorString(e));
  wbc_set_error_(b);
  return -2;
}
inline int plant_misuse(const char* what) { wbc_set_error_(what); return -1; }
inline int plant_misuse(const char* fn, const char* what) {
  char b[512];
  snprintf(b, sizeof b, "%s: %s", fn, what);
  return plant_misuse(b);
}
#define WBC_PLANT_TRY(x)                                   \
  do {                                                     \
    hipError_t e_ = (x);                                   \
    if (e_ != hipSuccess) return wbc::plant_fail(#x, e_);  \
  } while (0)

// The caller's table as the plant math takes it: axis-aligned joints in the x-y-y tree.  The permutations stay the identity.
inline int plant_model_axes(const char* fn, const wbc_model* model, ModelC* m) {
  if (model_from_flat(model->flat, m)) return plant_misuse(fn, "joint axes must be axis-aligned");
  if (!model_axes_are_xyy(m))
    return plant_misuse(fn, "unsupported kinematic tree -- legs with the abduction joint about +-x and the hip and knee joints "
                            "about +-y (Mini Cheetah, ANYmal)");
  return 0;
}

// plant_model_axes, then the caller's joint and actuator numbering
inline int plant_model(const char* fn, const wbc_model* model, ModelC* m) {
  const int rc = plant_model_axes(fn, model, m);
  if (rc) return rc;
  bool seen_q[12] = {0}, seen_a[12] = {0};
  int qp[12], ap[12];
  for (int i = 0; i < 12; i++) {
    qp[i] = model->q_perm[i]; ap[i] = model->act_perm[i];
    if (qp[i] < 0 || qp[i] >= 12 || ap[i] < 0 || ap[i] >= 12 || seen_q[qp[i]] || seen_a[ap[i]])
      return plant_misuse(fn, "q_perm/act_perm must be permutations of 0..11");
    seen_q[qp[i]] = seen_a[ap[i]] = true;
  }
  model_set_perms(m, qp, ap);
  return 0;
}

// a copy of m in `device`'s memory; the caller frees it
inline int plant_model_upload(int device, const ModelC& m, ModelC** out) {
  WBC_ON_DEVICE(device, plant_fail);
  ModelC* d = nullptr;
  WBC_PLANT_TRY(hipMalloc(&d, sizeof m));
  const hipError_t e = hipMemcpy(d, &m, sizeof m, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(d);
    return plant_fail("hipMemcpy(model)", e);
  }
  *out = d;
  return 0;
}

// The arguments every batch entry point takes.  `handle`: the plant's handle, called "<noun> handle"; `have_arrays`: whether the
// arrays named by `arrays` ("q, v and tau") are all there.
inline int plant_check_batch(const char* fn, const void* handle, const char* noun, int n, int ld, bool have_arrays, const char* arrays) {
  char b[256];
  if (n < 0 || n > WBC_MAX_LD) return plant_misuse(fn, "n out of range (0 .. WBC_MAX_LD)");
  if (ld > WBC_MAX_LD) return plant_misuse(fn, "ld exceeds WBC_MAX_LD");
  if (n > 0 && ld < n) return plant_misuse(fn, "ld must be >= n");
  if (!handle) { snprintf(b, sizeof b, "null %s handle", noun); return plant_misuse(fn, b); }
  if (n > 0 && !have_arrays) { snprintf(b, sizeof b, "%s are required", arrays); return plant_misuse(fn, b); }
  return 0;
}

// a quad of lanes per robot
inline dim3 plant_grid(int n) { return dim3((unsigned)(((size_t)n * 4 + QUAD_BLOCK - 1) / QUAD_BLOCK)); }

// the answer of a *_kernel_info entry point; `what` is the failing call as wbc_last_error() reports it
inline int plant_kernel_info(int device, const void* kernel, const char* what, int* num_vgpr, int* scratch_bytes, int* lds_bytes,
                             int* block_threads) {
  WBC_ON_DEVICE(device, plant_fail);
  hipFuncAttributes fa;
  const hipError_t e = hipFuncGetAttributes(&fa, kernel);
  if (e != hipSuccess) return plant_fail(what, e);
  if (num_vgpr) *num_vgpr = fa.numRegs;
  if (scratch_bytes) *scratch_bytes = (int)fa.localSizeBytes;
  if (lds_bytes) *lds_bytes = (int)fa.sharedSizeBytes;
  if (block_threads) *block_threads = QUAD_BLOCK;
  return 0;
}
#define WBC_PLANT_KERNEL_INFO(device, kernel, ...) \
  wbc::plant_kernel_info(device, (const void*)kernel, "hipFuncGetAttributes(&fa, (const void*)" #kernel ")", __VA_ARGS__)

// `steps` x (target lookup at time -> controller tick -> plant step) on `device`, the plant step being `launch()`.  The batch
// arguments were checked by the caller.  A host-pointer controller handle is refused before anything is launched.
template <class Launch>
int plant_rollout(const char* fn, wbc_handle h, wbc_traj traj, int device, void* hip_stream, int steps, int n, int ld, double* q,
                  double* v, double* time, double* targets, uint8_t* contact_mask, const double* mu, const double* mass_scale,
                  double* tau, double* metrics, int32_t* status, Launch launch) {
  // wbc_integrate with n = 0 is an argument check only
  if (wbc_integrate(h, 0, 0, 0.0, nullptr, nullptr, nullptr)) return plant_misuse(fn, "needs a WBC_DEVICE_PTRS controller handle");
  if (steps == 0 || n == 0) return 0;
  int rc = wbc_set_stream(h, hip_stream);
  if (rc) return rc;
  WBC_ON_DEVICE(device, plant_fail);
  for (int s = 0; s < steps; s++) {
    rc = wbc_traj_lookup(traj, hip_stream, n, ld, time, targets, contact_mask);
    if (rc) return rc;
    rc = wbc_step(h, n, ld, q, v, targets, contact_mask, mu, mass_scale, tau, metrics, status);
    if (rc) return rc;
    rc = launch();
    if (rc) return rc;
  }
  return 0;
}

}  // namespace wbc
