// wbc_plant_host.hpp -- the host side that only the C ABIs of the two plants share (wbc_plant.hip, wbc_ground.hip; internal, not
// installed): the upload of a plant's model, the argument checks of a batch, the launch grid, the kernel_info answer and the
// controller-to-plant rollout loop.  Error reporting and the model checks are wbc_host.hpp's.  Every message carries the calling
// entry point's name, which each function takes as `fn`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "wbc_host.hpp"
#include "wbc_quad.hpp"

namespace wbc {

// a copy of m in `device`'s memory; the caller frees it
inline int plant_model_upload(int device, const ModelC& m, ModelC** out) {
  WBC_ON_DEVICE(device, fail);
  ModelC* d = nullptr;
  HIP_TRY(hipMalloc(&d, sizeof m));
  const hipError_t e = hipMemcpy(d, &m, sizeof m, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(d);
    return fail("hipMemcpy(model)", e);
  }
  *out = d;
  return 0;
}

// The arguments every batch entry point takes.  `handle`: the plant's handle, called "<noun> handle"; `have_arrays`: whether the
// arrays named by `arrays` ("q, v and tau") are all there.
inline int plant_check_batch(const char* fn, const void* handle, const char* noun, int n, int ld, bool have_arrays, const char* arrays) {
  char b[256];
  if (n < 0 || n > WBC_MAX_LD) return misuse(fn, "n out of range (0 .. WBC_MAX_LD)");
  if (ld > WBC_MAX_LD) return misuse(fn, "ld exceeds WBC_MAX_LD");
  if (n > 0 && ld < n) return misuse(fn, "ld must be >= n");
  if (!handle) { snprintf(b, sizeof b, "null %s handle", noun); return misuse(fn, b); }
  if (n > 0 && !have_arrays) { snprintf(b, sizeof b, "%s are required", arrays); return misuse(fn, b); }
  return 0;
}

// a quad of lanes per robot
inline dim3 plant_grid(int n) { return dim3((unsigned)(((size_t)n * 4 + QUAD_BLOCK - 1) / QUAD_BLOCK)); }

// the answer of a plant's *_kernel_info entry point
#define WBC_PLANT_KERNEL_INFO(device, kernel, ...) \
  wbc::kernel_info(device, (const void*)kernel, "hipFuncGetAttributes(&fa, (const void*)" #kernel ")", wbc::QUAD_BLOCK, __VA_ARGS__)

// `steps` x (target lookup at time -> controller tick -> plant step) on `device`, the plant step being `launch()`.  The batch
// arguments were checked by the caller.  A host-pointer controller handle is refused before anything is launched.
// `between()` runs after the lookup and before the tick, on the targets the lookup wrote; by default it does nothing.
// `source(traj, hip_stream, n, ld, time, targets, contact_mask)` writes a tick's targets and mask; by default it is the lookup in
// `traj` (a gait set on the plant handle takes its place: include/wbc_gait.h).
struct NoRolloutHook {
  int operator()() const { return 0; }
};
struct TrajLookupSource {
  int operator()(wbc_traj traj, void* hip_stream, int n, int ld, const double* time, double* targets, uint8_t* contact_mask) const {
    return wbc_traj_lookup(traj, hip_stream, n, ld, time, targets, contact_mask);
  }
};
template <class Launch, class Between = NoRolloutHook, class Source = TrajLookupSource>
int plant_rollout(const char* fn, wbc_handle h, wbc_traj traj, int device, void* hip_stream, int steps, int n, int ld, double* q,
                  double* v, double* time, double* targets, uint8_t* contact_mask, const double* mu, const double* mass_scale,
                  double* tau, double* metrics, int32_t* status, Launch launch, Between between = Between(), Source source = Source()) {
  // wbc_integrate with n = 0 is an argument check only
  if (wbc_integrate(h, 0, 0, 0.0, nullptr, nullptr, nullptr)) return misuse(fn, "needs a WBC_DEVICE_PTRS controller handle");
  if (steps == 0 || n == 0) return 0;
  int rc = wbc_set_stream(h, hip_stream);
  if (rc) return rc;
  WBC_ON_DEVICE(device, fail);
  for (int s = 0; s < steps; s++) {
    rc = source(traj, hip_stream, n, ld, time, targets, contact_mask);
    if (rc) return rc;
    rc = between();
    if (rc) return rc;
    rc = wbc_step(h, n, ld, q, v, targets, contact_mask, mu, mass_scale, tau, metrics, status);
    if (rc) return rc;
    rc = launch();
    if (rc) return rc;
  }
  return 0;
}

}  // namespace wbc
