// host_gait_feedback.cpp -- TEST TOOL, not product code.
// Instantiates the gait planner's foot-placement feedback (quadruped_drake_amd/csrc/wbc_gait_feedback.hpp) on the host: what the
// device kernel runs on the four lanes of a quad, here one foot after the other, on a state the caller holds in the device's layout.
// Part of tools/libhost_gait.so; tests/host_gait_feedback.py loads it; the shipped library never calls it.
#include <math.h>
#include <stdint.h>
#include "../quadruped_drake_amd/csrc/wbc_gait_feedback.hpp"

using namespace wbc;

extern "C" {

// state [6][4 cap] <- 0, prev [cap] <- 0xF: what wbc_gait_set_feedback leaves
void host_gait_feedback_reset(int cap, double* state, uint8_t* prev) {
  for (size_t k = 0; k < (size_t)GAIT_FEEDBACK_ROWS * 4 * (size_t)cap; k++) state[k] = 0.0;
  for (int i = 0; i < cap; i++) prev[i] = 0xF;
}

// The pass of wbc_gait_targets_measured with host pointers, on targets and contact_mask that a gait twin wrote: advances state and
// prev.  offsets: optional.  Returns 0, -1 on arguments wbc_gait_check refuses, -6 on what wbc_gait_feedback_check refuses, -7 for
// n > cap.
int host_gait_feedback_batch(const wbc_gait_params* params, const wbc_gait_stride* strides, int count, const wbc_gait_feedback_params* fp, int n,
                             int ld, const double* time, const uint8_t* gait_id, const double* stride_scale, const double* q, const double* v,
                             double* targets, const uint8_t* contact_mask, double* offsets, int cap, double* state, uint8_t* prev) {
  if (gait_error(params, strides, count)) return -1;
  if (gait_feedback_error(fp)) return -6;
  if (n > cap) return -7;
  double table[GAIT_TABLE_DOUBLES] = {0.0};
  gait_pack(params, strides, count, table);
  const size_t l = (size_t)ld, row = 4 * (size_t)cap;
  for (int i = 0; i < n; i++) {
    double* out = targets + i;
    const GaitClock c = gait_feedback_clock(table, count, time[i], gait_id ? (int)gait_id[i] : 0, stride_scale ? stride_scale[i] : 1.0);
    double dx, dy;
    bool bad = !gait_feedback_offset(*fp, q[4 * l + i], q[5 * l + i], v[3 * l + i], v[4 * l + i], out[0], out[l], out[3 * l], out[4 * l], dx, dy) |
               not_finite(time[i]);
    for (int k = 0; k < 54; k++) bad |= not_finite(out[(size_t)k * l]);
    const unsigned mask = contact_mask[i], was = prev[i];
    for (int f = 0; f < 4; f++) {
      const size_t w = 4 * (size_t)i + (size_t)f;
      double cur[2], from[2], to[2], add[6];
      for (int k = 0; k < 2; k++) { cur[k] = state[(size_t)k * row + w]; from[k] = state[(size_t)(2 + k) * row + w]; to[k] = state[(size_t)(4 + k) * row + w]; }
      gait_feedback_foot(*fp, c, f, (mask >> f) & 1u, (was >> f) & 1u, dx, dy, cur, from, to, add);
      if (!bad) {
        double* o = out + (size_t)(18 + 9 * f) * l;
        for (int k = 0; k < 2; k++) {
          o[(size_t)k * l] = o[(size_t)k * l] + add[k];
          o[(size_t)(3 + k) * l] = o[(size_t)(3 + k) * l] + add[2 + k];
          o[(size_t)(6 + k) * l] = o[(size_t)(6 + k) * l] + add[4 + k];
          state[(size_t)k * row + w] = cur[k]; state[(size_t)(2 + k) * row + w] = from[k]; state[(size_t)(4 + k) * row + w] = to[k];
        }
      }
      if (offsets) {
        offsets[(size_t)(2 * f) * l + i] = bad ? __builtin_nan("") : add[0];
        offsets[(size_t)(2 * f + 1) * l + i] = bad ? __builtin_nan("") : add[1];
      }
    }
    if (!bad) prev[i] = (uint8_t)mask;
  }
  return 0;
}

}  // extern "C"
