// host_batch.hpp -- TEST TOOL, not product code.
// What the host instantiations of the two plants (host_plant.cpp, host_ground.cpp) do around their math, as the device kernels do
// it around theirs: gather one instance from the SoA batch (all four legs, the kernel's lane l being leg l here), check and clip
// its inputs, and scatter accelerations, state, time and flag counts back.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "../quadruped_drake_amd/csrc/wbc_model.hpp"
#include "../quadruped_drake_amd/csrc/wbc_plant.hpp"

namespace wbc {

// the quad sum in the kernel's order
inline double qsum4(const double* x) { return (x[0] + x[1]) + (x[2] + x[3]); }

struct HostInstance {
  double qb[7], vb[6], th[4][3], qd[4][3], tq[4][3], ta[4][3];   // base, then per leg: angles, rates, torques as given / clipped
  int qrow[4][3];                                                // the legs' joint rows in the caller's numbering
};

inline void host_gather(const ModelC& m, int i, size_t ld, const double* q, const double* v, const double* tau, HostInstance& s) {
  for (int k = 0; k < 7; k++) s.qb[k] = q[k * ld + i];
  for (int k = 0; k < 6; k++) s.vb[k] = v[k * ld + i];
  for (int l = 0; l < 4; l++)
    for (int k = 0; k < 3; k++) {
      s.qrow[l][k] = m.q_perm[3 * l + k];
      s.th[l][k] = q[(7 + s.qrow[l][k]) * ld + i];
      s.qd[l][k] = v[(6 + s.qrow[l][k]) * ld + i];
      s.tq[l][k] = tau[m.act_inv[3 * l + k] * ld + i];
    }
}

// true: something of the instance is not finite, or mu / s_p is not positive.  Sets `clip` and the clipped torques s.ta.
inline bool host_check_inputs(HostInstance& s, double tau_max, double mu, double s_p, bool& clip) {
  bool nf = false;
  clip = false;
  for (int k = 0; k < 7; k++) nf |= not_finite(s.qb[k]);
  for (int k = 0; k < 6; k++) nf |= not_finite(s.vb[k]);
  for (int l = 0; l < 4; l++)
    for (int k = 0; k < 3; k++) {
      nf |= not_finite(s.th[l][k]) | not_finite(s.qd[l][k]) | not_finite(s.tq[l][k]);
      clip |= fabs(s.tq[l][k]) > tau_max * (1.0 + PLANT_CLIP_TOL);
      s.ta[l][k] = fmin(fmax(s.tq[l][k], -tau_max), tau_max);
    }
  nf |= !(mu > 0.0) | not_finite(mu) | !(s_p > 0.0) | not_finite(s_p);
  return nf;
}

inline void host_store_vdot(const HostInstance& s, int i, size_t ld, bool bad, const double* vdb, const double (*vdl)[3], double* vdot) {
  for (int k = 0; k < 6; k++) vdot[k * ld + i] = bad ? 0.0 : vdb[k];
  for (int l = 0; l < 4; l++)
    for (int k = 0; k < 3; k++) vdot[(6 + s.qrow[l][k]) * ld + i] = bad ? 0.0 : vdl[l][k];
}

// the end of a step: the integrated state (s.qb, s.vb, s.th, s.qd) unless the instance is bad, the time, the flag counters
inline void host_store_step(const HostInstance& s, int i, size_t ld, bool bad, double dt, int bits, double* q, double* v, double* time,
                            int32_t* counts) {
  if (!bad) {
    for (int k = 0; k < 6; k++) v[k * ld + i] = s.vb[k];
    for (int k = 0; k < 7; k++) q[k * ld + i] = s.qb[k];
    for (int l = 0; l < 4; l++)
      for (int k = 0; k < 3; k++) {
        v[(6 + s.qrow[l][k]) * ld + i] = s.qd[l][k];
        q[(7 + s.qrow[l][k]) * ld + i] = s.th[l][k];
      }
  }
  if (time) time[i] += dt;
  if (counts)
    for (int b = 0; b < 4; b++)
      if ((bits >> b) & 1) counts[b * ld + i] += 1;
}

}  // namespace wbc
