// wbc_gait_feedback.hpp -- the gait planner's foot-placement feedback (include/wbc_gait_feedback.h, "The law"; product
// code): its one text, instantiated by wbc_gait_feedback_kernel (wbc_gait_feedback.hip, a quad of lanes per robot, one foot per lane)
// and by tools/host_gait_feedback.cpp.  The clock and the packed stride are wbc_gait.hpp's, read and not edited.
//
// The state of `cap` instances is six rows of 4 cap doubles -- cur_x, cur_y, from_x, from_y, to_x, to_y -- with foot f of instance i at
// 4 i + f in its row, which is the kernel's global lane number: a wavefront's loads and stores of a row are one contiguous 512 B.
// After them come cap bytes, the contact masks of the previous call.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/wbc_gait_feedback.h"
#include "wbc_gait.hpp"

namespace wbc {

constexpr int GAIT_FEEDBACK_ROWS = 6;

// what is wrong with the arguments of wbc_gait_feedback_check, or nullptr
inline const char* gait_feedback_error(const wbc_gait_feedback_params* P) {
  if (!P) return "null params";
  if (!(P->k_v >= 0.0) || not_finite(P->k_v)) return "k_v must be non-negative and finite";
  if (!(P->k_p >= 0.0) || not_finite(P->k_p)) return "k_p must be non-negative and finite";
  if (!(P->d_max > 0.0) || not_finite(P->d_max)) return "d_max must be positive and finite";
  if (!(P->u_hold >= 0.0) || !(P->u_hold <= 1.0)) return "u_hold must lie in 0 .. 1";
  return nullptr;
}

// The offset d the measured trunk asks for, from the eight numbers: measured position and velocity (qx, qy, vx, vy), planned (px, py,
// pdx, pdy).  Returns whether all eight are finite (d is then finite too); otherwise d is not to be used.
WBC_HD bool gait_feedback_offset(const wbc_gait_feedback_params& P, double qx, double qy, double vx, double vy, double px, double py,
                                 double pdx, double pdy, double& dx, double& dy) {
  WBC_GAIT_NO_CONTRACT
  const bool bad = not_finite(qx) | not_finite(qy) | not_finite(vx) | not_finite(vy) | not_finite(px) | not_finite(py) | not_finite(pdx) |
                   not_finite(pdy);
  const double epx = qx - px, epy = qy - py, evx = vx - pdx, evy = vy - pdy;
  const double rx = P.k_v * evx + P.k_p * epx, ry = P.k_v * evy + P.k_p * epy;
  const double m = sqrt(rx * rx + ry * ry);
  const double g = fmin(1.0, P.d_max / m);
  dx = m == 0.0 ? 0.0 : rx * g;
  dy = m == 0.0 ? 0.0 : ry * g;
  return !bad;
}

// One foot of an instance whose numbers are all finite.  c: the instance's clock; down, was: the foot's contact bit now and in the
// previous call; (dx, dy): gait_feedback_offset's.  cur, from, to [2]: the foot's state, advanced.  add [6] <- what the rows p_x, p_y,
// pd_x, pd_y, pdd_x, pdd_y of the foot gain; add[0 .. 1] is also the `offsets` output.
WBC_HD void gait_feedback_foot(const wbc_gait_feedback_params& P, const GaitClock& c, int f, bool down, bool was, double dx, double dy,
                               double* cur, double* from, double* to, double* add) {
  WBC_GAIT_NO_CONTRACT
  const double* e = c.stride + 12 + 6 * (8 * f + c.phase);
  const double a = c.kT + c.s * e[0], b = c.kT + c.s * e[1];       // gait_foot's a and b
  const double D = b - a, u = (c.tau - a) / D, w = 1.0 - u, uw = u * w;
  const double sg = (u * u) * u * (10.0 + u * (6.0 * u - 15.0));
  const double sgd = 30.0 * (uw * uw) / D, sgdd = 60.0 * uw * (1.0 - 2.0 * u) / (D * D);
  const bool lift = !down & was, land = down & !was;
  const bool take = !down & (was | (u <= P.u_hold));
  const double d[2] = {dx, dy};
  WBC_GAIT_UNROLL
  for (int k = 0; k < 2; k++) {
    from[k] = lift ? cur[k] : from[k];
    to[k] = take ? d[k] : to[k];
    cur[k] = land ? to[k] : cur[k];
    const double step = to[k] - from[k];
    add[k] = down ? cur[k] : from[k] + step * sg;
    add[2 + k] = down ? 0.0 : step * sgd;
    add[4 + k] = down ? 0.0 : step * sgdd;
  }
}

// the clock of the pass: gait_clock on the instance's time, stride and scale.  The command and the start play no part in a clock; an
// instance they spoil has NaN rows, which is what the pass looks at.
WBC_HD GaitClock gait_feedback_clock(const double* table, int count, double time, int id, double s) {
  GaitIn in;
  in.time = time; in.id = id; in.s = s;
  in.cx = 0.0; in.cy = 0.0; in.w = 0.0; in.x0 = 0.0; in.y0 = 0.0; in.psi0 = 0.0;
  return gait_clock(table, count, in);
}

}  // namespace wbc
