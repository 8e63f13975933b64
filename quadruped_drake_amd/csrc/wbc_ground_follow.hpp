// wbc_ground_follow.hpp -- targets that follow the terrain (include/wbc_ground.h, "Following the ground"; product code).
//
// The planners' 54 target rows are about the plane z = 0.  follow_instance rewrites one instance's rows, in place, for the terrain
// it stands on: every foot target is lifted onto the surface under it, the body target onto the line fitted through the four
// planned footholds, and in FOLLOW_FIT the body's attitude is turned with that line.  The law is the header's; this is its one
// text, instantiated by wbc_ground_follow_kernel (wbc_ground.hip, one thread per robot) and by tools/host_ground.cpp.
//
// The profile travels in registers: its 39 doubles are loaded once, after the target rows, and the piece under a point is picked
// by eight compares and selects (the knots increase, so the last knot at or below s names it) -- no indexed access to a local
// array, hence no scratch, and no load that waits for a piece's index.  The arithmetic of H and g is terrain_surface's.
#pragma once
#include <math.h>
#include <stddef.h>
#include "wbc_ground.hpp"

// pins a loaded value in its register at this point of the device code (the host has no use for it)
#if defined(__HIP_DEVICE_COMPILE__)
#define WBC_FOLLOW_HOLD(x) asm volatile("" : "+v"(x))
#else
#define WBC_FOLLOW_HOLD(x) (void)(x)
#endif

namespace wbc {

enum { FOLLOW_OFF = 0, FOLLOW_LIFT = 1, FOLLOW_FIT = 2 };
constexpr double FOLLOW_MIN_SPREAD = 1e-12;   // [m^2] sum of (s_i - s_mean)^2 below which the footholds give no slope
constexpr double FOLLOW_MIN_COS = 1e-9;       // |cos pitch'| below which rpy' has no rates
constexpr int FOLLOW_PROFILE_DOUBLES = TERRAIN_STRIDE - 1;   // the last double of a packed profile is padding

// s, and terrain_surface's H and g, of the profile held in `prof` under the world point (x, y)
template <class T> WBC_HD void follow_surface(const T* prof, T scale, T x, T y, T& s, T& H, T& g) {
  s = (x - prof[2]) * prof[0] + (y - prof[3]) * prof[1];
  T s0 = prof[12], h0 = prof[13], sl = prof[14];
  WBC_PLANT_UNROLL
  for (int k = 0; k < TERRAIN_MAX_KNOTS; k++) {
    const bool in = s >= prof[4 + k];
    s0 = in ? prof[15 + 3 * k] : s0;
    h0 = in ? prof[16 + 3 * k] : h0;
    sl = in ? prof[17 + 3 * k] : sl;
  }
  H = scale * (h0 + sl * (s - s0));
  g = scale * sl;
}

// The law on one instance's rows held in b (the 18 body rows) and f (the 36 foot rows).  mode: FOLLOW_LIFT or FOLLOW_FIT.
// Returns whether the nine attitude rows b[9 .. 17] were rewritten; lifted[c] says whether foot c's three z rows were.
template <class T> WBC_HD bool follow_law(int mode, const T* prof, T scale, T* b, T* f, bool* lifted) {
  const T cpsi = prof[0], spsi = prof[1];
  // ---- feet: onto the surface under them
  T s[4], H[4];
  WBC_PLANT_UNROLL
  for (int c = 0; c < 4; c++) {
    T* p = f + 9 * c;
    T g;
    follow_surface(prof, scale, p[0], p[1], s[c], H[c], g);
    lifted[c] = !(not_finite(p[0]) | not_finite(p[1]));
    p[2] = lifted[c] ? p[2] + H[c] : p[2];
    p[5] = lifted[c] ? p[5] + g * (p[3] * cpsi + p[4] * spsi) : p[5];
    p[8] = lifted[c] ? p[8] + g * (p[6] * cpsi + p[7] * spsi) : p[8];
  }
  // ---- the line H = Hm + slope (s - sm) through the usable footholds; the means are taken about the first of them, so that
  // equal heights give their own value back exactly
  T sb, Hb, gb;
  follow_surface(prof, scale, b[0], b[1], sb, Hb, gb);
  T sr = sb, Hr = Hb, cnt = T(0.0);
  WBC_PLANT_UNROLL
  for (int c = 3; c >= 0; c--) {
    sr = lifted[c] ? s[c] : sr;
    Hr = lifted[c] ? H[c] : Hr;
    cnt = cnt + (lifted[c] ? T(1.0) : T(0.0));
  }
  T ds = T(0.0), dH = T(0.0);
  WBC_PLANT_UNROLL
  for (int c = 0; c < 4; c++) {
    ds = ds + (lifted[c] ? s[c] - sr : T(0.0));
    dH = dH + (lifted[c] ? H[c] - Hr : T(0.0));
  }
  const T div = cnt > T(0.0) ? cnt : T(1.0);
  const T sm = sr + ds / div, Hm = Hr + dH / div;   // no usable foot: the body's own s and H
  T num = T(0.0), den = T(0.0);
  WBC_PLANT_UNROLL
  for (int c = 0; c < 4; c++) {
    const T es = lifted[c] ? s[c] - sm : T(0.0), eH = lifted[c] ? H[c] - Hm : T(0.0);
    num = num + es * eH;
    den = den + es * es;
  }
  const T slope = (cnt < T(2.0) || den < T(FOLLOW_MIN_SPREAD)) ? T(0.0) : num / den;
  // ---- body position: onto the line, x and y untouched
  b[2] = b[2] + (Hm + slope * (sb - sm));
  b[5] = b[5] + slope * (b[3] * cpsi + b[4] * spsi);
  b[8] = b[8] + slope * (b[6] * cpsi + b[7] * spsi);
  if (mode != FOLLOW_FIT || slope == T(0.0)) return false;   // R_fit = 1: the attitude stands as given
  // ---- body attitude: R' = R_fit Rz(yaw) Ry(pitch) Rx(roll), R_fit about (-sin psi, cos psi, 0) by -atan(slope)
  const T ct = T(1.0) / sqrt(T(1.0) + slope * slope), st = T(0.0) - slope * ct, k = T(1.0) - ct;
  const T F[9] = {ct + k * spsi * spsi, T(0.0) - k * spsi * cpsi, st * cpsi,
                  T(0.0) - k * spsi * cpsi, ct + k * cpsi * cpsi, st * spsi,
                  T(0.0) - st * cpsi, T(0.0) - st * spsi, ct};
  T sr_, cr_, sp_, cp_, sy_, cy_;
  wbc_sincos(b[9], sr_, cr_);
  wbc_sincos(b[10], sp_, cp_);
  wbc_sincos(b[11], sy_, cy_);
  // of R = Rz Ry Rx: its first column and, for the last row of R', all of it
  const T R[9] = {cy_ * cp_, cy_ * sp_ * sr_ - sy_ * cr_, cy_ * sp_ * cr_ + sy_ * sr_,
                  sy_ * cp_, sy_ * sp_ * sr_ + cy_ * cr_, sy_ * sp_ * cr_ - cy_ * sr_,
                  T(0.0) - sp_, cp_ * sr_, cp_ * cr_};
  const T r00 = F[0] * R[0] + F[1] * R[3] + F[2] * R[6];
  const T r10 = F[3] * R[0] + F[4] * R[3] + F[5] * R[6];
  const T r20 = F[6] * R[0] + F[7] * R[3] + F[8] * R[6];
  const T r21 = F[6] * R[1] + F[7] * R[4] + F[8] * R[7];
  const T r22 = F[6] * R[2] + F[7] * R[5] + F[8] * R[8];
  const T cpn = sqrt(r00 * r00 + r10 * r10);   // cos pitch' >= 0
  if (cpn < T(FOLLOW_MIN_COS)) return false;
  const T rpy[3] = {atan2(r21, r22), atan2(T(0.0) - r20, cpn), atan2(r10, r00)};
  // rates: w = E(rpy) rate, w' = R_fit w, rate' = E(rpy')^-1 w'   (no E-dot term, as everywhere in this project)
  // (the sines and cosines of pitch' and yaw' are the numbers their atan2 was taken of)
  const T spn = T(0.0) - r20, cpc = cpn, syn = r10 / cpn, cyn = r00 / cpn;
  WBC_PLANT_UNROLL
  for (int d = 0; d < 2; d++) {
    T* r = b + 12 + 3 * d;
    const T w[3] = {cp_ * cy_ * r[0] - sy_ * r[1], cp_ * sy_ * r[0] + cy_ * r[1], r[2] - sp_ * r[0]};
    const T u[3] = {F[0] * w[0] + F[1] * w[1] + F[2] * w[2], F[3] * w[0] + F[4] * w[1] + F[5] * w[2],
                    F[6] * w[0] + F[7] * w[1] + F[8] * w[2]};
    const T a = (cyn * u[0] + syn * u[1]) / cpc;
    r[0] = a;
    r[1] = cyn * u[1] - syn * u[0];
    r[2] = spn * a + u[2];
  }
  b[9] = rpy[0]; b[10] = rpy[1]; b[11] = rpy[2];
  return true;
}

// One instance of targets [54][ld], in place, on profile terrain_id[i] of `table` (count x TERRAIN_STRIDE doubles in memory) scaled
// by terrain_scale[i] (null pointers: profile 0, scale 1).  Every row the mode reads and the profile are loaded before the first
// store; the rows go out together with terrain_id and terrain_scale, the profile's address waits for terrain_id.  Only rows the law
// rewrote are stored: three z rows per usable foot, the body's three z rows, and in FOLLOW_FIT the nine attitude rows when they
// changed.  A terrain_id >= count or a non-finite scale: nothing is stored.
template <class T>
WBC_HD void follow_instance(int mode, const T* table, int count, const uint8_t* terrain_id, const T* terrain_scale, T* targets,
                            size_t ld, size_t i) {
  const bool fit = mode == FOLLOW_FIT;
  const int id = terrain_id ? (int)terrain_id[i] : 0;
  const T scale = terrain_scale ? terrain_scale[i] : T(1.0);
  T b[18], f[36], prof[FOLLOW_PROFILE_DOUBLES];
  WBC_PLANT_UNROLL
  for (int r = 0; r < 9; r++) b[r] = targets[r * ld + i];
  WBC_PLANT_UNROLL
  for (int r = 0; r < 36; r++) f[r] = targets[(18 + r) * ld + i];
  WBC_PLANT_UNROLL
  for (int r = 9; r < 18; r++) b[r] = T(0.0);
  if (fit) {
    WBC_PLANT_UNROLL
    for (int r = 9; r < 18; r++) b[r] = targets[r * ld + i];
  }
  // every row is in a register here: without this the compiler moves the loads down to where a row is used -- behind the check of
  // terrain_id, and a foot's z rows into the branch that stores them, where each waits for memory on its own
  WBC_PLANT_UNROLL
  for (int r = 0; r < 18; r++) WBC_FOLLOW_HOLD(b[r]);
  WBC_PLANT_UNROLL
  for (int r = 0; r < 36; r++) WBC_FOLLOW_HOLD(f[r]);
  if ((id >= count) | not_finite(scale)) return;
  const T* tab = table + id * TERRAIN_STRIDE;
  WBC_PLANT_UNROLL
  for (int k = 0; k < FOLLOW_PROFILE_DOUBLES; k++) prof[k] = tab[k];
  bool lifted[4];
  const bool turned = follow_law(mode, prof, scale, b, f, lifted);
  WBC_PLANT_UNROLL
  for (int c = 0; c < 4; c++)
    if (lifted[c]) {
      WBC_PLANT_UNROLL
      for (int d = 0; d < 3; d++) targets[(18 + 9 * c + 3 * d + 2) * ld + i] = f[9 * c + 3 * d + 2];
    }
  WBC_PLANT_UNROLL
  for (int d = 0; d < 3; d++) targets[(3 * d + 2) * ld + i] = b[3 * d + 2];
  if (turned) {
    WBC_PLANT_UNROLL
    for (int r = 9; r < 18; r++) targets[r * ld + i] = b[r];
  }
}

}  // namespace wbc
