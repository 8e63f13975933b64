// wbc_gait.hpp -- the gait planner's law (include/wbc_gait.h, "The law"; product code): its one text, instantiated by
// wbc_gait_targets_kernel (wbc_gait.hip, a quad of lanes per robot, one foot per lane), by the kernels of wbc_gait_schedule.hip (the
// SCHEDULE instantiations: "command schedules" below) and by tools/host_gait.cpp.
//
// The host packs the parameters and every stride into one table of doubles (gait_pack): per (foot, phase) the bounds of the run the
// phase lies in, relative to the start of the stride in progress, and for a swing run the bounds of the stance runs before and after
// it -- so the device searches for no run and divides only where the law does.  The phase is picked by seven compares, a run's
// six numbers by one indexed read of the table (LDS on the device): no indexed private array, hence no scratch.
//
//   table[0 .. 7]   stance[4][2]      table[8 .. 11]  height, swing_height, ramp_time, wait_time
//   stride p at table + GAIT_HEAD + p * GAIT_STRIDE:
//     [0 .. 6]  B_1 .. B_7, +inf from B_nphase on     [7] B_nphase     [8] the masks, phase j in bits 4j .. 4j+3     [9 .. 11] unused
//     [12 + 6 (8 f + j) ..]  a, b of foot f's run around phase j; pa, pb and na, nb of the stance runs before and after it when it is
//                            a swing run, a, b twice more when it is a stance run; a foot always in contact: -inf everywhere
//
// With a terrain (include/wbc_gait_terrain.h; the TERRAIN instantiations of gait_foot and gait_body) a second table
// rides beside the first: GAIT_TERRAIN_HEAD doubles of the handle's terrain parameters, then wbc_ground.hpp's packed profiles
// (terrain_pack, TERRAIN_STRIDE doubles each), which the plant's kernels read too.
//   ter[0] max_grade   [1] edge_margin   [2] apex_max   [3] unused
//   ter[4 .. 7] xt_f / sum xt^2,  ter[8 .. 11] yt_f / sum yt^2: the lever arms of the attitude fit over their sums, all zero with LIFT
//   profile p at ter + GAIT_TERRAIN_HEAD + p * TERRAIN_STRIDE
// The scans over a profile's knots run over all 8 padded knots with selects: +inf knots hold no foothold and bound no swing, and the
// padded pieces have slope 0, so they are never steep.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/wbc_gait.h"
#include "../../include/wbc_gait_terrain.h"
#include "wbc_tick.hpp"
#include "wbc_ground.hpp"

// the clock's arithmetic is rounded operation by operation on every instantiation (the header fixes k, r and the run times)
#if defined(__clang__)
#define WBC_GAIT_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define WBC_GAIT_NO_CONTRACT
#endif
#if defined(__HIPCC__)
#define WBC_GAIT_UNROLL _Pragma("unroll")
#else
#define WBC_GAIT_UNROLL
#endif

namespace wbc {

constexpr int GAIT_HEAD = 12;
constexpr int GAIT_STRIDE = 12 + 6 * 8 * 4;                                      // 204 doubles
constexpr int GAIT_TABLE_DOUBLES = GAIT_HEAD + WBC_GAIT_MAX_STRIDES * GAIT_STRIDE;   // 3276 doubles, 26208 B
constexpr double GAIT_SINC_SMALL = 1e-4;
constexpr int GAIT_TERRAIN_HEAD = 12;
constexpr int GAIT_TERRAIN_DOUBLES = GAIT_TERRAIN_HEAD + TERRAIN_MAX_PROFILES * TERRAIN_STRIDE;   // 652 doubles, 5216 B

// ---------------------------------------------------------------- host: checks and the packed table
// what is wrong with the arguments of wbc_gait_check, or nullptr
inline const char* gait_error(const wbc_gait_params* P, const wbc_gait_stride* S, int count) {
  if (!P || !S) return "null params or strides";
  if (count < 1 || count > WBC_GAIT_MAX_STRIDES) return "count must be 1 .. WBC_GAIT_MAX_STRIDES (16)";
  const double* p = &P->stance[0][0];
  for (int k = 0; k < 8; k++)
    if (not_finite(p[k])) return "stance must be finite";
  if (not_finite(P->height) || not_finite(P->swing_height) || not_finite(P->wait_time)) return "height, swing_height and wait_time must be finite";
  if (!(P->ramp_time >= 0.0) || not_finite(P->ramp_time)) return "ramp_time must be non-negative and finite";
  for (int s = 0; s < count; s++) {
    const wbc_gait_stride& g = S[s];
    if (g.nphase < 1 || g.nphase > WBC_GAIT_MAX_PHASES) return "nphase must be 1 .. WBC_GAIT_MAX_PHASES (8)";
    unsigned any = 0;
    for (int j = 0; j < g.nphase; j++) {
      if (!(g.duration[j] > 0.0) || not_finite(g.duration[j])) return "every duration must be positive and finite";
      if (g.contact[j] > 0xF) return "a contact mask has bits above 0xF";
      any |= g.contact[j];
    }
    if (any != 0xF) return "every foot must be in contact in at least one phase";
  }
  return nullptr;
}

// table <- the parameters and `count` checked strides
inline void gait_pack(const wbc_gait_params* P, const wbc_gait_stride* S, int count, double* table) {
  for (int k = 0; k < 8; k++) table[k] = (&P->stance[0][0])[k];
  table[8] = P->height; table[9] = P->swing_height; table[10] = P->ramp_time; table[11] = P->wait_time;
  for (int s = 0; s < count; s++) {
    const wbc_gait_stride& g = S[s];
    double* t = table + GAIT_HEAD + s * GAIT_STRIDE;
    const int n = g.nphase;
    double B[WBC_GAIT_MAX_PHASES + 1];
    B[0] = 0.0;
    for (int j = 0; j < n; j++) B[j + 1] = B[j] + g.duration[j];
    // the time of boundary i, any integer: B_(i mod n) + floor(i / n) B_n
    auto at = [&](int i) {
      int m = 0;
      while (i < 0) { i += n; m--; }
      while (i >= n) { i -= n; m++; }
      return B[i] + (double)m * B[n];
    };
    double masks = 0.0, w = 1.0;
    for (int j = 0; j < 8; j++) {
      if (j < 7) t[j] = (j + 1 < n) ? B[j + 1] : INFINITY;
      if (j < n) masks += w * (double)g.contact[j];
      w *= 16.0;
    }
    t[7] = B[n]; t[8] = masks; t[9] = t[10] = t[11] = 0.0;
    for (int f = 0; f < 4; f++) {
      auto bit = [&](int i) { return (g.contact[((i % n) + n) % n] >> f) & 1; };
      bool always = true;
      for (int j = 0; j < n; j++) always &= bit(j) == 1;
      for (int j = 0; j < 8; j++) {
        double* e = t + 12 + 6 * (8 * f + j);
        if (j >= n || always) {
          for (int k = 0; k < 6; k++) e[k] = (j < n) ? -INFINITY : 0.0;
          continue;
        }
        int lo = j, hi = j + 1;                           // the run is the phases lo .. hi-1: boundaries lo and hi
        while (bit(lo - 1) == bit(j)) lo--;
        while (bit(hi) == bit(j)) hi++;
        e[0] = at(lo); e[1] = at(hi);
        if (bit(j)) {
          e[2] = e[0]; e[3] = e[1]; e[4] = e[0]; e[5] = e[1];
        } else {
          int plo = lo, nhi = hi + 1;                     // the stance runs plo .. lo and hi .. nhi
          while (bit(plo - 1) == 1) plo--;
          while (bit(nhi) == 1) nhi++;
          e[2] = at(plo); e[3] = at(lo); e[4] = at(hi); e[5] = at(nhi);
        }
      }
    }
  }
}

// what is wrong with the arguments of wbc_gait_terrain_check apart from the profiles themselves (wbc_terrain_check), or nullptr
inline const char* gait_terrain_error(const wbc_gait_terrain_params* P) {
  if (!P) return "null params";
  if (P->body_mode != WBC_GAIT_BODY_LIFT && P->body_mode != WBC_GAIT_BODY_FIT) return "body_mode must be WBC_GAIT_BODY_LIFT (0) or WBC_GAIT_BODY_FIT (1)";
  if (!(P->max_grade > 0.0) || not_finite(P->max_grade)) return "max_grade must be positive and finite";
  if (!(P->edge_margin >= 0.0) || not_finite(P->edge_margin)) return "edge_margin must be non-negative and finite";
  if (not_finite(P->apex_max)) return "apex_max must be finite";
  return nullptr;
}

// what in the terrain parameters does not fit the gait whose packed table is `table`, or nullptr
inline const char* gait_terrain_fit_error(const wbc_gait_terrain_params* P, const double* table) {
  if (!(P->apex_max >= table[9])) return "apex_max must be at least the gait's swing_height";
  if (P->body_mode == WBC_GAIT_BODY_FIT) {
    const double mx = 0.25 * ((table[0] + table[2]) + (table[4] + table[6])), my = 0.25 * ((table[1] + table[3]) + (table[5] + table[7]));
    double sxx = 0.0, syy = 0.0;
    for (int f = 0; f < 4; f++) { sxx += (table[2 * f] - mx) * (table[2 * f] - mx); syy += (table[2 * f + 1] - my) * (table[2 * f + 1] - my); }
    if (!(sxx > 0.0) || !(syy > 0.0)) return "body_mode FIT needs a stance that spans x and y (sum xt^2 > 0 and sum yt^2 > 0)";
  }
  return nullptr;
}

// ter <- the terrain parameters, the lever arms of the gait packed in `table`, and `count` checked profiles
inline void gait_terrain_pack(const wbc_gait_terrain_params* P, const double* table, const wbc_terrain_profile* prof, int count, double* ter) {
  ter[0] = P->max_grade; ter[1] = P->edge_margin; ter[2] = P->apex_max; ter[3] = 0.0;
  const double mx = 0.25 * ((table[0] + table[2]) + (table[4] + table[6])), my = 0.25 * ((table[1] + table[3]) + (table[5] + table[7]));
  double sxx = 0.0, syy = 0.0;
  for (int f = 0; f < 4; f++) { sxx += (table[2 * f] - mx) * (table[2 * f] - mx); syy += (table[2 * f + 1] - my) * (table[2 * f + 1] - my); }
  const bool fit = P->body_mode == WBC_GAIT_BODY_FIT;
  for (int f = 0; f < 4; f++) {
    ter[4 + f] = fit ? (table[2 * f] - mx) / sxx : 0.0;
    ter[8 + f] = fit ? (table[2 * f + 1] - my) / syy : 0.0;
  }
  for (int p = 0; p < count; p++)
    terrain_pack(prof[p].nk, prof[p].x0, prof[p].y0, prof[p].yaw, prof[p].s, prof[p].h, ter + GAIT_TERRAIN_HEAD + p * TERRAIN_STRIDE);
}

// ---------------------------------------------------------------- host and device: one instance
struct GaitIn {        // what an instance brings
  double time, cx, cy, w, s, x0, y0, psi0;
  int id;
};
struct GaitClock {     // where an instance is in its stride
  bool bad, pre;       // malformed; tau < 0 (standing)
  double tau, s, k, kT;   // kT: the start of the stride in progress
  int phase;
  unsigned mask;
  const double* stride;
};

// theta, theta', theta'' at t >= 0
WBC_HD void gait_theta(double ramp, double t, double& th, double& thd, double& thdd) {
  const double x = t / ramp, y = 1.0 - x;               // ramp = 0: not used below
  const bool in = t < ramp;
  th = in ? ramp * ((x * x) * (x * x) * (2.5 + x * (x - 3.0))) : t - 0.5 * ramp;
  thd = in ? (x * x) * x * (10.0 + x * (6.0 * x - 15.0)) : 1.0;
  thdd = in ? 30.0 * (x * x) * (y * y) / ramp : 0.0;
}

// the body's (x, y) and the cosine and sine of its yaw at path parameter th
WBC_HD void gait_pose(const GaitIn& in, double th, double& x, double& y, double& cpsi, double& spsi) {
  const double a = 0.5 * (in.w * th);
  double sa, ca, sm, cm;
  wbc_sincos(a, sa, ca);
  wbc_sincos(in.psi0 + a, sm, cm);
  const double sinc = fabs(a) < GAIT_SINC_SMALL ? 1.0 - a * a / 6.0 : sa / a;
  const double g = th * sinc;
  x = in.x0 + g * (cm * in.cx - sm * in.cy);
  y = in.y0 + g * (sm * in.cx + cm * in.cy);
  cpsi = cm * ca - sm * sa;
  spsi = sm * ca + cm * sa;
}

// the clock of one instance; `count` strides in `table`.  A malformed instance runs on stride 0 at scale 1 and is answered with NaN.
WBC_HD GaitClock gait_clock(const double* table, int count, const GaitIn& in) {
  WBC_GAIT_NO_CONTRACT
  GaitClock c;
  c.bad = (in.id >= count) | !(in.s > 0.0) | not_finite(in.s) | not_finite(in.time) | not_finite(in.cx) | not_finite(in.cy) |
          not_finite(in.w) | not_finite(in.x0) | not_finite(in.y0) | not_finite(in.psi0);
  c.stride = table + GAIT_HEAD + (c.bad ? 0 : in.id) * GAIT_STRIDE;
  c.s = c.bad ? 1.0 : in.s;
  c.tau = in.time - table[11];
  c.pre = c.tau < 0.0;
  const double T = c.s * c.stride[7];
  double k = floor(c.tau / T);
  k = (k * T > c.tau) ? k - 1.0 : k;
  k = ((k + 1.0) * T <= c.tau) ? k + 1.0 : k;
  c.k = k;
  c.kT = k * T;
  const double r = c.tau - c.kT;
  int j = 0;
  WBC_GAIT_UNROLL
  for (int m = 0; m < 7; m++) j += (r >= c.s * c.stride[m]) ? 1 : 0;
  c.phase = j;
  // a clock that does not resolve in double is malformed too (the header's rule): T, and from tau = 0 on k T and the run [a, b) of
  // every foot that has one -- a and b as gait_foot forms them, the -inf of a foot that is always down exempt
  bool lost = !(T > 0.0) | not_finite(T);
  WBC_GAIT_UNROLL
  for (int f = 0; f < 4; f++) {
    const double* e = c.stride + 12 + 6 * (8 * f + j);
    const double a = c.kT + c.s * e[0], b = c.kT + c.s * e[1], D = b - a;
    lost |= !c.pre & (e[0] != -INFINITY) & (!(D > 0.0) | not_finite(D));
  }
  c.bad |= lost | (!c.pre & not_finite(c.kT));
  c.mask = (c.bad | c.pre) ? 0xFu : (((unsigned)c.stride[8] >> (4 * j)) & 0xFu);
  return c;
}

// the terrain an instance walks on: its packed profile and scale.  A malformed one walks on profile 0 at scale 1 and is answered
// with NaN (the caller ORs `bad` into its clock).
struct GaitGround {
  bool bad;
  const double* tab;
  double scale;
};
WBC_HD GaitGround gait_ground(const double* ter, int count, int id, double scale) {
  GaitGround g;
  g.bad = (id >= count) | not_finite(scale);
  g.tab = ter + GAIT_TERRAIN_HEAD + (g.bad ? 0 : id) * TERRAIN_STRIDE;
  g.scale = g.bad ? 1.0 : scale;
  return g;
}
WBC_HD void gait_clock_spoil(GaitClock& c, bool bad) {
  c.bad |= bad;
  c.mask = bad ? 0xFu : c.mask;
}

// The flat law's foothold (x, y) put on the terrain: moved off the first steep piece whose margin holds it unless `fixed` (a
// start-pose foothold); s: the foothold's coordinate along the profile, z: the height there.
WBC_HD void gait_foothold_on(const double* ter, const GaitGround& G, bool fixed, double& x, double& y, double& s, double& z) {
  const double* tab = G.tab;
  const double sF = (x - tab[2]) * tab[0] + (y - tab[3]) * tab[1];
  double e = sF;
  bool found = fixed;
  WBC_GAIT_UNROLL
  for (int j = 1; j < TERRAIN_MAX_KNOTS; j++) {                   // piece j of the packed profile: between knots j - 1 and j
    const double lo = tab[4 + j - 1] - ter[1], hi = tab[4 + j] + ter[1];
    const bool steep = fabs(G.scale * tab[12 + 3 * j + 2]) > ter[0];
    const bool hit = steep & (sF > lo) & (sF < hi) & !found;
    const double end = (hi - sF <= sF - lo) ? hi : lo;
    e = hit ? end : e;
    found |= hit;
  }
  x = x + (e - sF) * tab[0];
  y = y + (e - sF) * tab[1];
  s = e;
  int j = 0;
  WBC_GAIT_UNROLL
  for (int k = 0; k < TERRAIN_MAX_KNOTS; k++) j += (e >= tab[4 + k]) ? 1 : 0;
  const double* seg = tab + 12 + 3 * j;
  z = G.scale * (seg[1] + seg[2] * (e - seg[0]));
}

// the apex of a swing from (sA, zA) to (sB, zB): swing_height, raised over every knot strictly between them, capped
WBC_HD double gait_apex(const double* ter, const GaitGround& G, double swing_height, double sA, double zA, double sB, double zB) {
  const double* tab = G.tab;
  const double lo = fmin(sA, sB), hi = fmax(sA, sB), ds = sB - sA, dz = zB - zA;
  double m = 0.0;
  WBC_GAIT_UNROLL
  for (int k = 0; k < TERRAIN_MAX_KNOTS; k++) {
    const double sk = tab[4 + k], hk = tab[12 + 3 * (k + 1) + 1];   // knot k starts piece k + 1
    const bool inside = (sk > lo) & (sk < hi);
    const double lam = (sk - sA) / ds;
    const double q = (G.scale * hk - (zA + lam * dz)) / (4.0 * lam * (1.0 - lam));
    m = (inside & (q > m)) ? q : m;
  }
  return fmin(ter[2], swing_height + m);
}

// ---------------------------------------------------------------- command schedules (include/wbc_gait_schedule.h)
// wbc_gait_set_schedule resolves every instance's switches once (gait_schedule_resolve, one thread per instance) into GAIT_KNOT_ROWS
// rows per switch of a buffer [7 * GAIT_KNOT_ROWS][ld]; the SCHEDULE instantiations of gait_foot and gait_body then find a path
// parameter's segment by seven compares and read that switch's rows only (gait_schedule_pose).  Rows of switch j (0-based):
//   [0] Theta_j: +inf from the instance's m on; NaN in switch 0: the instance's schedule is invalid
//   [1 .. 3] S_j = (x, y, psi)     [4 .. 6] c_j = (cx, cy, omega)
//   [7 .. 12], [13 .. 18], [19 .. 24]  the blend's quintics of x, y and psi: q0, V0, A0 / 2, k3, k4, k5
constexpr int GAIT_KNOT_ROWS = 25;
constexpr int GAIT_MAX_SWITCHES = 7;
constexpr int GAIT_SCHEDULE_ROWS = GAIT_MAX_SWITCHES * GAIT_KNOT_ROWS;

// the quintic's six coefficients from value, V = beta q' and A = beta^2 q'' at its two ends
WBC_HD void gait_quintic(double q0, double V0, double A0, double q1, double V1, double A1, double* k, size_t ld) {
  const double D = q1 - q0 - V0 - 0.5 * A0, DV = V1 - V0 - A0, DA = A1 - A0;
  k[0] = q0; k[ld] = V0; k[2 * ld] = 0.5 * A0;
  k[3 * ld] = 10.0 * D - 4.0 * DV + 0.5 * DA;
  k[4 * ld] = 7.0 * DV - 15.0 * D - DA;
  k[5 * ld] = 6.0 * D - 3.0 * DV + 0.5 * DA;
}

// One instance's m switches -> its rows.  when and cmds point at the instance's column of when [7][ld] and cmds [21][ld] (rows from m
// on are not read), knots at its column of the buffer, whose leading dimension is ldk.
WBC_HD void gait_schedule_resolve(const GaitIn& in, double beta, int m, const double* when, const double* cmds, size_t ld, double* knots,
                                  size_t ldk) {
  bool bad = m > GAIT_MAX_SWITCHES;
  GaitIn seg = in;               // the arc of the segment before the switch: its start and command
  double org = 0.0;              // ... and the path parameter at which it starts
  double least = 0.0;            // what the next Theta must reach
  WBC_GAIT_UNROLL
  for (int j = 0; j < GAIT_MAX_SWITCHES; j++) {
    double* k = knots + (size_t)(j * GAIT_KNOT_ROWS) * ldk;
    if (j < m) {
      const double Th = when[(size_t)j * ld];
      const double cx = cmds[(size_t)(3 * j) * ld], cy = cmds[(size_t)(3 * j + 1) * ld], w = cmds[(size_t)(3 * j + 2) * ld];
      bad |= not_finite(Th) | not_finite(cx) | not_finite(cy) | not_finite(w) | !(Th >= least);
      least = Th + beta;
      double xE, yE, cE, sE, sS, cS;
      const double tl = Th - org;
      gait_pose(seg, tl, xE, yE, cE, sE);
      const double psiE = seg.psi0 + seg.w * tl;
      const double psiS = psiE + beta * (0.5 * (seg.w + w));
      wbc_sincos(psiS, sS, cS);
      const double ux = cE * seg.cx - sE * seg.cy, uy = sE * seg.cx + cE * seg.cy;   // Rz(psi_E) c_j-1
      const double vx = cS * cx - sS * cy, vy = sS * cx + cS * cy;                   // Rz(psi_S) c_j
      const double xS = xE + (0.5 * beta) * (ux + vx), yS = yE + (0.5 * beta) * (uy + vy);
      const double bb = beta * beta;
      k[0] = Th; k[ldk] = xS; k[2 * ldk] = yS; k[3 * ldk] = psiS; k[4 * ldk] = cx; k[5 * ldk] = cy; k[6 * ldk] = w;
      gait_quintic(xE, beta * ux, bb * (0.0 - seg.w * uy), xS, beta * vx, bb * (0.0 - w * vy), k + 7 * ldk, ldk);
      gait_quintic(yE, beta * uy, bb * (seg.w * ux), yS, beta * vy, bb * (w * vx), k + 13 * ldk, ldk);
      gait_quintic(psiE, beta * seg.w, 0.0, psiS, beta * w, 0.0, k + 19 * ldk, ldk);
      seg.x0 = xS; seg.y0 = yS; seg.psi0 = psiS; seg.cx = cx; seg.cy = cy; seg.w = w;
      org = least;
    } else {
      k[0] = INFINITY;
      WBC_GAIT_UNROLL
      for (int r = 1; r < GAIT_KNOT_ROWS; r++) k[(size_t)r * ldk] = 0.0;
    }
  }
  if (bad) knots[0] = __builtin_nan("");
}

struct GaitSchedule {   // what an instance's pose evaluations share
  const double* knots;  // the instance's column of the buffer
  size_t ld;
  double beta;
  double when[GAIT_MAX_SWITCHES];
  bool bad;
};
WBC_HD GaitSchedule gait_schedule_load(const double* knots, size_t ld, size_t i, double beta) {
  GaitSchedule S;
  S.knots = knots + i; S.ld = ld; S.beta = beta;
  WBC_GAIT_UNROLL
  for (int j = 0; j < GAIT_MAX_SWITCHES; j++) S.when[j] = S.knots[(size_t)(j * GAIT_KNOT_ROWS) * ld];
  S.bad = S.when[0] != S.when[0];
  return S;
}

struct GaitSegment {    // where a pose evaluation fell, for the body rows
  GaitIn a;             // the segment's arc as an instance: its start and its command
  double tl;            // ... and the arc parameter
  bool blend;           // inside a blend window: psi and the theta-derivatives below hold
  double psi, dx, dy, dpsi, ddx, ddy, ddpsi;
};

// q(u) of a quintic in the buffer (and, RATES, its first and second derivative in u)
template <bool RATES>
WBC_HD void gait_quintic_at(const double* k, size_t ld, double u, double& q, double& qd, double& qdd) {
  const double k0 = k[0], k1 = k[ld], k2 = k[2 * ld], k3 = k[3 * ld], k4 = k[4 * ld], k5 = k[5 * ld];
  q = k0 + u * (k1 + u * (k2 + u * (k3 + u * (k4 + u * k5))));
  if constexpr (RATES) {
    qd = k1 + u * (2.0 * k2 + u * (3.0 * k3 + u * (4.0 * k4 + u * (5.0 * k5))));
    qdd = 2.0 * k2 + u * (6.0 * k3 + u * (12.0 * k4 + u * (20.0 * k5)));
  }
}

// a b + c d where the instantiations under a schedule owe the plain ones' bits (wbc_gait_schedule.h, "Exact relation").  The device
// build contracts such a sum into one fused multiply-add, and which of the two products it fuses follows the order the optimiser
// left the operands in, kernel by kernel: under a schedule, where the yaw's sine and cosine arrive through the blend's branch, it
// left them the other way round.  So there the choice is written down -- the plain kernels': a b fused, c d rounded.  (On the
// host nothing is contracted, and the sum is the plain text.)  tests/test_gait_schedule_gpu.py holds the relation on the device.
WBC_HD double gait_pinned_dot2(double a, double b, double c, double d) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_fma(a, b, c * d);
#else
  return a * b + c * d;
#endif
}

// gait_pose under a schedule: P(th).  Before Theta_1 it is gait_pose(in, th) itself, on the same bits.
template <bool RATES>
WBC_HD void gait_schedule_pose(const GaitIn& in, const GaitSchedule& S, double th, double& x, double& y, double& cpsi, double& spsi,
                               GaitSegment* seg) {
  int s = 0;
  WBC_GAIT_UNROLL
  for (int j = 0; j < GAIT_MAX_SWITCHES; j++) s += (th >= S.when[j]) ? 1 : 0;
  const bool first = s == 0;
  const double* k = S.knots + (size_t)((first ? 0 : s - 1) * GAIT_KNOT_ROWS) * S.ld;
  const double Th = k[0];
  GaitIn a = in;
  a.x0 = first ? in.x0 : k[S.ld]; a.y0 = first ? in.y0 : k[2 * S.ld]; a.psi0 = first ? in.psi0 : k[3 * S.ld];
  a.cx = first ? in.cx : k[4 * S.ld]; a.cy = first ? in.cy : k[5 * S.ld]; a.w = first ? in.w : k[6 * S.ld];
  const double d = th - Th;
  const double tl = first ? th : d - S.beta;
  const bool blend = !first & (d < S.beta);
  gait_pose(a, tl, x, y, cpsi, spsi);
  if constexpr (RATES) { seg->a = a; seg->tl = tl; seg->blend = blend; }
  if (blend) {
    const double u = d / S.beta;
    double psi, r1, r2, r3, r4, r5, r6;
    gait_quintic_at<RATES>(k + 7 * S.ld, S.ld, u, x, r1, r2);
    gait_quintic_at<RATES>(k + 13 * S.ld, S.ld, u, y, r3, r4);
    gait_quintic_at<RATES>(k + 19 * S.ld, S.ld, u, psi, r5, r6);
    wbc_sincos(psi, spsi, cpsi);
    if constexpr (RATES) {
      const double ib = 1.0 / S.beta, ibb = ib * ib;
      seg->psi = psi;
      seg->dx = r1 * ib; seg->ddx = r2 * ibb;
      seg->dy = r3 * ib; seg->ddy = r4 * ibb;
      seg->dpsi = r5 * ib; seg->ddpsi = r6 * ibb;
    }
  }
}

// what the body rows take from a pose evaluation: under a schedule the segment's, otherwise the instance's own
template <bool SCHEDULE> WBC_HD const GaitIn& gait_arc(const GaitSegment& g, const GaitIn& in) {
  if constexpr (SCHEDULE) return g.a;
  else return in;
}
template <bool SCHEDULE> WBC_HD double gait_arc(const GaitSegment& g, double th) {
  if constexpr (SCHEDULE) return g.tl;
  else return th;
}

// the 18 body rows.  TERRAIN: ter the terrain table and gr[3 f + d] the ground height under foot f (d = 0) and its first and second
// time derivatives, as gait_foot hands them out.  SCHEDULE: S the instance's schedule.
template <bool TERRAIN = false, bool SCHEDULE = false>
WBC_HD void gait_body(const double* table, const GaitIn& in, const GaitClock& c, double* b, const double* ter = nullptr,
                      const double* gr = nullptr, const GaitSchedule* S = nullptr) {
  double th, thd, thdd, x, y, cp, sp;
  gait_theta(table[10], c.pre ? 0.0 : c.tau, th, thd, thdd);
  th = c.pre ? 0.0 : th; thd = c.pre ? 0.0 : thd; thdd = c.pre ? 0.0 : thdd;
  [[maybe_unused]] GaitSegment g;
  if constexpr (SCHEDULE) gait_schedule_pose<true>(in, *S, th, x, y, cp, sp, &g);
  else gait_pose(in, th, x, y, cp, sp);
  const GaitIn& e = gait_arc<SCHEDULE>(g, in);          // the arc the pose lies on, and its parameter: without a schedule, in and th
  const double tl = gait_arc<SCHEDULE>(g, th);
  const double vx = cp * e.cx - sp * e.cy, vy = sp * e.cx + cp * e.cy;   // Rz(psi) c
  const double cen = thd * thd * e.w;
  const double nan = __builtin_nan("");
  b[0] = x; b[1] = y; b[2] = table[8];
  b[3] = thd * vx; b[4] = thd * vy; b[5] = 0.0;
  b[6] = thdd * vx - cen * vy; b[7] = thdd * vy + cen * vx; b[8] = 0.0;
  b[9] = 0.0; b[10] = 0.0; b[11] = e.psi0 + e.w * tl;
  b[12] = 0.0; b[13] = 0.0; b[14] = e.w * thd;
  b[15] = 0.0; b[16] = 0.0; b[17] = e.w * thdd;
  if constexpr (SCHEDULE) {                              // inside a blend window: the chain rule on the quintics
    const double tt = thd * thd;
    b[3] = g.blend ? thd * g.dx : b[3]; b[4] = g.blend ? thd * g.dy : b[4];
    b[6] = g.blend ? thdd * g.dx + tt * g.ddx : b[6]; b[7] = g.blend ? thdd * g.dy + tt * g.ddy : b[7];
    b[11] = g.blend ? g.psi : b[11]; b[14] = g.blend ? thd * g.dpsi : b[14]; b[17] = g.blend ? thdd * g.dpsi + tt * g.ddpsi : b[17];
  }
  if constexpr (TERRAIN) {
    double m[3], P[3], Q[3];
    WBC_GAIT_UNROLL
    for (int d = 0; d < 3; d++) {
      m[d] = 0.25 * ((gr[d] + gr[3 + d]) + (gr[6 + d] + gr[9 + d]));
      P[d] = (ter[4] * gr[d] + ter[5] * gr[3 + d]) + (ter[6] * gr[6 + d] + ter[7] * gr[9 + d]);
      Q[d] = (ter[8] * gr[d] + ter[9] * gr[3 + d]) + (ter[10] * gr[6 + d] + ter[11] * gr[9 + d]);
    }
    const double p1 = 1.0 + P[0] * P[0], q1 = 1.0 + Q[0] * Q[0];
    b[2] = table[8] + m[0]; b[5] = m[1]; b[8] = m[2];
    b[9] = atan(Q[0]); b[10] = 0.0 - atan(P[0]);
    b[12] = Q[1] / q1; b[13] = 0.0 - P[1] / p1;
    b[15] = (Q[2] * q1 - 2.0 * Q[0] * (Q[1] * Q[1])) / (q1 * q1);
    b[16] = 0.0 - (P[2] * p1 - 2.0 * P[0] * (P[1] * P[1])) / (p1 * p1);
  }
  WBC_GAIT_UNROLL
  for (int r = 0; r < 18; r++) b[r] = c.bad ? nan : b[r];
}

// the 9 rows of foot f; run (optional, for the tests): the start a of the run the foot is in, and u = (tau - a) / D as the rows use it.
// TERRAIN: ter the terrain table, G the instance's ground; gr[3] <- the ground height under the foot and its two time derivatives.
// SCHEDULE: S the instance's schedule.
template <bool TERRAIN = false, bool SCHEDULE = false>
WBC_HD void gait_foot(const double* table, const GaitIn& in, const GaitClock& c, int f, double* o, double* run = nullptr,
                      const double* ter = nullptr, const GaitGround* G = nullptr, double* gr = nullptr, const GaitSchedule* S = nullptr) {
  const double* e = c.stride + 12 + 6 * (8 * f + c.phase);
  const double sx = table[2 * f], sy = table[2 * f + 1], ramp = table[10];
  double a, b, pa, pb, na, nb;
  {
    WBC_GAIT_NO_CONTRACT
    a = c.kT + c.s * e[0]; b = c.kT + c.s * e[1];
    pa = c.kT + c.s * e[2]; pb = c.kT + c.s * e[3];
    na = c.kT + c.s * e[4]; nb = c.kT + c.s * e[5];
  }
  const bool swing = !((c.mask >> f) & 1u);
  // the two footholds: of the stance run before and after a swing run; a stance run's own, twice
  double F[2][2];
  [[maybe_unused]] double Fs[2], Fz[2];
  WBC_GAIT_UNROLL
  for (int h = 0; h < 2; h++) {
    const double lo = h ? na : pa, hi = h ? nb : pb;
    double th, thd, thdd, x, y, cp, sp;
    gait_theta(ramp, fmax(0.5 * (lo + hi), 0.0), th, thd, thdd);
    th = (c.pre | (lo <= 0.0)) ? 0.0 : th;
    if constexpr (SCHEDULE) gait_schedule_pose<false>(in, *S, th, x, y, cp, sp, nullptr);
    else gait_pose(in, th, x, y, cp, sp);
    F[h][0] = x + (cp * sx - sp * sy);
    if constexpr (SCHEDULE) F[h][1] = y + gait_pinned_dot2(sp, sx, cp, sy);
    else F[h][1] = y + (sp * sx + cp * sy);
    if constexpr (TERRAIN) gait_foothold_on(ter, *G, c.pre | (lo <= 0.0), F[h][0], F[h][1], Fs[h], Fz[h]);
  }
  const double D = b - a, u = (c.tau - a) / D, w = 1.0 - u, uw = u * w;
  if (run) { run[0] = a; run[1] = u; }
  const double sg = (u * u) * u * (10.0 + u * (6.0 * u - 15.0));
  const double sgd = 30.0 * (uw * uw) / D, sgdd = 60.0 * uw * (1.0 - 2.0 * u) / (D * D);
  double apex = table[9];
  if constexpr (TERRAIN) apex = gait_apex(ter, *G, table[9], Fs[0], Fz[0], Fs[1], Fz[1]);
  const double hz = apex * 64.0;
  const double z = hz * (uw * uw) * uw, zd = hz * 3.0 * (uw * uw) * (1.0 - 2.0 * u) / D;
  const double zdd = hz * 6.0 * uw * (1.0 + 5.0 * u * (u - 1.0)) / (D * D);
  const double dx = F[1][0] - F[0][0], dy = F[1][1] - F[0][1];
  const double nan = __builtin_nan("");
  o[0] = swing ? F[0][0] + dx * sg : F[0][0];
  o[1] = swing ? F[0][1] + dy * sg : F[0][1];
  o[2] = swing ? z : 0.0;
  o[3] = swing ? dx * sgd : 0.0;
  o[4] = swing ? dy * sgd : 0.0;
  o[5] = swing ? zd : 0.0;
  o[6] = swing ? dx * sgdd : 0.0;
  o[7] = swing ? dy * sgdd : 0.0;
  o[8] = swing ? zdd : 0.0;
  if constexpr (TERRAIN) {
    const double dz = Fz[1] - Fz[0];
    gr[0] = swing ? Fz[0] + dz * sg : Fz[0];
    gr[1] = swing ? dz * sgd : 0.0;
    gr[2] = swing ? dz * sgdd : 0.0;
    o[2] = swing ? gr[0] + z : Fz[0];
    o[5] = swing ? gr[1] + zd : 0.0;
    o[8] = swing ? gr[2] + zdd : 0.0;
  }
  WBC_GAIT_UNROLL
  for (int r = 0; r < 9; r++) o[r] = c.bad ? nan : o[r];
}

// instance i of a batch: the inputs as wbc_gait_set_commands takes them (null optional pointers: their defaults)
WBC_HD GaitIn gait_load(const double* time, const double* cmd, const uint8_t* gait_id, const double* stride_scale, const double* start,
                        size_t ld, size_t i) {
  GaitIn in;
  in.time = time[i];
  in.cx = cmd[i]; in.cy = cmd[ld + i]; in.w = cmd[2 * ld + i];
  in.id = gait_id ? (int)gait_id[i] : 0;
  in.s = stride_scale ? stride_scale[i] : 1.0;
  in.x0 = start ? start[i] : 0.0; in.y0 = start ? start[ld + i] : 0.0; in.psi0 = start ? start[2 * ld + i] : 0.0;
  return in;
}

}  // namespace wbc
