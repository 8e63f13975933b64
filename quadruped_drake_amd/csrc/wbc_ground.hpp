// wbc_ground.hpp -- per-robot math of the compliant-ground plant (include/wbc_ground.h; product code).
//
// Forward dynamics of the quadruped under applied torques on a compliant half-space z = 0.  The ground force on a foot is an
// explicit function of the state (Hunt-Crossley normal force, regularised Coulomb friction), so there is no constraint:
//     M vd + Cv + tau_g = S' tau_a + w_ext + sum_c J_c' f_c(q, v)
// and the arrowhead elimination of wbc_plant.hpp stops after the base Schur solve (no Y / Z columns, no 12x12 contact operator):
//   S   = M_bb - sum_l B_l D_l^-1 B_l'                                 (6x6, Cholesky L L')
//   y_l = tau_a,l - h_l + J_l,leg' f_l
//   rho = -h_b + w_ext + sum_l ([rf_l x f_l; f_l] - B_l D_l^-1 y_l)
//   vd_b = S^-1 rho,   vd_l = D_l^-1 (y_l - B_l' vd_b)
// The force law, per foot with world position p and velocity pd (this project's definition, unpinned at Drake):
//   phi = foot_radius - p_z;   phi <= 0: f = 0 exactly;   otherwise
//   f_n = k phi max(0, 1 - d pd_z),   f_t = -mu_p f_n (pd_x, pd_y) / max(|(pd_x, pd_y)|, v_s),   f = (f_t, f_n).
// With a terrain (TERRAIN instantiations, further down) the same law is written about the normal n of the terrain segment under the
// foot: phi = radius - (p_z - H) n_z, v_n = pd . n, f = f_n n - mu_p f_n v_t / max(|v_t|, v_s) with v_t = pd - v_n n.
//
// One leg per call, as wbc_plant.hpp: the device kernel runs ground_leg_phase on the leg's own lane of a quad, tools/host_ground.cpp
// one leg after the other.  Kinematics, composite inertia and Newton-Euler come from wbc_tick.hpp, the base share, the Cholesky
// routines, the leg's final solve and the integrator from wbc_plant.hpp, all unchanged.
#pragma once
#include <math.h>
#include "wbc_plant.hpp"

namespace wbc {

enum { GROUND_SLIP = 1, GROUND_FELL = 2, GROUND_CLIP = 4, GROUND_BAD = 8 };
enum { GROUND_FOOT_TOUCH = 1, GROUND_FOOT_SLIP = 2 };   // what ground_foot_force returns
constexpr double GROUND_DELTA = 1e-3;          // static penetration of the default stiffness: k = weight / delta  [m]
constexpr double GROUND_V_STICTION = 0.05;     // default v_s  [m/s]
constexpr double GROUND_MAX_SUBSTEP = 6.25e-5; // default longest explicit substep  [s]

template <class T> struct GroundLaw {
  T k, d, vs, radius;   // stiffness [N/m], Hunt-Crossley dissipation [s/m], friction regularisation speed [m/s], foot radius [m]
};

// default stiffness and dissipation of a model: its weight at s_p = 1 carried at GROUND_DELTA of penetration, d = 1 / sqrt(g delta)
inline void ground_default_law(const ModelC& m, double* k, double* d) {
  *k = plant_weight<double>(m, 1.0) / GROUND_DELTA;
  *d = 1.0 / sqrt(m.gravity * GROUND_DELTA);
}

// Number of explicit substeps of a control period: ceil(dt / max_substep), with one part in 1e12 of slack so that a dt that is
// a whole multiple of max_substep up to rounding gets that multiple.  0: not answerable.
inline int ground_substeps(double dt, double max_substep) {
  if (!(dt > 0.0) || !(max_substep > 0.0)) return 1;
  const double s = ceil(dt / max_substep * (1.0 - 1e-12));
  if (!(s <= 1048576.0)) return 0;
  return s < 1.0 ? 1 : (int)s;
}

// Ground force on one foot from its height and velocity.  Returns GROUND_FOOT_TOUCH when phi > 0 and GROUND_FOOT_SLIP when the foot
// is loaded (f_n > 0) and slides faster than v_s.
template <class T> WBC_HD int ground_foot_force(const GroundLaw<T>& g, T mu, T pz, const T* pd, T* f) {
  const T phi = g.radius - pz;
  const bool touch = phi > T(0.0);
  const T damp = T(1.0) - g.d * pd[2];
  const T fn = (touch && damp > T(0.0)) ? g.k * phi * damp : T(0.0);
  const T vt = sqrt(pd[0] * pd[0] + pd[1] * pd[1]);
  const T sc = mu * fn / (vt > g.vs ? vt : g.vs);
  const bool loaded = fn > T(0.0);
  f[0] = loaded ? T(0.0) - sc * pd[0] : T(0.0);
  f[1] = loaded ? T(0.0) - sc * pd[1] : T(0.0);
  f[2] = fn;
  return (touch ? GROUND_FOOT_TOUCH : 0) | ((loaded && vt > g.vs) ? GROUND_FOOT_SLIP : 0);
}

// ---- terrain (include/wbc_ground.h): H(x, y) = scale h(s), s = (x - x0) cos psi + (y - y0) sin psi, h piecewise linear.
// A profile is packed once into TERRAIN_STRIDE doubles, so that the force law reads what it needs and computes no division:
//   [0] cos psi  [1] sin psi  [2] x0  [3] y0   [4 .. 11] the knots s_k, +inf beyond nk
//   [12 + 3 j ..], j = 0 .. 8: (s_start, h_start, slope) of the piece that holds the feet with j knots at or below their s:
//   j = 0 the level ground before the first knot, j = nk the level ground after the last, in between segment j - 1.
// The device kernels stage the table of all profiles in LDS once per launch; the host tool reads it from plain memory.
constexpr int TERRAIN_MAX_KNOTS = 8, TERRAIN_MAX_PROFILES = 16, TERRAIN_STRIDE = 40;

// what wbc_terrain_check refuses in one profile (nullptr: nothing)
inline const char* terrain_profile_error(int nk, double x0, double y0, double yaw, const double* s, const double* h) {
  if (nk < 1 || nk > TERRAIN_MAX_KNOTS) return "nk must be 1 .. 8";
  if (not_finite(x0) || not_finite(y0) || not_finite(yaw)) return "x0, y0 and yaw must be finite";
  for (int k = 0; k < nk; k++)
    if (not_finite(s[k]) || not_finite(h[k])) return "every knot must be finite";
  for (int k = 1; k < nk; k++)
    if (!(s[k] > s[k - 1])) return "the knots' s must be strictly increasing";
  return nullptr;
}

inline void terrain_pack(int nk, double x0, double y0, double yaw, const double* s, const double* h, double* out) {
  out[0] = cos(yaw); out[1] = sin(yaw); out[2] = x0; out[3] = y0;
  for (int k = 0; k < TERRAIN_MAX_KNOTS; k++) out[4 + k] = k < nk ? s[k] : INFINITY;
  for (int j = 0; j <= TERRAIN_MAX_KNOTS; j++) {
    const int a = j == 0 ? 0 : (j > nk ? nk : j) - 1;                     // the knot the piece starts from
    const bool ramp = j >= 1 && j < nk;
    out[12 + 3 * j] = s[a];
    out[12 + 3 * j + 1] = h[a];
    out[12 + 3 * j + 2] = ramp ? (h[j] - h[j - 1]) / (s[j] - s[j - 1]) : 0.0;
  }
  out[39] = 0.0;
}

// Height H and slope g (both scaled) of the packed profile `tab` under the world point (x, y).
template <class T> WBC_HD void terrain_surface(const T* tab, T scale, T x, T y, T& H, T& g) {
  const T s = (x - tab[2]) * tab[0] + (y - tab[3]) * tab[1];
  int j = 0;
  WBC_PLANT_UNROLL
  for (int k = 0; k < TERRAIN_MAX_KNOTS; k++) j += (s >= tab[4 + k]) ? 1 : 0;
  const T* seg = tab + 12 + 3 * j;
  H = scale * (seg[1] + seg[2] * (s - seg[0]));
  g = scale * seg[2];
}

// ground_foot_force about the normal of the terrain segment under the foot at world position p.
template <class T>
WBC_HD int ground_foot_force_terrain(const GroundLaw<T>& g, T mu, const T* tab, T scale, const T* p, const T* pd, T* f) {
  T H, gs;
  terrain_surface(tab, scale, p[0], p[1], H, gs);
  const T nz = T(1.0) / sqrt(T(1.0) + gs * gs);
  const T n[3] = {T(0.0) - gs * tab[0] * nz, T(0.0) - gs * tab[1] * nz, nz};
  const T phi = g.radius - (p[2] - H) * nz;
  const bool touch = phi > T(0.0);
  const T vn = pd[0] * n[0] + pd[1] * n[1] + pd[2] * n[2];
  const T damp = T(1.0) - g.d * vn;
  const T fn = (touch && damp > T(0.0)) ? g.k * phi * damp : T(0.0);
  const T t[3] = {pd[0] - vn * n[0], pd[1] - vn * n[1], pd[2] - vn * n[2]};
  const T vt = sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
  const T sc = mu * fn / (vt > g.vs ? vt : g.vs);
  const bool loaded = fn > T(0.0);
  WBC_PLANT_UNROLL
  for (int i = 0; i < 3; i++) f[i] = loaded ? fn * n[i] - sc * t[i] : T(0.0);
  return (touch ? GROUND_FOOT_TOUCH : 0) | ((loaded && vt > g.vs) ? GROUND_FOOT_SLIP : 0);
}

// FELL: the trunk origin qb[4 .. 6] at or below the ground under it plus fall_height.
template <bool TERRAIN, class T> WBC_HD bool ground_fell(const T* qb, T fall_height, const T* tab, T scale) {
  if (!TERRAIN) return !(qb[6] > fall_height);
  T H, gs;
  terrain_surface(tab, scale, qb[4], qb[5], H, gs);
  return !(qb[6] > H + fall_height);
}

// One leg at the substep's start state: kinematics, CRBA, RNEA, D^-1, the foot's ground force f3 and the leg's shares of S and rho
// (L.s).  L.r = tau_a,l - h_l as in the plant (plant_leg_final adds J_l,leg' f); L.bc is not used.  pz0 = base height (world),
// th / qd / tau3: own joints in canonical order, tau3 already clipped.  Returns ground_foot_force's bits.
// TERRAIN: px0, py0 = the base's world x, y and tab / scale the instance's packed profile and scale; unused otherwise.
template <bool TERRAIN = false, class T>
WBC_HD int ground_leg_phase(const ModelC& m, int l, const T* R0, const T* w0, const T* v0, T pz0, const T* th, const T* qd,
                            const T* tau3, const GroundLaw<T>& g, T mu, PlantLeg<T>& L, T* f3, T px0 = T(0.0), T py0 = T(0.0),
                            const T* tab = nullptr, T scale = T(1.0)) {
  T sn[3], cs[3];
  WBC_PLANT_UNROLL
  for (int k = 0; k < 3; k++) wbc_sincos(th[k], sn[k], cs[k]);
  LegKin<T> K;
  leg_fk_xyy(m, l, R0, sn, cs, K);
  const T mass3[3] = {T(m.link[l][0].mass), T(m.link[l][1].mass), T(m.link[l][2].mass)};
  LegDyn<T> D;
  T lm = T(0.0), lh[3] = {T(0.0), T(0.0), T(0.0)}, lI[6] = {T(0.0), T(0.0), T(0.0), T(0.0), T(0.0), T(0.0)};
  leg_crba(mass3, K, D, lm, lh, lI);
  WBC_PLANT_UNROLL
  for (int i = 0; i < 3; i++) L.rf[i] = K.rf(i);
  WBC_PLANT_UNROLL
  for (int k = 0; k < 3; k++) {
    const T d[3] = {L.rf[0] - K.r(k, 0), L.rf[1] - K.r(k, 1), L.rf[2] - K.r(k, 2)};
    const T axv[3] = {K.ax(k, 0), K.ax(k, 1), K.ax(k, 2)};
    T c[3];
    cross(axv, d, c);
    WBC_PLANT_UNROLL
    for (int i = 0; i < 3; i++) L.Jl[3 * i + k] = c[i];
  }
  T hl[3], Nb[3], Fb[3];
  leg_rnea<T, false>(mass3, K, w0, qd, T(m.gravity), hl, Nb, Fb, (LegDyn<T>*)nullptr);
  {
    T Mf[9];
    sym_to_full(D.Mll, Mf);
    inv3(Mf, L.Di);
  }
  WBC_PLANT_UNROLL
  for (int i = 0; i < 18; i++) L.B[i] = D.Mbl[i];
  // foot velocity v0 + w0 x rf + Jl qd, then the ground force
  T t[3], pd[3];
  cross(w0, L.rf, t);
  WBC_PLANT_UNROLL
  for (int i = 0; i < 3; i++) pd[i] = v0[i] + (t[i] + (L.Jl[3 * i] * qd[0] + L.Jl[3 * i + 1] * qd[1] + L.Jl[3 * i + 2] * qd[2]));
  int bits;
  if constexpr (TERRAIN) {
    const T p[3] = {px0 + L.rf[0], py0 + L.rf[1], pz0 + L.rf[2]};
    bits = ground_foot_force_terrain(g, mu, tab, scale, p, pd, f3);
  } else {
    bits = ground_foot_force(g, mu, pz0 + L.rf[2], pd, f3);
  }
  T y[3];   // tau_a,l - h_l + Jl' f
  WBC_PLANT_UNROLL
  for (int k = 0; k < 3; k++) {
    L.r[k] = tau3[k] - hl[k];
    L.bc[k] = T(0.0);
    y[k] = L.r[k] + (L.Jl[k] * f3[0] + L.Jl[3 + k] * f3[1] + L.Jl[6 + k] * f3[2]);
  }
  T BD[18];   // B D^-1
  WBC_PLANT_UNROLL
  for (int i = 0; i < 6; i++)
    WBC_PLANT_UNROLL
    for (int j = 0; j < 3; j++) BD[3 * i + j] = L.B[3 * i] * L.Di[j] + L.B[3 * i + 1] * L.Di[3 + j] + L.B[3 * i + 2] * L.Di[6 + j];
  WBC_PLANT_UNROLL
  for (int i = 0; i < 6; i++)
    WBC_PLANT_UNROLL
    for (int j = 0; j <= i; j++)
      L.s[sp(i, j)] = spatial_inertia(i, j, lm, lh, lI) - (BD[3 * i] * L.B[3 * j] + BD[3 * i + 1] * L.B[3 * j + 1] + BD[3 * i + 2] * L.B[3 * j + 2]);
  // base rows of J_c' f: [rf x f; f]
  T rxf[3];
  cross(L.rf, f3, rxf);
  const T hbN[6] = {Nb[0], Nb[1], Nb[2], Fb[0], Fb[1], Fb[2]};
  const T jf[6] = {rxf[0], rxf[1], rxf[2], f3[0], f3[1], f3[2]};
  WBC_PLANT_UNROLL
  for (int i = 0; i < 6; i++) L.s[21 + i] = (jf[i] - hbN[i]) - (BD[3 * i] * y[0] + BD[3 * i + 1] * y[1] + BD[3 * i + 2] * y[2]);
  return bits;
}

// The base solve once S (21, packed) and rho (6) are summed in s27: vd_b = S^-1 rho.  s27[0..20] is overwritten by the factor.
template <class T> WBC_HD void ground_base_solve(T* s27, T* vdb) {
  T rinv[6], piv[6];
  plant_chol<T, 6>(s27, rinv, piv);
  WBC_PLANT_UNROLL
  for (int k = 0; k < 6; k++) vdb[k] = s27[21 + k];
  plant_fwd<T, 6>(s27, rinv, vdb);
  plant_bwd<T, 6>(s27, rinv, vdb);
}

}  // namespace wbc
