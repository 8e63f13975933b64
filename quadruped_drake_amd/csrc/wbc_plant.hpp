// wbc_plant.hpp -- per-robot math of the rigid-contact plant step (include/wbc_plant.h; product code).
//
// Forward dynamics of the quadruped under applied torques with the stance feet held by bilateral contacts:
//     M vd + Cv + tau_g = S' tau_a + sum_{c in mask} J_c' f_c ,     J_c vd + Jdot_c v = -Kd J_c v   (c in mask)
// solved WITHOUT a dense 18x18 matrix.  M is an arrowhead: a 6x6 base block, four 3x3 leg blocks D_l and couplings B_l (6x3).
//   S      = M_bb - sum_l B_l D_l^-1 B_l'                         (6x6 base Schur complement, Cholesky L L')
//   M^-1 g : x_b = S^-1 (g_b - sum_l B_l D_l^-1 g_l),  x_l = D_l^-1 (g_l - B_l' x_b)
//   Y_c    = J_c,base' - B_c D_c^-1 J_c,leg'  (6x3),  Z_c = L^-1 Y_c
//   Lambda^-1 = blockdiag_c(J_c,leg D_c^-1 J_c,leg') + Z' Z        (<= 12x12, SPD, Cholesky; swing rows are identity rows)
//   f      = Lambda (bc - J a0),  a0 = M^-1 (S' tau_a - Cv - tau_g)
//   vd     : x_b = a0_b + L'^-1 sum_c Z_c f_c,  x_l = D_l^-1 (tau_a,l - h_l + J_l,leg' f_l - B_l' x_b)
// The base columns keep J_c at full row rank with a straight stance knee (the tick's status 2), so the plant still answers there.
//
// The phases below are what one leg computes (the device kernel runs each on the leg's own lane of a quad) and what the four
// legs share (replicated on the quad).  Templated on the scalar like wbc_tick.hpp so that tools/host_plant.cpp can run them on
// the host for the CPU tests.  Per-leg kinematics, composite inertia and Newton-Euler come from wbc_tick.hpp, unchanged.
#pragma once
#include <math.h>
#include "wbc_tick.hpp"
#include "wbc_model.hpp"

#if defined(__HIPCC__)
#define WBC_PLANT_UNROLL _Pragma("unroll")
#else
#define WBC_PLANT_UNROLL
#endif

namespace wbc {

enum { PLANT_PULL = 1, PLANT_CONE = 2, PLANT_CLIP = 4, PLANT_BAD = 8 };
constexpr double PLANT_PIVOT_REL = 1e-12;   // a contact-system pivot below this fraction of the largest one: BAD
constexpr double PLANT_FORCE_TOL = 1e-9;    // PULL / CONE slack, relative to the instance's total |f| + its weight
constexpr double PLANT_CLIP_TOL = 1e-9;     // CLIP: |tau| > tau_max (1 + this)

// packed lower triangle of a symmetric matrix
WBC_HD constexpr int sp(int i, int j) { return (i >= j) ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i; }

// What one leg contributes.  Base rows are [angular; linear] about the base origin, world-aligned (wbc_tick.hpp).
template <class T> struct PlantLeg {
  T B[18];    // M_bl: 6x3 row-major, columns = own joints
  T Di[9];    // D_l^-1 (D_l = M_ll), 3x3
  T Jl[9];    // d(foot velocity) / d(own joint rates)
  T rf[3];    // foot position relative to the base origin
  T r[3];     // tau_a,l - h_l: applied minus bias + gravity torques of the own joints
  T bc[3];    // stance row's right-hand side -Kd J v - Jdot v (0 for a swing leg)
  T s[27];    // this leg's share of S (21, packed) and of rho = g_b - sum_l B_l D_l^-1 g_l (6)
};

// 6x6 spatial-inertia entry (i, j) of a composite body (mass m, first moment h, rotational inertia I about the base origin)
template <class T> WBC_HD T spatial_inertia(int i, int j, const T& m, const T* h, const T* I) {
  if (i < j) { const int t = i; i = j; j = t; }
  if (i < 3) return I[(i == j) ? i : (i + j + 2)];   // xx yy zz | xy (1,0) xz (2,0) yz (2,1)
  if (j >= 3) return (i == j) ? m : T(0.0);
  // lower-left block = ([h]x)' : entry (3 + a, b) = [h]x (b, a)
  const int a = i - 3, b = j;
  if (a == b) return T(0.0);
  const int c = 3 - a - b;                          // the remaining axis
  const bool even = ((b + 1) % 3) == a;             // (b, a, c) cyclic
  return even ? T(0.0) - h[c] : h[c];
}

// Rotation of the base from the quaternion: Drake's RotationMatrix(quaternion) scales by 2 / |q|^2 (wbc_hex.hpp)
template <class T> WBC_HD void plant_rotation(const T* qb, T* R0) {
  const T qw = qb[0], qx = qb[1], qy = qb[2], qz = qb[3];
  const T s = T(2.0) / (qw * qw + qx * qx + qy * qy + qz * qz);
  R0[0] = T(1.0) - s * (qy * qy + qz * qz); R0[1] = s * (qx * qy - qw * qz); R0[2] = s * (qx * qz + qw * qy);
  R0[3] = s * (qx * qy + qw * qz); R0[4] = T(1.0) - s * (qx * qx + qz * qz); R0[5] = s * (qy * qz - qw * qx);
  R0[6] = s * (qx * qz - qw * qy); R0[7] = s * (qy * qz + qw * qx); R0[8] = T(1.0) - s * (qx * qx + qy * qy);
}

// Phase 1, one leg: kinematics, CRBA, RNEA, D^-1 and the leg's shares of S and rho.
// th / qd / tau3: own joints in canonical order, tau3 already clipped.
template <class T>
WBC_HD void plant_leg_phase1(const ModelC& m, int l, const T* R0, const T* w0, const T* v0, const T* th, const T* qd,
                             const T* tau3, bool stance, T Kd, PlantLeg<T>& L) {
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
  leg_rnea<T, true>(mass3, K, w0, qd, T(m.gravity), hl, Nb, Fb, &D);
  {
    T Mf[9];
    sym_to_full(D.Mll, Mf);
    inv3(Mf, L.Di);
  }
  WBC_PLANT_UNROLL
  for (int i = 0; i < 18; i++) L.B[i] = D.Mbl[i];
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
  WBC_PLANT_UNROLL
  for (int k = 0; k < 3; k++) L.r[k] = tau3[k] - hl[k];
  const T hbN[6] = {Nb[0], Nb[1], Nb[2], Fb[0], Fb[1], Fb[2]};
  WBC_PLANT_UNROLL
  for (int i = 0; i < 6; i++) L.s[21 + i] = T(0.0) - hbN[i] - (BD[3 * i] * L.r[0] + BD[3 * i + 1] * L.r[1] + BD[3 * i + 2] * L.r[2]);
  // foot velocity v0 + w0 x rf + Jl qd; stance row -Kd J v - Jdot v (as the tick's bc[])
  T t[3];
  cross(w0, L.rf, t);
  WBC_PLANT_UNROLL
  for (int i = 0; i < 3; i++) {
    const T pd = v0[i] + (t[i] + (L.Jl[3 * i] * qd[0] + L.Jl[3 * i + 1] * qd[1] + L.Jl[3 * i + 2] * qd[2]));
    L.bc[i] = stance ? (T(0.0) - Kd * pd - D.Jdv[i]) : T(0.0);
  }
}

// The base's own share of S (21) and of rho (6): trunk mass and inertia scaled by s_p (wbc_step's mass_scale), bias + gravity.
template <class T> WBC_HD void plant_base_share(const ModelC& m, const T* R0, const T* w0, T s_p, T* s27) {
  const T bm = T(m.base_mass) * s_p;
  T bmc[3], bI[6];
  {
    const T t[3] = {T(m.base_mc[0]) * s_p, T(m.base_mc[1]) * s_p, T(m.base_mc[2]) * s_p};
    rotv(R0, t, bmc);
    rot_inertia(R0, m.base_I, bI);
    WBC_PLANT_UNROLL
    for (int i = 0; i < 6; i++) bI[i] = bI[i] * s_p;
  }
  WBC_PLANT_UNROLL
  for (int i = 0; i < 6; i++)
    WBC_PLANT_UNROLL
    for (int j = 0; j <= i; j++) s27[sp(i, j)] = spatial_inertia(i, j, bm, bmc, bI);
  T t2[3], t3[3], Iw_w[3], t4[3];
  const T g3[3] = {T(0.0), T(0.0), T(m.gravity)};
  cross(w0, bmc, t2);
  cross(w0, t2, t2);
  symv(bI, w0, Iw_w);
  cross(w0, Iw_w, t3);
  cross(bmc, g3, t4);
  WBC_PLANT_UNROLL
  for (int i = 0; i < 3; i++) { s27[21 + i] = T(0.0) - (t3[i] + t4[i]); s27[24 + i] = T(0.0) - (bm * g3[i] + t2[i]); }
}

// In-place Cholesky of a packed symmetric N x N matrix: A <- L (lower), rinv[j] = 1 / L_jj, piv[j] = the pivot L_jj^2.
template <class T, int N> WBC_HD void plant_chol(T* A, T* rinv, T* piv) {
  WBC_PLANT_UNROLL
  for (int j = 0; j < N; j++) {
    T d = A[sp(j, j)];
    WBC_PLANT_UNROLL
    for (int k = 0; k < j; k++) d = d - A[sp(j, k)] * A[sp(j, k)];
    piv[j] = d;
    T root, rs;
    fast_sqrt_rsq(d, root, rs);
    A[sp(j, j)] = root;
    rinv[j] = rs;
    WBC_PLANT_UNROLL
    for (int i = j + 1; i < N; i++) {
      T x = A[sp(i, j)];
      WBC_PLANT_UNROLL
      for (int k = 0; k < j; k++) x = x - A[sp(i, k)] * A[sp(j, k)];
      A[sp(i, j)] = x * rs;
    }
  }
}
// y <- L^-1 y
template <class T, int N> WBC_HD void plant_fwd(const T* L, const T* rinv, T* y) {
  WBC_PLANT_UNROLL
  for (int i = 0; i < N; i++) {
    T x = y[i];
    WBC_PLANT_UNROLL
    for (int k = 0; k < i; k++) x = x - L[sp(i, k)] * y[k];
    y[i] = x * rinv[i];
  }
}
// y <- L'^-1 y
template <class T, int N> WBC_HD void plant_bwd(const T* L, const T* rinv, T* y) {
  WBC_PLANT_UNROLL
  for (int i = N - 1; i >= 0; i--) {
    T x = y[i];
    WBC_PLANT_UNROLL
    for (int k = i + 1; k < N; k++) x = x - L[sp(k, i)] * y[k];
    y[i] = x * rinv[i];
  }
}

// Phase 2, one leg (after the base solve): the unconstrained joint accelerations a0_l and this leg's part of the contact
// system: Z = L^-1 Y (6x3 row-major), G = Jl D^-1 Jl' (3x3), e = bc - J a0.  A swing leg contributes an identity block.
template <class T>
WBC_HD void plant_leg_phase2(const PlantLeg<T>& L, const T* Lb, const T* rinvb, const T* a0b, bool stance, T* Z, T* G, T* e,
                             T* a0l) {
  T y[3];
  WBC_PLANT_UNROLL
  for (int k = 0; k < 3; k++) {
    T s = L.r[k];
    WBC_PLANT_UNROLL
    for (int i = 0; i < 6; i++) s = s - L.B[3 * i + k] * a0b[i];
    y[k] = s;
  }
  rotv(L.Di, y, a0l);
  T DJ[9];   // D^-1 Jl'
  WBC_PLANT_UNROLL
  for (int i = 0; i < 3; i++)
    WBC_PLANT_UNROLL
    for (int j = 0; j < 3; j++) DJ[3 * i + j] = L.Di[3 * i] * L.Jl[3 * j] + L.Di[3 * i + 1] * L.Jl[3 * j + 1] + L.Di[3 * i + 2] * L.Jl[3 * j + 2];
  // Y = Jb' - B D^-1 Jl';  Jb' f = [rf x f; f]
  const T* rf = L.rf;
  const T JbT[18] = {T(0.0), T(0.0) - rf[2], rf[1], rf[2], T(0.0), T(0.0) - rf[0], T(0.0) - rf[1], rf[0], T(0.0),
                     T(1.0), T(0.0), T(0.0), T(0.0), T(1.0), T(0.0), T(0.0), T(0.0), T(1.0)};
  WBC_PLANT_UNROLL
  for (int j = 0; j < 3; j++) {
    T col[6];
    WBC_PLANT_UNROLL
    for (int i = 0; i < 6; i++) col[i] = JbT[3 * i + j] - (L.B[3 * i] * DJ[j] + L.B[3 * i + 1] * DJ[3 + j] + L.B[3 * i + 2] * DJ[6 + j]);
    plant_fwd<T, 6>(Lb, rinvb, col);
    WBC_PLANT_UNROLL
    for (int i = 0; i < 6; i++) Z[3 * i + j] = stance ? col[i] : T(0.0);
  }
  WBC_PLANT_UNROLL
  for (int i = 0; i < 3; i++)
    WBC_PLANT_UNROLL
    for (int j = 0; j < 3; j++) {
      const T g = L.Jl[3 * i] * DJ[j] + L.Jl[3 * i + 1] * DJ[3 + j] + L.Jl[3 * i + 2] * DJ[6 + j];
      G[3 * i + j] = stance ? g : T(i == j ? 1.0 : 0.0);
    }
  T t[3];
  cross(a0b, rf, t);
  WBC_PLANT_UNROLL
  for (int i = 0; i < 3; i++) {
    const T ja = a0b[3 + i] + (t[i] + (L.Jl[3 * i] * a0l[0] + L.Jl[3 * i + 1] * a0l[1] + L.Jl[3 * i + 2] * a0l[2]));
    e[i] = stance ? L.bc[i] - ja : T(0.0);
  }
}

// Block (c, d) of Lambda^-1: Z_c' Z_d (+ G_c on the diagonal), 3x3 row-major
template <class T> WBC_HD void plant_lambda_block(const T* Zc, const T* Zd, const T* Gc, bool diag, T* blk) {
  WBC_PLANT_UNROLL
  for (int i = 0; i < 3; i++)
    WBC_PLANT_UNROLL
    for (int j = 0; j < 3; j++) {
      T s = diag ? Gc[3 * i + j] : T(0.0);
      WBC_PLANT_UNROLL
      for (int k = 0; k < 6; k++) s = s + Zc[3 * k + i] * Zd[3 * k + j];
      blk[3 * i + j] = s;
    }
}

// The contact forces from the assembled system (packed 12x12 Lambda^-1, overwritten) and e.  Returns false when a stance
// pivot falls below PLANT_PIVOT_REL of the largest stance pivot (or is not a number).
template <class T> WBC_HD bool plant_contact_solve(T* A, const T* e, unsigned mask, T* f) {
  T rinv[12], piv[12];
  plant_chol<T, 12>(A, rinv, piv);
  T pmax = T(0.0), pmin = T(__builtin_huge_val());
  WBC_PLANT_UNROLL
  for (int j = 0; j < 12; j++) {
    const bool st = (mask >> (j / 3)) & 1u;
    const T p = piv[j];
    pmax = (st && p > pmax) ? p : pmax;
    pmin = (st && !(p >= pmin)) ? p : pmin;   // a NaN pivot is kept as the minimum
  }
  WBC_PLANT_UNROLL
  for (int j = 0; j < 12; j++) f[j] = e[j];
  plant_fwd<T, 12>(A, rinv, f);
  plant_bwd<T, 12>(A, rinv, f);
  return pmin >= T(PLANT_PIVOT_REL) * pmax;
}

// The plant robot's weight (trunk scaled by s_p): the force unit of the flag slack
template <class T> WBC_HD T plant_weight(const ModelC& m, T s_p) {
  T w = T(m.base_mass) * s_p;
  for (int l = 0; l < 4; l++)
    for (int k = 0; k < 3; k++) w = w + T(m.link[l][k].mass);
  return w * T(m.gravity);
}

// PULL / CONE bits of the stance feet's forces under the plant's friction mu.  The slack is rounding level of the instance's
// forces, tol = 1e-9 (sum_{c in mask} (|f_x| + |f_y| + |f_z|) + weight): a foot the QP leaves at exactly zero force (a vertex of
// its cone) comes out of the plant as rounding noise of the other feet's -- or, when the QP unloads every foot, of the weight's --
// magnitude, which a per-foot slack would flag.
template <class T> WBC_HD int plant_force_flags(const T* f, unsigned mask, T mu, T weight) {
  T fsum = weight;
  WBC_PLANT_UNROLL
  for (int c = 0; c < 4; c++) fsum = fsum + (((mask >> c) & 1u) ? (wabs(f[3 * c]) + wabs(f[3 * c + 1]) + wabs(f[3 * c + 2])) : T(0.0));
  const T tol = T(PLANT_FORCE_TOL) * fsum;
  int bits = 0;
  WBC_PLANT_UNROLL
  for (int c = 0; c < 4; c++) {
    const T fx = f[3 * c], fy = f[3 * c + 1], fz = f[3 * c + 2];
    const bool st = (mask >> c) & 1u;
    const T lim = mu * fz + tol;
    bits |= (st && fz < T(0.0) - tol) ? PLANT_PULL : 0;
    bits |= (st && (wabs(fx) > lim || wabs(fy) > lim)) ? PLANT_CONE : 0;
  }
  return bits;
}

// Final phase, one leg: the joint accelerations of the leg given the base accelerations and its own force
template <class T> WBC_HD void plant_leg_final(const PlantLeg<T>& L, const T* vdb, const T* f3, T* vdl) {
  T y[3];
  WBC_PLANT_UNROLL
  for (int k = 0; k < 3; k++) {
    T s = L.r[k] + (L.Jl[k] * f3[0] + L.Jl[3 + k] * f3[1] + L.Jl[6 + k] * f3[2]);
    WBC_PLANT_UNROLL
    for (int i = 0; i < 6; i++) s = s - L.B[3 * i + k] * vdb[i];
    y[k] = s;
  }
  rotv(L.Di, y, vdl);
}

// Semi-implicit Euler with exactly the arithmetic of wbc_integrate_kernel (wbc_kernels.hip): base part (quaternion, position,
// base velocity; qb[7] and vb[6] updated in place) and one joint.
template <class T> WBC_HD void plant_integrate_base(T dt, const T* vdb, T* qb, T* vb) {
  T vn[6];
  WBC_PLANT_UNROLL
  for (int r = 0; r < 6; r++) vn[r] = vb[r] + dt * vdb[r];
  quat_step(dt, vn[0], vn[1], vn[2], qb);
  WBC_PLANT_UNROLL
  for (int r = 0; r < 3; r++) qb[4 + r] += dt * vn[3 + r];
  WBC_PLANT_UNROLL
  for (int r = 0; r < 6; r++) vb[r] = vn[r];
}
template <class T> WBC_HD void plant_integrate_joint(T dt, T vd, T& q, T& v) {
  v = v + dt * vd;
  q += dt * v;
}

}  // namespace wbc
