// host_plant.cpp -- TEST TOOL, not product code.
// Instantiates the plant math (quadruped_drake_amd/csrc/wbc_plant.hpp) on the host with `double`: the same phases the device
// kernel runs on the four lanes of a quad, here one leg after the other, with the quad sums as plain sums in the kernel's order
// ((leg0 + leg1) + (leg2 + leg3)).  tests/host_plant.py builds it; the shipped library never calls it.
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "../quadruped_drake_amd/csrc/wbc_model.hpp"
#include "../quadruped_drake_amd/csrc/wbc_plant.hpp"

using namespace wbc;

static double qsum4(const double* x) { return (x[0] + x[1]) + (x[2] + x[3]); }

// one instance; q, v in place when step != 0
static void plant_one(const ModelC& m, double Kd, double tau_max, double mu0, int i, size_t ld, int step, double dt, double* q,
                      double* v, double* time, const double* tau, const uint8_t* maskp, const double* mup, const double* msp,
                      double* vdot, double* force, int32_t* flags, int32_t* counts) {
  double qb[7], vb[6], th[4][3], qd[4][3], tq[4][3];
  int qrow[4][3];
  for (int k = 0; k < 7; k++) qb[k] = q[k * ld + i];
  for (int k = 0; k < 6; k++) vb[k] = v[k * ld + i];
  for (int l = 0; l < 4; l++)
    for (int k = 0; k < 3; k++) {
      qrow[l][k] = m.q_perm[3 * l + k];
      th[l][k] = q[(7 + qrow[l][k]) * ld + i];
      qd[l][k] = v[(6 + qrow[l][k]) * ld + i];
      tq[l][k] = tau[m.act_inv[3 * l + k] * ld + i];
    }
  const unsigned mask = maskp[i] & 15u;
  const double mu = mup ? mup[i] : mu0, s_p = msp ? msp[i] : 1.0;
  int bits = 0;
  bool nf = false, clip = false;
  for (int k = 0; k < 7; k++) nf |= not_finite(qb[k]);
  for (int k = 0; k < 6; k++) nf |= not_finite(vb[k]);
  double ta[4][3];
  for (int l = 0; l < 4; l++)
    for (int k = 0; k < 3; k++) {
      nf |= not_finite(th[l][k]) | not_finite(qd[l][k]) | not_finite(tq[l][k]);
      clip |= fabs(tq[l][k]) > tau_max * (1.0 + PLANT_CLIP_TOL);
      ta[l][k] = fmin(fmax(tq[l][k], -tau_max), tau_max);
    }
  nf |= !(mu > 0.0) | not_finite(mu) | !(s_p > 0.0) | not_finite(s_p);
  bits = (nf ? PLANT_BAD : 0) | (clip ? PLANT_CLIP : 0);
  double R0[9];
  plant_rotation(qb, R0);
  const double w0[3] = {vb[0], vb[1], vb[2]}, v0[3] = {vb[3], vb[4], vb[5]};
  PlantLeg<double> L[4];
  for (int l = 0; l < 4; l++) plant_leg_phase1(m, l, R0, w0, v0, th[l], qd[l], ta[l], ((mask >> l) & 1u) != 0, Kd, L[l]);
  double S[27];
  plant_base_share(m, R0, w0, s_p, S);
  for (int k = 0; k < 27; k++) {
    const double x[4] = {L[0].s[k], L[1].s[k], L[2].s[k], L[3].s[k]};
    S[k] = S[k] + qsum4(x);
  }
  double rinvb[6], pivb[6], a0b[6];
  plant_chol<double, 6>(S, rinvb, pivb);
  for (int k = 0; k < 6; k++) a0b[k] = S[21 + k];
  plant_fwd<double, 6>(S, rinvb, a0b);
  plant_bwd<double, 6>(S, rinvb, a0b);
  double Z[4][18], G[4][9], e[12], a0l[4][3];
  for (int l = 0; l < 4; l++) plant_leg_phase2(L[l], S, rinvb, a0b, ((mask >> l) & 1u) != 0, Z[l], G[l], e + 3 * l, a0l[l]);
  double A[78], f[12];
  for (int c = 0; c < 4; c++)
    for (int d = 0; d <= c; d++) {
      double blk[9];
      plant_lambda_block(Z[c], Z[d], G[c], c == d, blk);
      for (int ii = 0; ii < 3; ii++)
        for (int j = 0; j < 3; j++)
          if (d < c || j <= ii) A[sp(3 * c + ii, 3 * d + j)] = blk[3 * ii + j];
    }
  const bool pivots_ok = plant_contact_solve(A, e, mask, f);
  double vdb[6], vdl[4][3];
  for (int k = 0; k < 6; k++) {
    double x[4];
    for (int l = 0; l < 4; l++) x[l] = Z[l][3 * k] * f[3 * l] + Z[l][3 * k + 1] * f[3 * l + 1] + Z[l][3 * k + 2] * f[3 * l + 2];
    vdb[k] = qsum4(x);
  }
  plant_bwd<double, 6>(S, rinvb, vdb);
  for (int k = 0; k < 6; k++) vdb[k] = a0b[k] + vdb[k];
  for (int l = 0; l < 4; l++) plant_leg_final(L[l], vdb, f + 3 * l, vdl[l]);
  nf = !pivots_ok;
  for (int k = 0; k < 6; k++) nf |= not_finite(vdb[k]);
  for (int l = 0; l < 4; l++)
    for (int k = 0; k < 3; k++) nf |= not_finite(vdl[l][k]) | not_finite(f[3 * l + k]);
  bits |= nf ? PLANT_BAD : 0;
  const bool bad = bits & PLANT_BAD;
  bits |= bad ? 0 : plant_force_flags(f, mask, mu, plant_weight(m, s_p));
  for (int k = 0; k < 6; k++) vdb[k] = bad ? 0.0 : vdb[k];
  for (int l = 0; l < 4; l++)
    for (int k = 0; k < 3; k++) {
      vdl[l][k] = bad ? 0.0 : vdl[l][k];
      f[3 * l + k] = (bad || !((mask >> l) & 1u)) ? 0.0 : f[3 * l + k];
    }
  if (flags) flags[i] = bits;
  if (vdot) {
    for (int k = 0; k < 6; k++) vdot[k * ld + i] = vdb[k];
    for (int l = 0; l < 4; l++)
      for (int k = 0; k < 3; k++) vdot[(6 + qrow[l][k]) * ld + i] = vdl[l][k];
  }
  if (force)
    for (int k = 0; k < 12; k++) force[k * ld + i] = f[k];
  if (!step) return;
  if (!bad) {
    plant_integrate_base(dt, vdb, qb, vb);
    for (int k = 0; k < 6; k++) v[k * ld + i] = vb[k];
    for (int k = 0; k < 7; k++) q[k * ld + i] = qb[k];
    for (int l = 0; l < 4; l++)
      for (int k = 0; k < 3; k++) {
        double qn = th[l][k], vn = qd[l][k];
        plant_integrate_joint(dt, vdl[l][k], qn, vn);
        v[(6 + qrow[l][k]) * ld + i] = vn;
        q[(7 + qrow[l][k]) * ld + i] = qn;
      }
  }
  if (time) time[i] += dt;
  if (counts)
    for (int b = 0; b < 4; b++)
      if ((bits >> b) & 1) counts[b * ld + i] += 1;
}

extern "C" {

// params3: Kd_contact, tau_max, mu (NULL = 100, +inf, 1.0).  step = 0: forward only (q, v untouched).  Returns <0 on a bad model.
int host_plant_batch(const double* flat215, const int* q_perm, const int* act_perm, const double* params3, int n, int ld, int step,
                     double dt, double* q, double* v, double* time, const double* tau, const uint8_t* mask, const double* mu,
                     const double* mass_scale, double* vdot, double* force, int32_t* flags, int32_t* counts) {
  ModelC m;
  if (model_from_flat(flat215, &m) || !model_axes_are_xyy(&m)) return -1;
  model_set_perms(&m, q_perm, act_perm);
  const double Kd = params3 ? params3[0] : 100.0, tau_max = params3 ? params3[1] : INFINITY, mu0 = params3 ? params3[2] : 1.0;
  for (int i = 0; i < n; i++)
    plant_one(m, Kd, tau_max, mu0, i, (size_t)ld, step, dt, q, v, time, tau, mask, mu, mass_scale, vdot, force, flags, counts);
  return 0;
}

}  // extern "C"
