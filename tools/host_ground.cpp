// host_ground.cpp -- TEST TOOL, not product code.
// Instantiates the compliant-ground plant math (quadruped_drake_amd/csrc/wbc_ground.hpp) on the host with `double`: the phases the
// device kernel runs on the four lanes of a quad, here one leg after the other, with the quad sums as plain sums in the kernel's
// order ((leg0 + leg1) + (leg2 + leg3)).  Both instantiations of the force law: the flat one (host_ground_batch) and the TERRAIN
// one (host_terrain_batch), whose packed table -- staged in LDS by the device kernels -- lives in plain memory here; and the law
// that makes the targets follow the terrain (host_follow_batch, wbc_ground_follow.hpp).
// tests/host_ground.py, tests/host_terrain.py and tests/host_follow.py load it; the shipped library never calls it.
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "../include/wbc_ground.h"
#include "../quadruped_drake_amd/csrc/wbc_ground.hpp"
#include "../quadruped_drake_amd/csrc/wbc_ground_follow.hpp"
#include "host_batch.hpp"

using namespace wbc;

struct HostGround {
  GroundLaw<double> law;
  double mu0, tau_max, fall_height;
  int count;                                            // 0: flat
  double table[TERRAIN_MAX_PROFILES * TERRAIN_STRIDE];
  const uint8_t* id;
  const double* scale;
};

// one instance; `substeps` force evaluations, each followed by an Euler step of h when step != 0 (q, v in place)
template <bool TERRAIN>
static void ground_one(const ModelC& m, const HostGround& P, int i, size_t ld, int step, int substeps, double dt, double* q, double* v,
                       double* time, const double* tau, const double* mup, const double* msp, const double* wext, double* vdot,
                       double* force, uint8_t* contact, int32_t* flags, int32_t* counts) {
  HostInstance s;
  host_gather(m, i, ld, q, v, tau, s);
  double we[6];
  for (int k = 0; k < 6; k++) we[k] = wext ? wext[k * ld + i] : 0.0;
  const double mu = mup ? mup[i] : P.mu0, s_p = msp ? msp[i] : 1.0;
  bool clip;
  bool nf = host_check_inputs(s, P.tau_max, mu, s_p, clip);
  for (int k = 0; k < 6; k++) nf |= not_finite(we[k]);
  const double* tab = nullptr;
  double tscale = 1.0;
  if (TERRAIN) {
    const int id = P.id ? (int)P.id[i] : 0;
    tscale = P.scale ? P.scale[i] : 1.0;
    const bool tbad = id >= P.count || not_finite(tscale);
    nf |= tbad;
    tab = P.table + (tbad ? 0 : id) * TERRAIN_STRIDE;
  }
  int bits = clip ? GROUND_CLIP : 0;
  const double h = step ? dt / substeps : 0.0;
  double fsum[12] = {0}, vdb[6] = {0}, vdl[4][3] = {{0}};
  int touch = 0, slip = 0;
  for (int sub = 0; sub < substeps; sub++) {
    double R0[9];
    plant_rotation(s.qb, R0);
    const double w0[3] = {s.vb[0], s.vb[1], s.vb[2]}, v0[3] = {s.vb[3], s.vb[4], s.vb[5]};
    PlantLeg<double> L[4];
    double f[12];
    touch = 0;
    for (int l = 0; l < 4; l++) {
      const int fb = ground_leg_phase<TERRAIN>(m, l, R0, w0, v0, s.qb[6], s.th[l], s.qd[l], s.ta[l], P.law, mu, L[l], f + 3 * l, s.qb[4],
                                               s.qb[5], tab, tscale);
      touch |= (fb & GROUND_FOOT_TOUCH) ? (1 << l) : 0;
      slip |= (fb & GROUND_FOOT_SLIP) ? 1 : 0;
    }
    double S[27];
    plant_base_share(m, R0, w0, s_p, S);
    for (int k = 0; k < 27; k++) {
      const double x[4] = {L[0].s[k], L[1].s[k], L[2].s[k], L[3].s[k]};
      S[k] = S[k] + qsum4(x);
    }
    for (int k = 0; k < 6; k++) S[21 + k] = S[21 + k] + we[k];
    ground_base_solve(S, vdb);
    for (int l = 0; l < 4; l++) plant_leg_final(L[l], vdb, f + 3 * l, vdl[l]);
    for (int k = 0; k < 6; k++) nf |= not_finite(vdb[k]);
    for (int l = 0; l < 4; l++)
      for (int k = 0; k < 3; k++) nf |= not_finite(vdl[l][k]) | not_finite(f[3 * l + k]);
    for (int k = 0; k < 12; k++) fsum[k] += f[k];
    if (step) {
      plant_integrate_base(h, vdb, s.qb, s.vb);
      for (int l = 0; l < 4; l++)
        for (int k = 0; k < 3; k++) plant_integrate_joint(h, vdl[l][k], s.th[l][k], s.qd[l][k]);
    }
  }
  for (int k = 0; k < 7; k++) nf |= not_finite(s.qb[k]);
  bits |= nf ? GROUND_BAD : 0;
  const bool bad = nf;
  if (!bad) bits |= (slip ? GROUND_SLIP : 0) | (ground_fell<TERRAIN>(s.qb, P.fall_height, tab, tscale) ? GROUND_FELL : 0);
  if (flags) flags[i] = bits;
  if (contact) contact[i] = bad ? 0 : (uint8_t)touch;
  if (vdot) host_store_vdot(s, i, ld, bad, vdb, vdl, vdot);
  const double inv = 1.0 / substeps;
  if (force)
    for (int k = 0; k < 12; k++) force[k * ld + i] = bad ? 0.0 : fsum[k] * inv;
  if (step) host_store_step(s, i, ld, bad, dt, bits, q, v, time, counts);
}

extern "C" {

// out8: stiffness, dissipation, mu, v_stiction, foot_radius, tau_max, max_substep, fall_height (wbc_ground_params_default)
int host_ground_defaults(const double* flat215, double* out8) {
  ModelC m;
  if (model_from_flat(flat215, &m) || !model_axes_are_xyy(&m)) return -1;
  ground_default_law(m, &out8[0], &out8[1]);
  out8[2] = 1.0; out8[3] = GROUND_V_STICTION; out8[4] = 0.0; out8[5] = INFINITY; out8[6] = GROUND_MAX_SUBSTEP; out8[7] = 0.0;
  return 0;
}

// params8 as host_ground_defaults writes them (NULL = the defaults).  step = 0: one force evaluation (q, v untouched, substeps
// ignored); step != 0: `substeps` explicit substeps of dt / substeps (substeps <= 0: ceil(dt / max_substep) as the product).
// Then the terrain as wbc_ground_set_terrain takes it, with host pointers; profiles NULL or count 0: no terrain, the flat
// instantiation.  Returns the number of substeps, -1 on a malformed model, -2 on a malformed terrain.
int host_terrain_batch(const double* flat215, const int* q_perm, const int* act_perm, const double* params8, int n, int ld, int step,
                       int substeps, double dt, double* q, double* v, double* time, const double* tau, const double* mu,
                       const double* mass_scale, const double* ext_wrench, double* vdot, double* force, uint8_t* contact,
                       int32_t* flags, int32_t* counts, const wbc_terrain_profile* profiles, int count, const uint8_t* terrain_id,
                       const double* terrain_scale) {
  ModelC m;
  if (model_from_flat(flat215, &m) || !model_axes_are_xyy(&m)) return -1;
  model_set_perms(&m, q_perm, act_perm);
  double p8[8];
  host_ground_defaults(flat215, p8);
  if (params8) memcpy(p8, params8, sizeof p8);
  HostGround P;
  P.law.k = p8[0]; P.law.d = p8[1]; P.mu0 = p8[2]; P.law.vs = p8[3]; P.law.radius = p8[4]; P.tau_max = p8[5]; P.fall_height = p8[7];
  P.count = 0; P.id = terrain_id; P.scale = terrain_scale;
  if (profiles && count != 0) {
    if (count < 1 || count > TERRAIN_MAX_PROFILES) return -2;
    for (int p = 0; p < count; p++) {
      const wbc_terrain_profile& t = profiles[p];
      if (terrain_profile_error(t.nk, t.x0, t.y0, t.yaw, t.s, t.h)) return -2;
      terrain_pack(t.nk, t.x0, t.y0, t.yaw, t.s, t.h, P.table + p * TERRAIN_STRIDE);
    }
    P.count = count;
  }
  if (!step) substeps = 1;
  else if (substeps <= 0) substeps = ground_substeps(dt, p8[6]);
  if (substeps <= 0) return -1;
  for (int i = 0; i < n; i++) {
    if (P.count)
      ground_one<true>(m, P, i, (size_t)ld, step, substeps, dt, q, v, time, tau, mu, mass_scale, ext_wrench, vdot, force, contact, flags, counts);
    else
      ground_one<false>(m, P, i, (size_t)ld, step, substeps, dt, q, v, time, tau, mu, mass_scale, ext_wrench, vdot, force, contact, flags, counts);
  }
  return substeps;
}

// wbc_ground_follow_targets on the host: follow_instance of wbc_ground_follow.hpp, one instance after the other, in place on
// targets [54][ld], with the terrain as wbc_ground_set_terrain takes it (host pointers).  No terrain, mode 0 or n = 0: nothing.
// Returns 0, -2 on a malformed terrain, -3 on a mode outside 0 .. 2.
int host_follow_batch(const wbc_terrain_profile* profiles, int count, const uint8_t* terrain_id, const double* terrain_scale, int n,
                      int ld, int mode, double* targets) {
  if (mode != FOLLOW_OFF && mode != FOLLOW_LIFT && mode != FOLLOW_FIT) return -3;
  if (!profiles || count == 0 || mode == FOLLOW_OFF) return 0;
  if (count < 1 || count > TERRAIN_MAX_PROFILES) return -2;
  double table[TERRAIN_MAX_PROFILES * TERRAIN_STRIDE];
  for (int p = 0; p < count; p++) {
    const wbc_terrain_profile& t = profiles[p];
    if (terrain_profile_error(t.nk, t.x0, t.y0, t.yaw, t.s, t.h)) return -2;
    terrain_pack(t.nk, t.x0, t.y0, t.yaw, t.s, t.h, table + p * TERRAIN_STRIDE);
  }
  for (int i = 0; i < n; i++) follow_instance(mode, table, count, terrain_id, terrain_scale, targets, (size_t)ld, (size_t)i);
  return 0;
}

// host_terrain_batch without a terrain
int host_ground_batch(const double* flat215, const int* q_perm, const int* act_perm, const double* params8, int n, int ld, int step,
                      int substeps, double dt, double* q, double* v, double* time, const double* tau, const double* mu,
                      const double* mass_scale, const double* ext_wrench, double* vdot, double* force, uint8_t* contact,
                      int32_t* flags, int32_t* counts) {
  return host_terrain_batch(flat215, q_perm, act_perm, params8, n, ld, step, substeps, dt, q, v, time, tau, mu, mass_scale, ext_wrench,
                            vdot, force, contact, flags, counts, nullptr, 0, nullptr, nullptr);
}

}  // extern "C"
