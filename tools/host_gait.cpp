// host_gait.cpp -- TEST TOOL, not product code.
// Instantiates the gait planner's law (quadruped_drake_amd/csrc/wbc_gait.hpp) on the host: what the device kernel runs on the four
// lanes of a quad, here one foot after the other, on the same packed table in plain memory.  tests/host_gait.py loads it; the shipped
// library never calls it.
#include <math.h>
#include <stdint.h>
#include "../include/wbc_gait.h"
#include "../quadruped_drake_amd/csrc/wbc_gait.hpp"

using namespace wbc;

extern "C" {

// wbc_gait_create + wbc_gait_set_commands + wbc_gait_targets with host pointers.  Returns 0, -1 on arguments wbc_gait_check refuses.
// table_out (optional, GAIT_TABLE_DOUBLES doubles): the packed table; diag (optional, [4][ld]): per instance the stride number k,
// the phase, and u and the run's start of foot `diag_foot` as gait_foot itself reports them.
int host_gait_batch(const wbc_gait_params* params, const wbc_gait_stride* strides, int count, int n, int ld, const double* time,
                    const double* cmd, const uint8_t* gait_id, const double* stride_scale, const double* start, double* targets,
                    uint8_t* contact_mask, double* table_out, double* diag, int diag_foot) {
  if (gait_error(params, strides, count)) return -1;
  double table[GAIT_TABLE_DOUBLES] = {0.0};
  gait_pack(params, strides, count, table);
  if (table_out)
    for (int k = 0; k < GAIT_TABLE_DOUBLES; k++) table_out[k] = table[k];
  for (int i = 0; i < n; i++) {
    const GaitIn in = gait_load(time, cmd, gait_id, stride_scale, start, (size_t)ld, (size_t)i);
    const GaitClock c = gait_clock(table, count, in);
    double b[18], f[9], run[2], seen[2] = {0.0, 0.0};
    gait_body(table, in, c, b);
    for (int k = 0; k < 18; k++) targets[(size_t)k * ld + i] = b[k];
    for (int l = 0; l < 4; l++) {
      gait_foot(table, in, c, l, f, run);
      if (l == diag_foot) { seen[0] = run[0]; seen[1] = run[1]; }
      for (int k = 0; k < 9; k++) targets[(size_t)(18 + 9 * l + k) * ld + i] = f[k];
    }
    contact_mask[i] = (uint8_t)c.mask;
    if (diag) {
      diag[i] = c.k;
      diag[ld + i] = (double)c.phase;
      diag[2 * (size_t)ld + i] = seen[1];
      diag[3 * (size_t)ld + i] = seen[0];
    }
  }
  return 0;
}

// The same with a terrain (include/wbc_gait_terrain.h): + wbc_gait_set_terrain with host pointers.  Returns -2 on what
// wbc_gait_terrain_check refuses in the parameters, -3 on a profile wbc_terrain_check refuses, -4 on parameters that do not fit the gait.
int host_gait_terrain_batch(const wbc_gait_params* params, const wbc_gait_stride* strides, int count, const wbc_gait_terrain_params* tparams,
                            const wbc_terrain_profile* profiles, int tcount, int n, int ld, const double* time, const double* cmd,
                            const uint8_t* gait_id, const double* stride_scale, const double* start, const uint8_t* terrain_id,
                            const double* terrain_scale, double* targets, uint8_t* contact_mask) {
  if (gait_error(params, strides, count)) return -1;
  if (gait_terrain_error(tparams)) return -2;
  if (!profiles || tcount < 1 || tcount > TERRAIN_MAX_PROFILES) return -3;
  for (int p = 0; p < tcount; p++)
    if (terrain_profile_error(profiles[p].nk, profiles[p].x0, profiles[p].y0, profiles[p].yaw, profiles[p].s, profiles[p].h)) return -3;
  double table[GAIT_TABLE_DOUBLES] = {0.0}, ter[GAIT_TERRAIN_DOUBLES] = {0.0};
  gait_pack(params, strides, count, table);
  if (gait_terrain_fit_error(tparams, table)) return -4;
  gait_terrain_pack(tparams, table, profiles, tcount, ter);
  for (int i = 0; i < n; i++) {
    const GaitIn in = gait_load(time, cmd, gait_id, stride_scale, start, (size_t)ld, (size_t)i);
    const GaitGround G = gait_ground(ter, tcount, terrain_id ? (int)terrain_id[i] : 0, terrain_scale ? terrain_scale[i] : 1.0);
    GaitClock c = gait_clock(table, count, in);
    gait_clock_spoil(c, G.bad);
    double b[18], f[9], gr[12];
    for (int l = 0; l < 4; l++) {
      gait_foot<true>(table, in, c, l, f, nullptr, ter, &G, gr + 3 * l);
      for (int k = 0; k < 9; k++) targets[(size_t)(18 + 9 * l + k) * ld + i] = f[k];
    }
    gait_body<true>(table, in, c, b, ter, gr);
    for (int k = 0; k < 18; k++) targets[(size_t)k * ld + i] = b[k];
    contact_mask[i] = (uint8_t)c.mask;
  }
  return 0;
}

// The same under command schedules (include_gait_schedule/wbc_gait_schedule.h): + wbc_gait_set_schedule with host pointers, on the plane
// (tparams NULL) or on a terrain.  Returns -5 on null schedule arrays or a blend that is negative or not finite.  knots (optional,
// [GAIT_SCHEDULE_ROWS][ld]): the resolved schedules, as the handle's buffer holds them.
int host_gait_schedule_batch(const wbc_gait_params* params, const wbc_gait_stride* strides, int count, const wbc_gait_terrain_params* tparams,
                             const wbc_terrain_profile* profiles, int tcount, int n, int ld, const double* time, const double* cmd,
                             const uint8_t* gait_id, const double* stride_scale, const double* start, const uint8_t* terrain_id,
                             const double* terrain_scale, double blend, const uint8_t* nswitch, const double* when, const double* cmds,
                             double* targets, uint8_t* contact_mask, double* knots) {
  if (gait_error(params, strides, count)) return -1;
  if (!nswitch || !when || !cmds || !(blend >= 0.0) || not_finite(blend)) return -5;
  double table[GAIT_TABLE_DOUBLES] = {0.0}, ter[GAIT_TERRAIN_DOUBLES] = {0.0};
  gait_pack(params, strides, count, table);
  if (tparams) {
    if (gait_terrain_error(tparams)) return -2;
    if (!profiles || tcount < 1 || tcount > TERRAIN_MAX_PROFILES) return -3;
    for (int p = 0; p < tcount; p++)
      if (terrain_profile_error(profiles[p].nk, profiles[p].x0, profiles[p].y0, profiles[p].yaw, profiles[p].s, profiles[p].h)) return -3;
    if (gait_terrain_fit_error(tparams, table)) return -4;
    gait_terrain_pack(tparams, table, profiles, tcount, ter);
  }
  double own[GAIT_SCHEDULE_ROWS];
  for (int i = 0; i < n; i++) {
    const GaitIn in = gait_load(time, cmd, gait_id, stride_scale, start, (size_t)ld, (size_t)i);
    double* k = knots ? knots + i : own;
    const size_t ldk = knots ? (size_t)ld : 1;
    gait_schedule_resolve(in, blend, (int)nswitch[i], when + i, cmds + i, (size_t)ld, k, ldk);
    const GaitSchedule S = gait_schedule_load(k, ldk, 0, blend);
    GaitClock c = gait_clock(table, count, in);
    double b[18], f[9], gr[12];
    if (tparams) {
      const GaitGround G = gait_ground(ter, tcount, terrain_id ? (int)terrain_id[i] : 0, terrain_scale ? terrain_scale[i] : 1.0);
      gait_clock_spoil(c, G.bad | S.bad);
      for (int l = 0; l < 4; l++) {
        gait_foot<true, true>(table, in, c, l, f, nullptr, ter, &G, gr + 3 * l, &S);
        for (int r = 0; r < 9; r++) targets[(size_t)(18 + 9 * l + r) * ld + i] = f[r];
      }
      gait_body<true, true>(table, in, c, b, ter, gr, &S);
    } else {
      gait_clock_spoil(c, S.bad);
      for (int l = 0; l < 4; l++) {
        gait_foot<false, true>(table, in, c, l, f, nullptr, nullptr, nullptr, nullptr, &S);
        for (int r = 0; r < 9; r++) targets[(size_t)(18 + 9 * l + r) * ld + i] = f[r];
      }
      gait_body<false, true>(table, in, c, b, nullptr, nullptr, &S);
    }
    for (int r = 0; r < 18; r++) targets[(size_t)r * ld + i] = b[r];
    contact_mask[i] = (uint8_t)c.mask;
  }
  return 0;
}

}  // extern "C"
