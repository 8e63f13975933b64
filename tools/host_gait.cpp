// host_gait.cpp -- TEST TOOL, not product code.
// Instantiates the gait planner's law (quadruped_drake_amd/csrc/wbc_gait.hpp) on the host: what the device kernel runs on the four
// lanes of a quad, here one foot after the other, on the same packed table in plain memory.  tests/host_gait.py loads it; the shipped
// library never calls it.
#include <math.h>
#include <stdint.h>
#include "../include/wbc_gait.h"
#include "../quadruped_drake_amd/csrc/wbc_gait.hpp"

using namespace wbc;

namespace {

struct Terrain {    // wbc_gait_set_terrain's arguments
  const wbc_gait_terrain_params* params;
  const wbc_terrain_profile* profiles;
  int count;
  const uint8_t* id;
  const double* scale;
};
struct Schedule {   // wbc_gait_set_schedule's arguments; knots (optional): where the resolved schedules go
  double blend;
  const uint8_t* nswitch;
  const double* when;
  const double* cmds;
  double* knots;
};

// Instance i's 54 rows and its mask from the <TERRAIN, SCHEDULE> instantiation of the law: the four feet one after the other, then
// the body.  G, S: the instance's ground and schedule where the instantiation has them.  diag: host_gait_batch's.
template <bool TERRAIN, bool SCHEDULE>
void instance(const double* table, int count, const double* ter, const GaitIn& in, const GaitGround* G, const GaitSchedule* S, size_t ld,
              size_t i, double* targets, uint8_t* contact_mask, double* diag, int diag_foot) {
  GaitClock c = gait_clock(table, count, in);
  if constexpr (TERRAIN || SCHEDULE) gait_clock_spoil(c, (TERRAIN && G->bad) | (SCHEDULE && S->bad));
  double b[18], f[9], gr[12], run[2], seen[2] = {0.0, 0.0};
  for (int l = 0; l < 4; l++) {
    gait_foot<TERRAIN, SCHEDULE>(table, in, c, l, f, run, ter, G, gr + 3 * l, S);
    if (l == diag_foot) { seen[0] = run[0]; seen[1] = run[1]; }
    for (int k = 0; k < 9; k++) targets[(size_t)(18 + 9 * l + k) * ld + i] = f[k];
  }
  gait_body<TERRAIN, SCHEDULE>(table, in, c, b, ter, gr, S);
  for (int k = 0; k < 18; k++) targets[(size_t)k * ld + i] = b[k];
  contact_mask[i] = (uint8_t)c.mask;
  if (diag) {
    diag[i] = c.k;
    diag[ld + i] = (double)c.phase;
    diag[2 * ld + i] = seen[1];
    diag[3 * ld + i] = seen[0];
  }
}

// What the three entry points below share: the arguments checked in the order of their return codes, the tables packed, and every
// instance through the instantiation its handle would launch.  T, sch: null for a handle without a terrain, without a schedule.
int batch(const wbc_gait_params* params, const wbc_gait_stride* strides, int count, const Terrain* T, const Schedule* sch, int n, int ld,
          const double* time, const double* cmd, const uint8_t* gait_id, const double* stride_scale, const double* start, double* targets,
          uint8_t* contact_mask, double* table_out = nullptr, double* diag = nullptr, int diag_foot = -1) {
  if (gait_error(params, strides, count)) return -1;
  if (sch && (!sch->nswitch || !sch->when || !sch->cmds || !(sch->blend >= 0.0) || not_finite(sch->blend))) return -5;
  double table[GAIT_TABLE_DOUBLES] = {0.0}, ter[GAIT_TERRAIN_DOUBLES] = {0.0};
  gait_pack(params, strides, count, table);
  if (T) {
    if (gait_terrain_error(T->params)) return -2;
    if (!T->profiles || T->count < 1 || T->count > TERRAIN_MAX_PROFILES) return -3;
    for (int p = 0; p < T->count; p++) {
      const wbc_terrain_profile& f = T->profiles[p];
      if (terrain_profile_error(f.nk, f.x0, f.y0, f.yaw, f.s, f.h)) return -3;
    }
    if (gait_terrain_fit_error(T->params, table)) return -4;
    gait_terrain_pack(T->params, table, T->profiles, T->count, ter);
  }
  if (table_out)
    for (int k = 0; k < GAIT_TABLE_DOUBLES; k++) table_out[k] = table[k];
  double own[GAIT_SCHEDULE_ROWS];
  for (int i = 0; i < n; i++) {
    const GaitIn in = gait_load(time, cmd, gait_id, stride_scale, start, (size_t)ld, (size_t)i);
    GaitGround G{};
    GaitSchedule S{};
    if (T) G = gait_ground(ter, T->count, T->id ? (int)T->id[i] : 0, T->scale ? T->scale[i] : 1.0);
    if (sch) {
      double* k = sch->knots ? sch->knots + i : own;
      const size_t ldk = sch->knots ? (size_t)ld : 1;
      gait_schedule_resolve(in, sch->blend, (int)sch->nswitch[i], sch->when + i, sch->cmds + i, (size_t)ld, k, ldk);
      S = gait_schedule_load(k, ldk, 0, sch->blend);
    }
    const auto rows = T ? (sch ? instance<true, true> : instance<true, false>) : (sch ? instance<false, true> : instance<false, false>);
    rows(table, count, ter, in, &G, &S, (size_t)ld, (size_t)i, targets, contact_mask, diag, diag_foot);
  }
  return 0;
}

}  // namespace

extern "C" {

// wbc_gait_create + wbc_gait_set_commands + wbc_gait_targets with host pointers.  Returns 0, -1 on arguments wbc_gait_check refuses.
// table_out (optional, GAIT_TABLE_DOUBLES doubles): the packed table; diag (optional, [4][ld]): per instance the stride number k,
// the phase, and u and the run's start of foot `diag_foot` as gait_foot itself reports them.
int host_gait_batch(const wbc_gait_params* params, const wbc_gait_stride* strides, int count, int n, int ld, const double* time,
                    const double* cmd, const uint8_t* gait_id, const double* stride_scale, const double* start, double* targets,
                    uint8_t* contact_mask, double* table_out, double* diag, int diag_foot) {
  return batch(params, strides, count, nullptr, nullptr, n, ld, time, cmd, gait_id, stride_scale, start, targets, contact_mask, table_out, diag,
               diag_foot);
}

// The same with a terrain (include/wbc_gait_terrain.h): + wbc_gait_set_terrain with host pointers.  Returns -2 on what
// wbc_gait_terrain_check refuses in the parameters, -3 on a profile wbc_terrain_check refuses, -4 on parameters that do not fit the gait.
int host_gait_terrain_batch(const wbc_gait_params* params, const wbc_gait_stride* strides, int count, const wbc_gait_terrain_params* tparams,
                            const wbc_terrain_profile* profiles, int tcount, int n, int ld, const double* time, const double* cmd,
                            const uint8_t* gait_id, const double* stride_scale, const double* start, const uint8_t* terrain_id,
                            const double* terrain_scale, double* targets, uint8_t* contact_mask) {
  const Terrain T{tparams, profiles, tcount, terrain_id, terrain_scale};
  return batch(params, strides, count, &T, nullptr, n, ld, time, cmd, gait_id, stride_scale, start, targets, contact_mask);
}

// The same under command schedules (include/wbc_gait_schedule.h): + wbc_gait_set_schedule with host pointers, on the plane
// (tparams NULL) or on a terrain.  Returns -5 on null schedule arrays or a blend that is negative or not finite.  knots (optional,
// [GAIT_SCHEDULE_ROWS][ld]): the resolved schedules, as the handle's buffer holds them.
int host_gait_schedule_batch(const wbc_gait_params* params, const wbc_gait_stride* strides, int count, const wbc_gait_terrain_params* tparams,
                             const wbc_terrain_profile* profiles, int tcount, int n, int ld, const double* time, const double* cmd,
                             const uint8_t* gait_id, const double* stride_scale, const double* start, const uint8_t* terrain_id,
                             const double* terrain_scale, double blend, const uint8_t* nswitch, const double* when, const double* cmds,
                             double* targets, uint8_t* contact_mask, double* knots) {
  const Terrain T{tparams, profiles, tcount, terrain_id, terrain_scale};
  const Schedule sch{blend, nswitch, when, cmds, knots};
  return batch(params, strides, count, tparams ? &T : nullptr, &sch, n, ld, time, cmd, gait_id, stride_scale, start, targets, contact_mask);
}

}  // extern "C"
