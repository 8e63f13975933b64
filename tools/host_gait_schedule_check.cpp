// host_gait_schedule_check.cpp -- TEST TOOL, not product code.
// A stand-alone program over tools/host_gait.cpp: the host instantiation of the gait planner's law under command schedules
// (include/wbc_gait_schedule.h) on a batch that visits every m = 0 .. 7, an invalid m, blends of 0 and 0.5, the plane
// and a terrain.  tests/test_gait_schedule_cpu.py builds it with -fsanitize=address,undefined and runs it: the program prints a
// checksum and returns 0, and the sanitizers abort it on anything they find.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/wbc_gait_schedule.h"
#include "../include/wbc_gait_terrain.h"

extern "C" int host_gait_schedule_batch(const wbc_gait_params* params, const wbc_gait_stride* strides, int count, const wbc_gait_terrain_params* tparams,
                                        const wbc_terrain_profile* profiles, int tcount, int n, int ld, const double* time, const double* cmd,
                                        const uint8_t* gait_id, const double* stride_scale, const double* start, const uint8_t* terrain_id,
                                        const double* terrain_scale, double blend, const uint8_t* nswitch, const double* when, const double* cmds,
                                        double* targets, uint8_t* contact_mask, double* knots);

int main(void) {
  const int n = 67, ld = 67;   // exactly the batch: a read or write past column n - 1 is past the allocation
  wbc_gait_params P;
  const double stance[4][2] = {{0.19, 0.11}, {0.19, -0.11}, {-0.19, 0.11}, {-0.19, -0.11}};
  memcpy(P.stance, stance, sizeof stance);
  P.height = 0.3; P.swing_height = 0.05; P.ramp_time = 0.5; P.wait_time = 0.25;
  wbc_gait_stride S[2];
  memset(S, 0, sizeof S);
  S[0].nphase = 4;
  const double d0[4] = {0.3, 0.2, 0.3, 0.2};
  const uint8_t m0[4] = {9, 15, 6, 15};
  for (int j = 0; j < 4; j++) { S[0].duration[j] = d0[j]; S[0].contact[j] = m0[j]; }
  S[1].nphase = 8;
  const uint8_t m1[8] = {11, 15, 14, 15, 7, 15, 13, 15};
  for (int j = 0; j < 8; j++) { S[1].duration[j] = j % 2 ? 0.2 : 0.3; S[1].contact[j] = m1[j]; }
  wbc_gait_terrain_params T;
  T.body_mode = WBC_GAIT_BODY_FIT; T.max_grade = 0.5; T.edge_margin = 0.03; T.apex_max = 0.25;
  wbc_terrain_profile prof;
  memset(&prof, 0, sizeof prof);
  prof.nk = 2; prof.yaw = 0.3;
  prof.s[0] = 0.3; prof.s[1] = 0.35; prof.h[0] = 0.0; prof.h[1] = 0.1;

  double* time = (double*)malloc(sizeof(double) * ld);
  double* cmd = (double*)malloc(sizeof(double) * 3 * ld);
  double* start = (double*)malloc(sizeof(double) * 3 * ld);
  double* scale = (double*)malloc(sizeof(double) * ld);
  uint8_t* gid = (uint8_t*)malloc(ld);
  uint8_t* ns = (uint8_t*)malloc(ld);
  double* when = (double*)malloc(sizeof(double) * 7 * ld);
  double* cmds = (double*)malloc(sizeof(double) * 21 * ld);
  double* tg = (double*)malloc(sizeof(double) * 54 * ld);
  uint8_t* mk = (uint8_t*)malloc(ld);
  double* knots = (double*)malloc(sizeof(double) * 175 * ld);
  double sum = 0.0;
  int bad = 0;
  for (int pass = 0; pass < 4; pass++) {
    const double blend = pass % 2 ? 0.5 : 0.0;
    for (int i = 0; i < n; i++) {
      time[i] = -0.1 + 0.31 * i;
      cmd[i] = 0.2 + 0.01 * i; cmd[ld + i] = -0.1 + 0.005 * i; cmd[2 * ld + i] = i % 3 ? 0.5 - 0.02 * i : 0.0;
      start[i] = 0.1 * i; start[ld + i] = -0.05 * i; start[2 * ld + i] = 0.3 * i;
      scale[i] = 0.5 + 0.02 * i;
      gid[i] = (uint8_t)(i % 2);
      ns[i] = (uint8_t)(i % 9 == 8 ? 9 : i % 9);          // 0 .. 7, and 9: an invalid schedule
      for (int j = 0; j < 7; j++) {
        when[j * ld + i] = 0.4 + 1.3 * j + 0.01 * i;
        cmds[(3 * j) * ld + i] = 0.3 - 0.05 * j; cmds[(3 * j + 1) * ld + i] = 0.02 * j; cmds[(3 * j + 2) * ld + i] = j % 2 ? -0.6 : 0.4;
      }
    }
    const int rc = host_gait_schedule_batch(&P, S, 2, pass < 2 ? NULL : &T, pass < 2 ? NULL : &prof, pass < 2 ? 0 : 1, n, ld, time, cmd, gid, scale,
                                            start, NULL, NULL, blend, ns, when, cmds, tg, mk, pass % 2 ? knots : NULL);
    if (rc) { printf("pass %d: rc %d\n", pass, rc); return 1; }
    for (int i = 0; i < n; i++) {
      const int invalid = ns[i] > 7;
      for (int r = 0; r < 54; r++) {
        const double x = tg[r * ld + i];
        if (invalid != (x != x)) bad++;
        if (!invalid) sum += x;
      }
      if (invalid && mk[i] != 0xF) bad++;
    }
  }
  printf("host_gait_schedule_check: checksum %.17g, %d rows out of place\n", sum, bad);
  free(time); free(cmd); free(start); free(scale); free(gid); free(ns); free(when); free(cmds); free(tg); free(mk); free(knots);
  return bad ? 1 : 0;
}
