// host_gait_feedback_check.cpp -- TEST TOOL, not product code.
// A stand-alone program over tools/host_gait_feedback.cpp and tools/host_gait.cpp: the host instantiation of the gait planner's
// foot-placement feedback (include/wbc_gait_feedback.h) driven tick by tick through the cases of
// tests/test_gait_feedback_cpu.py -- a perturbed walk on two strides, zero gains, a measurement on the plan, a constant velocity error,
// and damaged instances -- on arrays exactly as long as the batch.  That test builds it with -fsanitize=address,undefined and runs it:
// the program prints a checksum and returns 0, and the sanitizers abort it on anything they find.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/wbc_gait_feedback.h"

extern "C" int host_gait_batch(const wbc_gait_params* params, const wbc_gait_stride* strides, int count, int n, int ld, const double* time,
                               const double* cmd, const uint8_t* gait_id, const double* stride_scale, const double* start, double* targets,
                               uint8_t* contact_mask, double* table_out, double* diag, int diag_foot);
extern "C" void host_gait_feedback_reset(int cap, double* state, uint8_t* prev);
extern "C" int host_gait_feedback_batch(const wbc_gait_params* params, const wbc_gait_stride* strides, int count, const wbc_gait_feedback_params* fp,
                                        int n, int ld, const double* time, const uint8_t* gait_id, const double* stride_scale, const double* q,
                                        const double* v, double* targets, const uint8_t* contact_mask, double* offsets, int cap, double* state,
                                        uint8_t* prev);

int main(void) {
  const int n = 37, ld = 37, ticks = 400;   // exactly the batch: a read or write past column n - 1 is past the allocation
  wbc_gait_params P;
  const double stance[4][2] = {{0.19, 0.11}, {0.19, -0.11}, {-0.19, 0.11}, {-0.19, -0.11}};
  memcpy(P.stance, stance, sizeof stance);
  P.height = 0.3; P.swing_height = 0.05; P.ramp_time = 0.5; P.wait_time = 0.05;
  wbc_gait_stride S[2];
  memset(S, 0, sizeof S);
  S[0].nphase = 4;
  const double d0[4] = {0.3, 0.2, 0.3, 0.2};
  const uint8_t m0[4] = {9, 15, 6, 15};
  for (int j = 0; j < 4; j++) { S[0].duration[j] = d0[j]; S[0].contact[j] = m0[j]; }
  S[1].nphase = 8;
  const uint8_t m1[8] = {11, 15, 14, 15, 7, 15, 13, 15};
  for (int j = 0; j < 8; j++) { S[1].duration[j] = j % 2 ? 0.2 : 0.3; S[1].contact[j] = m1[j]; }
  wbc_gait_feedback_params F;
  F.k_v = sqrt(P.height / 9.81); F.k_p = 0.0; F.d_max = 0.10; F.u_hold = 0.5;   // wbc_gait_feedback_params_default's

  double* time = (double*)malloc(sizeof(double) * ld);
  double* cmd = (double*)malloc(sizeof(double) * 3 * ld);
  double* scale = (double*)malloc(sizeof(double) * ld);
  uint8_t* gid = (uint8_t*)malloc(ld);
  double* q = (double*)calloc(19 * ld, sizeof(double));
  double* v = (double*)calloc(18 * ld, sizeof(double));
  double* tg = (double*)malloc(sizeof(double) * 54 * ld);
  double* plain = (double*)malloc(sizeof(double) * 54 * ld);
  uint8_t* mk = (uint8_t*)malloc(ld);
  double* off = (double*)malloc(sizeof(double) * 8 * ld);
  double* state = (double*)malloc(sizeof(double) * 24 * n);
  uint8_t* prev = (uint8_t*)malloc(n);
  double sum = 0.0;
  int bad = 0;
  // pass 0: a perturbed walk; 1: zero gains; 2: the measurement on the plan; 3: a constant velocity error; 4: damage on every third tick
  for (int pass = 0; pass < 5; pass++) {
    wbc_gait_feedback_params G = F;
    G.k_p = pass == 0 || pass == 4 ? 0.5 : 0.0;
    G.d_max = 0.05;
    if (pass == 1) G.k_v = 0.0;
    host_gait_feedback_reset(n, state, prev);
    for (int k = 0; k < ticks; k++) {
      for (int i = 0; i < n; i++) {
        time[i] = 0.0025 * k + 0.0001234 - 0.002 * i;
        cmd[i] = 0.2 + 0.01 * i; cmd[ld + i] = -0.1 + 0.005 * i; cmd[2 * ld + i] = i % 3 ? 0.5 - 0.02 * i : 0.0;
        scale[i] = 0.4 + 0.02 * i;
        gid[i] = (uint8_t)(i % 2);
      }
      const int victim = k % n;
      if (pass == 4 && k % 3 == 0) {
        if (k % 2) time[victim] = NAN; else gid[victim] = 7;
      }
      if (host_gait_batch(&P, S, 2, n, ld, time, cmd, gid, scale, NULL, tg, mk, NULL, NULL, 0)) return 1;
      memcpy(plain, tg, sizeof(double) * 54 * ld);
      for (int i = 0; i < n; i++) {
        const double w = pass == 0 || pass == 4 ? 1.0 : 0.0, c = pass == 3 ? 1.0 : 0.0;
        q[4 * ld + i] = tg[i] + w * 0.05 * sin(3.1 * time[i] + i);
        q[5 * ld + i] = tg[ld + i] + w * 0.05 * cos(2.3 * time[i] - i);
        v[3 * ld + i] = tg[3 * ld + i] + w * 0.3 * sin(5.7 * time[i] + 2.0 * i) + c * 0.1;
        v[4 * ld + i] = tg[4 * ld + i] + w * 0.3 * cos(4.1 * time[i]) - c * 0.05;
      }
      if (pass == 4 && k % 3 == 1) v[3 * ld + victim] = INFINITY;
      const int rc = host_gait_feedback_batch(&P, S, 2, &G, n, ld, time, gid, scale, q, v, tg, mk, k % 2 ? off : NULL, n, state, prev);
      if (rc) { printf("pass %d tick %d: rc %d\n", pass, k, rc); return 1; }
      for (int i = 0; i < n; i++) {
        const int hit = pass == 4 && i == victim && k % 3 != 2;
        for (int r = 0; r < 54; r++) {
          const double x = tg[r * ld + i], y = plain[r * ld + i];
          if (hit || pass == 1 || pass == 2) { if (memcmp(&x, &y, sizeof x) && !(x == y)) bad++; }   // untouched, or + 0.0
          if (x == x) sum += x;
        }
        if (k % 2) for (int r = 0; r < 8; r++) { const double x = off[r * ld + i]; if (hit != (x != x)) bad++; if ((pass == 1 || pass == 2) && !hit && x != 0.0) bad++; }
      }
      for (int w = 0; w < 4 * n; w++)
        for (int r = 0; r < 6; r += 2)
          if (!(hypot(state[r * 4 * n + w], state[(r + 1) * 4 * n + w]) <= G.d_max * (1.0 + 4.0 * 0x1p-52))) bad++;
    }
  }
  if (host_gait_feedback_batch(&P, S, 2, &F, n + 1, ld + 1, time, gid, scale, q, v, tg, mk, NULL, n, state, prev) != -7) bad++;   // n > cap: refused before any access
  F.d_max = 0.0;
  if (host_gait_feedback_batch(&P, S, 2, &F, n, ld, time, gid, scale, q, v, tg, mk, NULL, n, state, prev) != -6) bad++;
  printf("host_gait_feedback_check: checksum %.17g, %d things out of place\n", sum, bad);
  free(time); free(cmd); free(scale); free(gid); free(q); free(v); free(tg); free(plain); free(mk); free(off); free(state); free(prev);
  return bad ? 1 : 0;
}
