// host_tick_check.cpp -- TEST TOOL: a stand-alone driver of host_tick.cpp, linked with it into one executable and run under sanitizers
// (tests/test_host_twin_standalone_cpu.py), because that code is otherwise only ever checked inside python.
//   host_tick_check hex FILE    the 16-lane emulation and its rollout; a repeated call must give the bits of the first (address, undefined)
//   host_tick_check bench FILE  host_tick_bench alone, 4 threads and 6 passes over 16 instances (thread)
// FILE: flat[215], then q[19][8], v[18][8], targets[54][8] (doubles) and mask[8] (bytes) of workloads.make_batch(cfg, n=8) for cfg 2, then 3.
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>

extern "C" {
int host_hex_batch(int kind, const double* flat215, const double* params12, const int* q_perm, const int* act_perm, int n, int stride,
                   const double* q, const double* v, const double* tg, const unsigned char* mask, const double* mu, const double* mass_scale,
                   double* tau, double* met, int* status, int* iters);
int host_hex_rollout(int kind, const double* flat215, const double* params12, int n, int stride, int steps, double dt, int warm, double* q, double* v,
                     const double* tg_seq, const unsigned char* masks, const double* mu, const double* mass_scale, double* tau, double* met,
                     int* status, double* iters_sum, int* status_nonzero_ticks);
int host_tick_bench(int kind, const double* flat215, int n, int stride, const double* q, const double* v, const double* tg, const unsigned char* mask,
                    const double* mu, const double* mass_scale, double* tau, int* status, int nthreads, int reps);
void host_set_vdot_sink(double* vdot);
}

enum { ID = 0, MPTC = 1, PC = 2, CLF = 3, N = 8 };
struct Batch { double q[19][N], v[18][N], tg[54][N]; unsigned char mask[N]; };
struct Out {
  double tau[12][N], met[4][N];
  int status[N], iters[N];
};

static int fail(const char* what) { fprintf(stderr, "host_tick_check: %s\n", what); return 1; }

static bool hex(int kind, const double* flat, const double* params12, const Batch& b, Out* o) {
  memset(o, 0, sizeof(*o));
  if (host_hex_batch(kind, flat, params12, nullptr, nullptr, N, N, &b.q[0][0], &b.v[0][0], &b.tg[0][0], b.mask, nullptr, nullptr, &o->tau[0][0],
                     &o->met[0][0], o->status, o->iters)) return false;
  for (int k = 0; k < 12 * N; k++) if (!isfinite((&o->tau[0][0])[k])) return false;
  return true;
}

int main(int argc, char** argv) {
  if (argc != 3) return fail("usage: host_tick_check hex|bench FILE");
  double flat[215];
  Batch b2, b3;
  FILE* f = fopen(argv[2], "rb");
  if (!f || fread(flat, sizeof(flat), 1, f) != 1 || fread(&b2, sizeof(b2), 1, f) != 1 || fread(&b3, sizeof(b3), 1, f) != 1) return fail("cannot read FILE");
  fclose(f);

  if (!strcmp(argv[1], "bench")) {
    // 16 instances: config 3's eight, then config 2's
    std::vector<double> q(19 * 16), v(18 * 16), tg(54 * 16), tau(12 * 16, NAN);
    unsigned char mask[16];
    int status[16];
    for (int i = 0; i < 16; i++) {
      const Batch& b = i < N ? b3 : b2;
      for (int r = 0; r < 19; r++) q[r * 16 + i] = b.q[r][i % N];
      for (int r = 0; r < 18; r++) v[r * 16 + i] = b.v[r][i % N];
      for (int r = 0; r < 54; r++) tg[r * 16 + i] = b.tg[r][i % N];
      mask[i] = b.mask[i % N];
      status[i] = -1;
    }
    if (host_tick_bench(MPTC, flat, 16, 16, q.data(), v.data(), tg.data(), mask, nullptr, nullptr, tau.data(), status, 4, 6)) return fail("host_tick_bench");
    for (int i = 0; i < 16; i++) if (status[i] < 0) return fail("the last pass left a status unwritten");
    for (double x : tau) if (!isfinite(x)) return fail("the last pass left a torque unwritten");
    return 0;
  }

  // four laws and a torque box (params12 of the ID law with tau_max = 8)
  const double boxed[12] = {500.0, 50.0, 500.0, 50.0, 100.0, 20.0, 10.0, 1.0, 0.7, 100.0, 8.0, 1e-8};
  Out first, o;
  if (!hex(ID, flat, nullptr, b2, &first) || !hex(MPTC, flat, nullptr, b3, &o) || !hex(PC, flat, nullptr, b3, &o) || !hex(CLF, flat, nullptr, b2, &o) ||
      !hex(ID, flat, boxed, b2, &o)) return fail("host_hex_batch");
  {  // warm rollout, 2 robots x 5 ticks: config 2's first two states under the targets of its first five instances
    double q[19][2], v[18][2], tgs[5][54], tau[12][2], met[4][2], its[2];
    unsigned char masks[5];
    int status[2], bad = -1;
    for (int i = 0; i < 2; i++) {
      for (int r = 0; r < 19; r++) q[r][i] = b2.q[r][i];
      for (int r = 0; r < 18; r++) v[r][i] = b2.v[r][i];
    }
    for (int s = 0; s < 5; s++) {
      for (int r = 0; r < 54; r++) tgs[s][r] = b2.tg[r][s];
      masks[s] = b2.mask[s];
    }
    if (host_hex_rollout(ID, flat, nullptr, 2, 2, 5, 5e-3, 1, &q[0][0], &v[0][0], &tgs[0][0], masks, nullptr, nullptr, &tau[0][0], &met[0][0], status, its,
                         &bad) || bad < 0) return fail("host_hex_rollout");
  }
  // nothing is remembered between calls: the first call again, then once more after a sink was set and cleared
  if (!hex(ID, flat, nullptr, b2, &o) || memcmp(&o, &first, sizeof(o))) return fail("the first batch, repeated after other calls, gave other bits");
  double vdot[18][N];
  host_set_vdot_sink(&vdot[0][0]);
  host_set_vdot_sink(nullptr);
  if (!hex(ID, flat, nullptr, b2, &o) || memcmp(&o, &first, sizeof(o))) return fail("the first batch, repeated after a sink was set and cleared, gave other bits");
  return 0;
}
