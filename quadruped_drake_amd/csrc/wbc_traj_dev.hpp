// wbc_traj_dev.hpp -- device-side pieces shared by the stand-alone target lookup (wbc_traj.hip) and the
// persistent closed-loop kernel (wbc_kernels.hip): the stored trunk trajectory as plain device pointers,
// the nearest-sample index of planners/towr.py:92-106, and the semi-implicit Euler step of the rollout.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define WBC_TRAJ_HD __host__ __device__ inline
#else
#define WBC_TRAJ_HD inline
#endif
#include <math.h>
#include <stdint.h>

namespace wbc {

struct TrajDev {
  int K;
  double wait_time;
  const double* ts;        // [K] non-decreasing
  const double* table;     // [K][54]
  const uint8_t* masks;    // [K]
  const double* standing;  // [54]
  uint8_t standing_mask;
};

// Index of the sample np.abs(timestamps - (t - wait_time)).argmin() returns, for EVERY double t and any hint, or -1 for the standing
// targets (t < wait_time, or an empty trajectory).  The law in numpy's own terms: tq = t - wait_time rounded to double, d[j] =
// |ts[j] - tq| rounded to double, and the answer is the first j whose d[j] is a NaN, else the first j of the smallest d[j].
//   tq NaN (t NaN): every d[j] is NaN, the answer is 0.  (t < wait_time is false for a NaN: no standing targets.)
//   otherwise, with lo = the first index whose ts[lo] >= tq: rounding is monotone, so d does not increase up to lo - 1 and does not
//   decrease from lo on; the smallest d is d[lo - 1] or d[lo].  If d[lo] is smaller -- or a NaN, which is tq = ts[lo] = +inf -- the
//   answer is lo (no equal timestamp precedes lo).  Else it is the first j <= lo - 1 with d[j] <= d[lo - 1]: equal timestamps, real
//   ties, and every distance that the subtraction ROUNDS to the same double (tq = 2^53 against a table near 0; tq = 1e17 or +inf, where
//   all d are equal and the answer is 0).  d does not increase there, so that j is found by galloping back from lo - 1 and bisecting:
//   O(log) loads, and where d[lo - 2] > d[lo - 1] -- the ordinary case -- the one load of ts[lo - 2].
// `hint`: where to start looking (any value; the previous tick's index makes the search O(1) in a rollout).  It changes how lo is
// found, never the answer.
WBC_TRAJ_HD int traj_index(const TrajDev& T, double t, int hint) {
  if (t < T.wait_time || T.K == 0) return -1;
  t -= T.wait_time;
  if (t != t) return 0;
  const double* ts = T.ts;
  const int K = T.K;
  // bracket the first index with ts[idx] >= t by galloping from the hint, then bisect
  int lo, hi;
  int h = hint < 0 ? 0 : (hint >= K ? K - 1 : hint);
  if (ts[h] < t) {
    int step = 1;
    lo = h + 1;
    hi = K;
    while (lo < K) {
      const int probe = (h + step < K) ? h + step : K - 1;
      if (ts[probe] < t) { lo = probe + 1; if (probe == K - 1) break; step <<= 1; }
      else { hi = probe; break; }
    }
    if (lo > hi) lo = hi;
  } else {
    int step = 1;
    hi = h;
    lo = 0;
    while (hi > 0) {
      const int probe = (h - step > 0) ? h - step : 0;
      if (ts[probe] >= t) { hi = probe; if (probe == 0) break; step <<= 1; }
      else { lo = probe + 1; break; }
    }
  }
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ts[mid] < t) lo = mid + 1; else hi = mid;
  }
  if (lo == 0) return 0;
  const double dl = fabs(ts[lo - 1] - t);
  if (lo < K && !(dl <= fabs(ts[lo] - t))) return lo;   // (a NaN on the right is tq = ts[lo] = +inf: numpy's first NaN)
  // the first j <= lo - 1 with d[j] <= dl: gallop back while the distance holds, then bisect between the last miss and the last hit
  int c = lo - 1, miss = -1, step = 1;
  while (c > 0) {
    const int probe = (c - step > 0) ? c - step : 0;
    if (fabs(ts[probe] - t) <= dl) { c = probe; step <<= 1; }
    else { miss = probe; break; }
  }
  int l = miss + 1;
  while (l < c) {
    const int mid = (l + c) >> 1;
    if (fabs(ts[mid] - t) <= dl) c = mid; else l = mid + 1;
  }
  return c;
}

}  // namespace wbc
