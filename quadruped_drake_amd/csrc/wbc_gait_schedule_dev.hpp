// wbc_gait_schedule_dev.hpp -- what wbc_gait.hip and wbc_gait_schedule.hip share (internal, not installed): the gait planner's
// command schedules (include_gait_schedule/wbc_gait_schedule.h) have their kernels and entry points in a translation unit of their
// own, and the gait handle keeps their state behind one pointer.
#pragma once
#include <stdint.h>

namespace wbc {

struct GaitScheduleArgs {
  int n;                 // instances resolved; 0: no schedule
  int ld;                // the buffer's leading dimension in this resolution
  double beta;
  const double* knots;   // GAIT_SCHEDULE_ROWS rows of ld doubles (wbc_gait.hpp)
};

struct GaitScheduleState {
  double* d_knots;       // the buffer, GAIT_SCHEDULE_ROWS x capacity doubles, grown by wbc_gait_set_schedule as needed
  int capacity;
  GaitScheduleArgs args;
};

// one wbc_gait_targets call as the handle sees it: the plain kernel's arguments, and the terrain's (tcount 0: none)
struct GaitLaunch {
  int n, ld, count;
  const double* table;
  const double* time;
  const double* cmd;
  const uint8_t* gait_id;
  const double* scale;
  const double* start;
  double* targets;
  uint8_t* mask;
  int tcount;
  const double* ttable;
  const uint8_t* tid;
  const double* tscale;
};

inline bool gait_schedule_on(const GaitScheduleState* s) { return s && s->args.n > 0; }
// the schedule kernel for L, without or with a terrain, on the current device
int gait_schedule_launch(const GaitScheduleState* s, void* hip_stream, const GaitLaunch& L);
// the current device is the handle's and idle
void gait_schedule_free(GaitScheduleState* s);

}  // namespace wbc
