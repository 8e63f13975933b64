// wbc_gait_handle.hpp -- the gait planner's handle (internal, host only, not installed): what wbc_gait.hip, wbc_gait_schedule.hip and
// wbc_gait_feedback.hip share, and what wbc_plant.hip and wbc_ground.hip read of a gait set on a plant.  The three gait files stay
// three translation units, each with its own kernels, so that every kernel's code is what its own file compiles to; their host code
// works on this one struct.  The only call that crosses them is the launch of a schedule kernel (gait_schedule_launch).
#pragma once
#include <stdint.h>

#include "../../include/wbc_gait.h"
#include "../../include/wbc_gait_feedback.h"
#include "wbc_gait.hpp"

namespace wbc {

// one wbc_gait_targets call: the arguments of the plain kernel, and the first of every other target kernel
struct GaitArgs {
  int n, ld, count;
  const double* table;   // GAIT_HEAD + count * GAIT_STRIDE doubles
  const double* time;
  const double* cmd;
  const uint8_t* gait_id;
  const double* scale;
  const double* start;
  double* targets;
  uint8_t* mask;
};

struct GaitTerrainArgs {
  int count;             // profiles in the table; 0: no terrain
  const double* table;   // GAIT_TERRAIN_HEAD + count * TERRAIN_STRIDE doubles
  const uint8_t* id;
  const double* scale;
};

struct GaitScheduleArgs {
  int n;                 // instances resolved; 0: no schedule
  int ld;                // the buffer's leading dimension in this resolution
  double beta;
  const double* knots;   // GAIT_SCHEDULE_ROWS rows of ld doubles (wbc_gait.hpp)
};

}  // namespace wbc

struct wbc_gait_s {      // wbc_gait_create value-initialises it: every pointer null, every count 0
  int device, count;
  double table[wbc::GAIT_TABLE_DOUBLES];
  double* d_table;       // allocated and filled by the first wbc_gait_set_commands
  const double* cmd;     // nullptr: no wbc_gait_set_commands yet
  const uint8_t* gait_id;
  const double* scale;
  const double* start;
  double* d_terrain;             // the packed terrain table, GAIT_TERRAIN_DOUBLES doubles, allocated by the first wbc_gait_set_terrain
  wbc::GaitTerrainArgs terrain;  // count == 0: no terrain, the plain kernel
  // command schedules (wbc_gait_schedule.hip)
  double* d_knots;               // the buffer, GAIT_SCHEDULE_ROWS x knots_capacity doubles, grown by wbc_gait_set_schedule as needed
  int knots_capacity;
  wbc::GaitScheduleArgs schedule;   // n == 0: no schedule; wbc_gait_clear_schedule keeps the buffer
  // foot-placement feedback (wbc_gait_feedback.hip)
  wbc_gait_feedback_params feedback;
  int feedback_n;                // instances; 0: no feedback
  double* d_feedback;            // GAIT_FEEDBACK_ROWS rows of 4 feedback_n doubles, then feedback_n bytes: the previous masks
};

namespace wbc {

inline bool gait_schedule_on(const wbc_gait_s& g) { return g.schedule.n > 0; }
inline bool gait_feedback_on(const wbc_gait_s& g) { return g.feedback_n > 0; }
// the schedule kernel for a, without or with the handle's terrain, on the current device (wbc_gait_schedule.hip, where the kernels are)
int gait_schedule_launch(const wbc_gait_s& g, void* hip_stream, const GaitArgs& a);

}  // namespace wbc
