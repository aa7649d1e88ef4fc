// Launcher of plant_task_score_kernels.hip (the task score of the device-resident plant), shared with ilqr_capi.hip through the per-knot
// module's table (ilqr_kernels.h AlKnotModule::plant_task_score).
#pragma once
#include <hip/hip_runtime.h>

namespace ilqr {

#define PLANT_TASK_SCORE_TERMS 8      // doubles per rollout of the record and of a term row (include/ilqr_hip.h ILQR_PLANT_TASK_SCORE_TERMS)
// What the kernels read besides the ring: the task window the handle currently holds and the contact schedule (h1_cost_dev.h ProblemDev::altb,
// altb_stride, altb_knot, stance, stance_stride: the same values).  bounds: rows of ALTB_STRIDE doubles, row t of rollout b at
// b * bounds_stride + t * bounds_knot; stance: the flags of knot t of rollout b at b * stance_stride + 2 t.
struct PlantTaskScoreDev {
  const double* bounds; long bounds_stride, bounds_knot;
  const int* stance; long stance_stride;
  double tol;
};
// Scores the `count` ring rows (hist_row0 + j) % hist_cap, j = 0 .. count - 1, of hist_x [hist_cap][B][51] against the window rows and schedule
// rows knot0 + j (<= N), into terms [count][B][8], and adds them to record [B][8] in interval order.  count <= hist_cap: every row still
// holds what its interval wrote.
void launch_plant_task_score(const PlantTaskScoreDev& T, int B, const double* hist_x, long hist_row0, long hist_cap, int knot0, int count, double* terms, double* record, hipStream_t st);

}  // namespace ilqr
