// Launchers of al_bounds_track_kernels.hip (windows of augmented-Lagrangian bounds written on the device), shared with ilqr_capi.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace ilqr {

// The bounds track on the device (ilqr_hip_set_al_bounds_track): `rows` >= 1 records per given part, in the padded layouts of the window
// records (h1_cost_dev.h: ALB_STRIDE = 80 doubles of joint / torque bounds, ALSB_STRIDE = 64 doubles of state bounds).  A part that was
// not given is null.  The task part (ilqr_hip_set_al_task_bounds_track; al_task_dev.h: rows of ALTB_STRIDE = 32 doubles) is a track of its
// own with its own row count.
struct AlBoundsTrackDev {
  const double* joint_ctrl;      // [rows][80] or null
  const double* state;           // [rows][64] or null
  int rows;
  const double* task;            // [rows_task][32] or null.  Appended: nothing above moves
  int rows_task;
};
// the window buffers the cost kernels read (ilqr_hip_ctx AlFamily::window), each sized for one window per rollout
struct AlBoundsWindowDev {
  double* joint_ctrl;            // per set [N+1][80]
  double* state;                 // per set [N+1][64]
  double* task;                  // per set [N+1][32]
};
// Writes, for each of `n_sets` sets (set b: s = start[b] + step) and t = 0..N, row min(s + t, rows - 1) of each given part of the track
// (rows_task - 1 for the task part) into row t of set b's window of that part.  start: device array of n_sets ints.  Every row index is clamped into [0, rows - 1] whatever start
// and step are; a part whose track or window pointer is null is skipped.  A pure copy.
void launch_al_bounds_window_from_track(const AlBoundsTrackDev& T, const AlBoundsWindowDev& W, const int* start, int n_sets, int step, int N, hipStream_t st);
// Expands one record per set into a window of N + 1 equal rows: win[b][t][0..width) = rec[b * rec_stride + 0..width) for b < n_sets, t = 0..N
// (width = 80 or 64 doubles; rec_stride 0: one record for every set).  A pure copy.
void launch_al_bounds_expand(const double* rec, long rec_stride, double* win, int width, int n_sets, int N, hipStream_t st);

}  // namespace ilqr
