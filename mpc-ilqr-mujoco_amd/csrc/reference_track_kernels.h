// Launcher of reference_track_kernels.hip (reference windows cut from a track on the device), shared with ilqr_capi.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace ilqr {

// RobotUtils' full-length arrays on the device (x_ref_full_ ... contact_schedule_, robot_utils.cpp:281-492): `rows` >= 1 rows of each
// reference array, `contact_rows` >= 0 rows of stance flags (0: no table, contact may be null).
struct TrackDev {
  const double *x, *u, *com, *ee, *com_vel;      // [rows][51], [rows][19], [rows][3], [rows][2][3], [rows][3]
  const int* contact;                            // [contact_rows][2]
  int rows, contact_rows;
};
// the buffers the solver reads its reference sets from (ilqr_hip_ctx d_xref ...), each sized for one window per rollout
struct WindowDev {
  double *x, *u, *com, *ee, *com_vel;            // per set [N+1][51], [N][19], [N+1][3], [N+1][2][3], [N+1][3]
  int* stance;                                   // per set [N+1][2]
};
// Writes the windows of `n_sets` sets (set b: s = start[b] + step) of horizon N: x / u / com from the rows min(s + t, rows - 1), into
// consecutive sets of W.x / W.u / W.com; ee / com_vel / stance from the rows r = (follow ? s : 0) + t into `sched_sets` consecutive
// sets of W.ee / W.com_vel / W.stance -- sched_sets = n_sets with follow != 0, 1 otherwise (the rows are then the same for every set).
// start: device array of n_sets ints.  Every source row is clamped into the track whatever start and step are.
void launch_window_from_track(const TrackDev& T, const WindowDev& W, const int* start, int n_sets, int sched_sets, int step, int follow, int N, hipStream_t st);

}  // namespace ilqr
