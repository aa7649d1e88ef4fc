// Windows of augmented-Lagrangian bounds written on the device (include/ilqr_hip.h ilqr_hip_al_bounds_window_from_track): the end clamp of
// the reference windows (reference_track_kernels.hip: rows s .. s + N, clamped to the last row), for one start row per set.
//   k_al_bounds_window_from_track  one workgroup per set: writes that set's windows of the given parts into the buffers the cost kernels read.
//   k_al_bounds_expand             one workgroup per set: one record repeated over the N + 1 rows of the set's window (what the library does to
//                                  a whole-horizon record of one family while the other family has a window).
// Both are pure copies -- no arithmetic on a value -- so the windows are bit for bit what the host setters upload.  Track rows and window
// rows are whole 128-byte lines (80, 64 or 32 doubles, 128-byte aligned: h1_cost_dev.h ALB_STRIDE, ALSB_STRIDE, al_task_dev.h ALTB_STRIDE): the copy runs in 16-byte
// pieces, consecutive lanes on consecutive pieces, so that eight lanes write one line and a wave eight whole lines per store instruction.
// A translation unit of its own: no kernel of the solve or of the plant shares a compilation with it.  Linked into libilqr_hip_alknot.so
// (csrc/Makefile; ilqr_kernels.h AlKnotModule), not into the library: ilqr_capi.hip calls the two entry points at the end of this file.
#include <hip/hip_runtime.h>

#include "al_bounds_track_kernels.h"

namespace ilqr {

#define ABT_THREADS 256
typedef double abt_v2d __attribute__((ext_vector_type(2)));

// dst[t][0..W) = src[clamp(s + t, 0, rows - 1)][0..W) for t = 0 .. count - 1 (W even; rows >= 1).  Every index formed is inside
// src[rows][W] and dst[count][W] whatever s is.
template <int W>
__device__ __forceinline__ void cut_bound_rows(double* __restrict__ dst, const double* __restrict__ src, long s, int rows, int count, int tid) {
  static_assert(W % 16 == 0, "whole 128-byte lines");
  constexpr int P = W / 2;      // 16-byte pieces of a row
  abt_v2d* d2 = reinterpret_cast<abt_v2d*>(dst);
  const abt_v2d* s2 = reinterpret_cast<const abt_v2d*>(src);
  for (int e = tid; e < count * P; e += ABT_THREADS) {
    const int t = e / P, i = e - t * P;
    long r = s + t;
    r = r < 0 ? 0 : (r > (long)rows - 1 ? (long)rows - 1 : r);
    d2[e] = s2[r * P + i];
  }
}

// grid (n_sets): blockIdx.x = the set; its start row is one scalar load.  64-bit offsets throughout.
__global__ void __launch_bounds__(ABT_THREADS) k_al_bounds_window_from_track(AlBoundsTrackDev T, AlBoundsWindowDev Wd, const int* __restrict__ start, int step, int N) {
  const int tid = threadIdx.x;
  const size_t b = blockIdx.x, n1 = (size_t)N + 1;
  const long s = (long)start[b] + step;
  if (T.joint_ctrl && Wd.joint_ctrl) cut_bound_rows<80>(Wd.joint_ctrl + b * n1 * 80, T.joint_ctrl, s, T.rows, N + 1, tid);
  if (T.state && Wd.state) cut_bound_rows<64>(Wd.state + b * n1 * 64, T.state, s, T.rows, N + 1, tid);
  if (T.task && Wd.task) cut_bound_rows<32>(Wd.task + b * n1 * 32, T.task, s, T.rows_task, N + 1, tid);
}

// the same copy from a "track" of one row: every window row is the set's record
__global__ void __launch_bounds__(ABT_THREADS) k_al_bounds_expand(const double* __restrict__ rec, long rec_stride, double* __restrict__ win, int width, int N) {
  const size_t b = blockIdx.x, n1 = (size_t)N + 1;
  const double* src = rec + (long)b * rec_stride;
  if (width == 80) cut_bound_rows<80>(win + b * n1 * 80, src, 0, 1, N + 1, threadIdx.x);
  else cut_bound_rows<64>(win + b * n1 * 64, src, 0, 1, N + 1, threadIdx.x);
}

void launch_al_bounds_window_from_track(const AlBoundsTrackDev& T, const AlBoundsWindowDev& W, const int* start, int n_sets, int step, int N, hipStream_t st) {
  hipLaunchKernelGGL(k_al_bounds_window_from_track, dim3((unsigned)n_sets), dim3(ABT_THREADS), 0, st, T, W, start, step, N);
}
void launch_al_bounds_expand(const double* rec, long rec_stride, double* win, int width, int n_sets, int N, hipStream_t st) {
  hipLaunchKernelGGL(k_al_bounds_expand, dim3((unsigned)n_sets), dim3(ABT_THREADS), 0, st, rec, rec_stride, win, width, N);
}

}  // namespace ilqr

extern "C" void ilqr_alknot_module_window_from_track(const ilqr::AlBoundsTrackDev* T, const ilqr::AlBoundsWindowDev* W, const int* start, int n_sets, int step, int N, hipStream_t st) {
  ilqr::launch_al_bounds_window_from_track(*T, *W, start, n_sets, step, N, st);
}
extern "C" void ilqr_alknot_module_expand(const double* rec, long rec_stride, double* win, int width, int n_sets, int N, hipStream_t st) {
  ilqr::launch_al_bounds_expand(rec, rec_stride, win, width, n_sets, N, st);
}
