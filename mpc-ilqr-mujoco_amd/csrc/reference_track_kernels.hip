// Reference windows cut from a track on the device (include/ilqr_hip.h ilqr_hip_window_from_track): the rule of
// RobotUtils::getReferenceWindow (reference src/common/robot_utils.cpp:422-443: rows t0 .. t0 + N, clamped to the last row), of
// getEEReference / getCoMVelReference (:525-549) and of isStance (:494-504: out of range -> stance), for one start row per set.
//   k_window_from_track  one workgroup per set: writes that set's six windows into the buffers the solver reads.  A pure copy -- no
//                        arithmetic on a value -- so the windows are bit for bit what the host setters upload.
// A window is a contiguous span of the track followed, past the track's end, by repeats of its last row.  The span is copied flat:
// consecutive lanes read consecutive doubles of the track and write consecutive doubles of the window, with no row index at all; the
// clamped rows are then written one row per wave, the row decided once.  The track is small (5 MB for 7840 rows) and every set reads a
// span of it: it stays in cache, and the kernel's time is its stores.  Loads and stores are 8 bytes per lane: a start row times 51
// doubles is not 16-byte aligned for odd starts, nor is a set's window for odd set indices.
// A translation unit of its own: no kernel of the solve or of the plant shares a compilation with it.
#include <hip/hip_runtime.h>

#include "reference_track_kernels.h"

namespace ilqr {

#define RT_THREADS 256
#define RT_WAVES (RT_THREADS / 64)

// dst[t][i] = src[min(s + t, rows - 1)][i] for t = 0 .. count - 1, i = 0 .. W - 1; s >= 0, rows >= 1.  Every index formed is inside
// src[rows][W] and dst[count][W] whatever s is.
template <int W>
__device__ __forceinline__ void cut_rows(double* __restrict__ dst, const double* __restrict__ src, long s, int rows, int count, int tid) {
  long held = (long)rows - s;      // rows of the window the track still holds
  held = held < 0 ? 0 : (held > count ? count : held);
  const double* span = src + (held > 0 ? s : 0) * W;
  const int ne = (int)held * W;
#pragma unroll 4
  for (int e = tid; e < ne; e += RT_THREADS) dst[e] = span[e];
  const double* last = src + (long)(rows - 1) * W;
  const int wave = tid >> 6, lane = tid & 63;
  for (int t = (int)held + wave; t < count; t += RT_WAVES)
    for (int i = lane; i < W; i += 64) dst[t * W + i] = last[i];
}

// dst[t][f] = r0 + t < contact_rows ? (contact[r0 + t][f] == 1) : 1 for t = 0 .. count - 1 (contact_rows == 0: contact is not read)
__device__ __forceinline__ void cut_stance(int* __restrict__ dst, const int* __restrict__ contact, long r0, int contact_rows, int count, int tid) {
  long held = (long)contact_rows - r0;
  held = held < 0 ? 0 : (held > count ? count : held);
  const int* span = contact + (held > 0 ? r0 : 0) * 2;
  const int ne = (int)held * 2;
  for (int e = tid; e < 2 * count; e += RT_THREADS) dst[e] = e < ne ? (span[e] == 1 ? 1 : 0) : 1;
}

// grid (n_sets): blockIdx.x = the set; its start row is one scalar load.  64-bit offsets: B (N + 1) 51 doubles pass 2^31 bytes.
__global__ void __launch_bounds__(RT_THREADS) k_window_from_track(TrackDev T, WindowDev W, const int* __restrict__ start, int sched_sets, int step, int follow, int N) {
  const int tid = threadIdx.x;
  const size_t b = blockIdx.x;
  long s = (long)start[b] + step;
  s = s < 0 ? 0 : s;
  const size_t n1 = (size_t)N + 1;
  cut_rows<51>(W.x + b * n1 * 51, T.x, s, T.rows, N + 1, tid);
  cut_rows<19>(W.u + b * (size_t)N * 19, T.u, s, T.rows, N, tid);
  cut_rows<3>(W.com + b * n1 * 3, T.com, s, T.rows, N + 1, tid);
  if (b < (size_t)sched_sets) {
    const long r0 = follow ? s : 0;
    cut_rows<6>(W.ee + b * n1 * 6, T.ee, r0, T.rows, N + 1, tid);
    cut_rows<3>(W.com_vel + b * n1 * 3, T.com_vel, r0, T.rows, N + 1, tid);
    cut_stance(W.stance + b * n1 * 2, T.contact, r0, T.contact_rows, N + 1, tid);
  }
}

void launch_window_from_track(const TrackDev& T, const WindowDev& W, const int* start, int n_sets, int sched_sets, int step, int follow, int N, hipStream_t st) {
  hipLaunchKernelGGL(k_window_from_track, dim3((unsigned)n_sets), dim3(RT_THREADS), 0, st, T, W, start, sched_sets, step, follow, N);
}

}  // namespace ilqr
