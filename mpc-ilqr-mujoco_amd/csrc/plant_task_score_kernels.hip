// Task score of the device-resident plant (include/ilqr_hip.h ilqr_hip_plant_set_task_score): did the trajectory the plant actually drove obey
// the task bounds -- the CoM, the left and the right ankle origin (al_task_dev.h) against the window the handle currently holds --
// accumulated per rollout behind every plant call.
//   k_plant_task_score_terms  one lane per (interval, rollout): the nine points of the state row the plant kernel has just appended to the
//                             history ring, by al_task_points -- the double the solver's kernels and ilqr_hip_get_al_task_points form --
//                             against row knot0 + j of the window, a foot's rows off where schedule row knot0 + j has it in stance
//   k_plant_task_score_add    one lane per rollout: folds the call's term rows into the record in interval order (no atomics: a fused call
//                             and its single intervals fold the same numbers in the same order)
// Both read what the plant kernel of the same call wrote and are enqueued behind it (and behind the cost score's kernels) on the handle's
// stream.  A translation unit of its own, linked into libilqr_hip_alknot.so (csrc/Makefile): the task family cannot exist without that module.
#include <hip/hip_runtime.h>

#include "al_task_dev.h"
#include "plant_task_score_kernels.h"

using namespace h1;

namespace ilqr {

#define PTS_LD H1_NX
// grid (ceil(B / 64), count): blockIdx.y = interval j of the call, blockIdx.x = a chunk of 64 consecutive rollouts, as k_plant_score_terms
// (plant_score_kernels.hip): a wave never straddles two intervals, so the ring row and the knot of the window and schedule rows are
// wave-uniform.  The chunk's state rows are contiguous in the ring ([row][B][51]) and are fetched coalesced through LDS, half a wave at a
// time.  Lanes past B take the chunk's last rollout and store nothing.
__global__ void __launch_bounds__(64) k_plant_task_score_terms(PlantTaskScoreDev T, int B, const double* hist_x, long hist_row0, long hist_cap, int knot0, double* terms) {
#pragma clang fp contract(off)
  __shared__ double xs[32 * PTS_LD];     // 13 KB
  const int lane = threadIdx.x;
  const int j = blockIdx.y;
  const long row = (hist_row0 + j) % hist_cap;
  const int t = knot0 + j;
  const int first = blockIdx.x * 64;
  const int nrow = first + 64 <= B ? 64 : B - first;      // >= 1 by the grid
  const bool own = lane < nrow;
  const int b = first + (own ? lane : nrow - 1);
  const double* src = hist_x + ((size_t)row * B + first) * H1_NX;
  double x[H1_NX];
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const int r0 = 32 * half, nr = nrow - r0 < 32 ? nrow - r0 : 32;      // rows r0 .. r0 + nr of this chunk (nr <= 0: none)
    if (half) __syncthreads();
    {
      // all the loads of the half first, then the LDS writes; an element past the chunk's rows falls back to the chunk's first element,
      // which always exists
      const int cnt = nr * H1_NX;
      constexpr int NIT = (32 * H1_NX + 63) / 64;
      double tmp[NIT];
#pragma unroll
      for (int it = 0; it < NIT; ++it) { const int e = lane + 64 * it; tmp[it] = src[e < cnt ? r0 * H1_NX + e : 0]; }
#pragma unroll
      for (int it = 0; it < NIT; ++it) { const int e = lane + 64 * it; if (e < cnt) xs[e] = tmp[it]; }
    }
    __syncthreads();
    if ((lane >> 5) == half) {
      const int r = (own ? lane : nrow - 1) - r0;
#pragma unroll
      for (int i = 0; i < H1_NX; ++i) x[i] = xs[(r >= 0 ? r : 0) * PTS_LD + i];
    }
  }
  double p[ALT_COORDS];
  al_task_points(x, p);
  const double* bd = T.bounds + (long)b * T.bounds_stride + (long)t * T.bounds_knot;
  const int* st = T.stance + (long)b * T.stance_stride + 2 * t;
  const int stf[2] = {st[0], st[1]};
  // the violation as compares: an infinite side gives -inf, which never exceeds 0
  double V[3] = {0.0, 0.0, 0.0}, sq = 0.0;
  bool finite = true;
#pragma unroll
  for (int i = 0; i < ALT_COORDS; ++i) {
    finite = finite && __builtin_fabs(p[i]) < __builtin_inf();
    double v = 0.0;
    if (!al_task_row_off(i, stf)) {
      const double dh = p[i] - bd[ALTB_HI + i], dl = bd[ALTB_LO + i] - p[i];
      if (dh > v) v = dh;
      if (dl > v) v = dl;
    }
    if (v > V[i / 3]) V[i / 3] = v;
    sq += v * v;
  }
  if (own) {
    double* o = terms + ((size_t)j * B + b) * PLANT_TASK_SCORE_TERMS;
#pragma unroll
    for (int g = 0; g < 3; ++g) {
      o[g] = finite ? V[g] : 0.0;
      o[3 + g] = (finite && V[g] > T.tol) ? 1.0 : 0.0;
    }
    o[6] = finite ? sq : __builtin_nan("");
    o[7] = 1.0;
  }
}

// record[b] <- the call's rows j = 0 .. count - 1 of rollout b folded in, in that order: slots 0..2 the maximum, the rest sums
__global__ void __launch_bounds__(64) k_plant_task_score_add(int B, int count, const double* terms, double* record) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  double* r = record + (size_t)b * PLANT_TASK_SCORE_TERMS;
  double acc[PLANT_TASK_SCORE_TERMS];
#pragma unroll
  for (int k = 0; k < PLANT_TASK_SCORE_TERMS; ++k) acc[k] = r[k];
  for (int j = 0; j < count; ++j) {
    const double* tj = terms + ((size_t)j * B + b) * PLANT_TASK_SCORE_TERMS;
#pragma unroll
    for (int k = 0; k < 3; ++k) { const double v = tj[k]; if (v > acc[k]) acc[k] = v; }
#pragma unroll
    for (int k = 3; k < PLANT_TASK_SCORE_TERMS; ++k) acc[k] += tj[k];
  }
#pragma unroll
  for (int k = 0; k < PLANT_TASK_SCORE_TERMS; ++k) r[k] = acc[k];
}

void launch_plant_task_score(const PlantTaskScoreDev& T, int B, const double* hist_x, long hist_row0, long hist_cap, int knot0, int count, double* terms, double* record, hipStream_t st) {
  hipLaunchKernelGGL(k_plant_task_score_terms, dim3((unsigned)((B + 63) / 64), (unsigned)count), dim3(64), 0, st, T, B, hist_x, hist_row0, hist_cap, knot0, terms);
  hipLaunchKernelGGL(k_plant_task_score_add, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, B, count, (const double*)terms, record);
}

}  // namespace ilqr

extern "C" void ilqr_alknot_module_plant_task_score(const ilqr::PlantTaskScoreDev* T, int B, const double* hist_x, long hist_row0, long hist_cap, int knot0, int count, double* terms, double* record, hipStream_t st) {
  ilqr::launch_plant_task_score(*T, B, hist_x, hist_row0, hist_cap, knot0, count, terms, record, st);
}
