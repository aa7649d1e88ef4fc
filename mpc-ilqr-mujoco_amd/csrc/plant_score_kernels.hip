// Closed-loop score of the device-resident plant (include/ilqr_hip.h ilqr_hip_plant_set_score): the terms of iLQR::computeTotalCost
// (reference src/ilqr/ilqr.cpp:363-518) of the trajectory the plant actually drove, accumulated per rollout behind every plant call.
//   k_plant_score_terms  one lane per (interval, rollout): the six terms of knot_cost_terms (h1_cost_dev.h) at the row the plant kernel has
//                        just appended to the history ring -- the state its control law saw, the control it reported -- against row
//                        knot0 + j of the reference window, under the scoring weights; plus the pelvis height
//   k_plant_score_add    one lane per rollout: adds the call's term rows into the record in interval order (no atomics: a fused call and
//                        its single intervals add the same numbers in the same order)
// Both read what the plant kernel of the same call wrote and are enqueued directly behind it on the handle's stream.  A translation unit
// of its own: no kernel of the solve or of the plant shares a compilation with it.
#include <hip/hip_runtime.h>

#include "h1_cost_dev.h"
#include "h1_aba_reg.h"
#include "plant_score_kernels.h"

using namespace h1;

namespace ilqr {

struct ScoreCom { DEVFN void operator()(const double* x, double* com) const { h1r::com_mj(x, com); } };

#define PS_LD H1_NX
// grid (ceil(B / 64), count): blockIdx.y = interval j of the call, blockIdx.x = a chunk of 64 consecutive rollouts -- a wave never
// straddles two intervals, so the ring row, the knot and (with shared sets) the reference rows are wave-uniform and the weights in P are
// scalar loads.  The chunk's state rows are contiguous in the ring ([row][B][51]): fetched coalesced through LDS as k_traj_knot_cost
// (dyn_kernels.hip) fetches its rows, half a wave at a time.  Lanes past B take the chunk's last rollout and store nothing.
__global__ void __launch_bounds__(64) k_plant_score_terms(ProblemDev P, int B, const double* hist_x, const double* hist_u, long hist_row0, long hist_cap, int knot0, double* terms) {
  __shared__ double xs[32 * PS_LD];     // 13 KB
  const int lane = threadIdx.x;
  const int j = blockIdx.y;
  const long row = (hist_row0 + j) % hist_cap;
  const int t = knot0 + j;
  const int first = blockIdx.x * 64;
  const int nrow = first + 64 <= B ? 64 : B - first;      // >= 1 by the grid
  const bool own = lane < nrow;
  const int b = first + (own ? lane : nrow - 1);
  const double* src = hist_x + ((size_t)row * B + first) * H1_NX;
  double x[H1_NX], u[H1_NU];
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const int r0 = 32 * half, nr = nrow - r0 < 32 ? nrow - r0 : 32;      // rows r0 .. r0 + nr of this chunk (nr <= 0: none)
    if (half) __syncthreads();
    {
      // all the loads of the half first, then the LDS writes (see k_traj_knot_cost); an element past the chunk's rows falls back to
      // the chunk's first element, which always exists
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
      for (int i = 0; i < H1_NX; ++i) x[i] = xs[(r >= 0 ? r : 0) * PS_LD + i];
    }
  }
  const double* ug = hist_u + ((size_t)row * B + b) * H1_NU;
#pragma unroll
  for (int i = 0; i < H1_NU; ++i) u[i] = ug[i];
  double c[6];
  knot_cost_terms(P, b, t, x, u, ScoreCom(), c);
  if (own) {
    double* o = terms + ((size_t)j * B + b) * PLANT_SCORE_TERMS;
#pragma unroll
    for (int k = 0; k < 6; ++k) o[k] = c[k];
    o[6] = x[2];
    o[7] = 1.0;
  }
}

// record[b] += the call's rows j = 0 .. count - 1 of rollout b, in that order; slot 6 the minimum (a NaN height is ignored), slot 7 the count
__global__ void __launch_bounds__(64) k_plant_score_add(int B, int count, const double* terms, double* record) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  double* r = record + (size_t)b * PLANT_SCORE_TERMS;
  double acc[PLANT_SCORE_TERMS];
#pragma unroll
  for (int k = 0; k < PLANT_SCORE_TERMS; ++k) acc[k] = r[k];
  for (int j = 0; j < count; ++j) {
    const double* tj = terms + ((size_t)j * B + b) * PLANT_SCORE_TERMS;
#pragma unroll
    for (int k = 0; k < 6; ++k) acc[k] += tj[k];
    const double v = tj[6], m = acc[6];
    acc[6] = v < m ? v : m;
    acc[7] += tj[7];
  }
#pragma unroll
  for (int k = 0; k < PLANT_SCORE_TERMS; ++k) r[k] = acc[k];
}

void launch_plant_score(const ProblemDev& P, int B, const double* hist_x, const double* hist_u, long hist_row0, long hist_cap, int knot0, int count, double* terms, double* record, hipStream_t st) {
  hipLaunchKernelGGL(k_plant_score_terms, dim3((unsigned)((B + 63) / 64), (unsigned)count), dim3(64), 0, st, P, B, hist_x, hist_u, hist_row0, hist_cap, knot0, terms);
  hipLaunchKernelGGL(k_plant_score_add, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, B, count, (const double*)terms, record);
}

}  // namespace ilqr
