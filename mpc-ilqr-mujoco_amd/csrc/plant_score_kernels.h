// Launcher of plant_score_kernels.hip (the closed-loop score of the device-resident plant), shared with ilqr_capi.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace h1 {
struct ProblemDev;
}  // namespace h1

namespace ilqr {

#define PLANT_SCORE_TERMS 8      // doubles per rollout of the record and of a term row (include/ilqr_hip.h ILQR_PLANT_SCORE_TERMS)
// Scores the `count` ring rows (hist_row0 + j) % hist_cap, j = 0 .. count - 1, of hist_x [hist_cap][B][51] / hist_u [hist_cap][B][19]
// against the rows knot0 + j (< P.N) of P's reference sets under P's shared weights (P.wsets is not read), into terms [count][B][8],
// and adds them to record [B][8] in interval order.  count <= hist_cap: every row still holds what its interval wrote.
void launch_plant_score(const h1::ProblemDev& P, int B, const double* hist_x, const double* hist_u, long hist_row0, long hist_cap, int knot0, int count, double* terms, double* record, hipStream_t st);

}  // namespace ilqr
