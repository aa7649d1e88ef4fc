// The per-knot instantiations of k_al_update (al_kernels.h), for windows of bounds (ilqr_hip_set_al_knot_bounds,
// ilqr_hip_set_al_state_knot_bounds, ilqr_hip_al_bounds_window_from_track, ilqr_hip_set_al_task_bounds), and the task family's shift and points kernels.  Compiled with -DAL_KNOT_MODULE into libilqr_hip_alknot.so only
// (csrc/Makefile; ilqr_kernels.h AlKnotModule says why the module exists): the library's own launch_al_update calls the entry point below
// where AlDev::bounds_knot is set.
#include <hip/hip_runtime.h>

#ifndef AL_KNOT_MODULE
#error "al_knot_kernels.hip belongs to the per-knot bounds module: compile it with -DAL_KNOT_MODULE"
#endif
#include "h1_cost_dev.h"
#include "ilqr_kernels.h"

using namespace h1;

#include "al_kernels.h"

extern "C" {
void ilqr_alknot_module_al_update(const ilqr::DevState* S, const ilqr::AlDev* A, int round, int masked, hipStream_t st);
// dyn_kernels.hip, quad_kernels.hip and al_bounds_track_kernels.hip of this module
void ilqr_alknot_module_knot_cost(const ilqr::DevState* S, const h1::ProblemDev* P, int mode, const double* xsrc, const double* usrc, int cshift, int oshift, const int* gate, hipStream_t st);
void ilqr_alknot_module_state_knot_cost(const ilqr::DevState* S, const h1::ProblemDev* P, int mode, const double* xsrc, int cshift, int oshift, const int* gate, hipStream_t st);
void ilqr_alknot_module_cost_quadratics(const ilqr::DevState* S, const h1::ProblemDev* P, int mode, const int* list, const int* count, int lower, hipStream_t st);
void ilqr_alknot_module_window_from_track(const ilqr::AlBoundsTrackDev* T, const ilqr::AlBoundsWindowDev* W, const int* start, int n_sets, int step, int N, hipStream_t st);
void ilqr_alknot_module_expand(const double* rec, long rec_stride, double* win, int width, int n_sets, int N, hipStream_t st);
void ilqr_alknot_module_task_knot_cost(const ilqr::DevState* S, const h1::ProblemDev* P, int mode, const double* xsrc, int cshift, int oshift, const int* gate, hipStream_t st);
void ilqr_alknot_module_task_shift(const ilqr::AlDev* A, int B, int N, int shift, hipStream_t st);
void ilqr_alknot_module_task_points(const ilqr::DevState* S, double* out, hipStream_t st);
void ilqr_alknot_module_task_velocities(const ilqr::DevState* S, double* out, hipStream_t st);
// plant_task_score_kernels.hip of this module
void ilqr_alknot_module_plant_task_score(const ilqr::PlantTaskScoreDev* T, int B, const double* hist_x, long hist_row0, long hist_cap, int knot0, int count, double* terms, double* record, hipStream_t st);
// the one symbol the library resolves: the table of the module's entry points (ilqr_kernels.h AlKnotModule)
const ilqr::AlKnotModule* ilqr_alknot_module() {
  static const ilqr::AlKnotModule table = {ilqr_alknot_module_knot_cost, ilqr_alknot_module_state_knot_cost, ilqr_alknot_module_cost_quadratics,
                                           ilqr_alknot_module_al_update, ilqr_alknot_module_window_from_track, ilqr_alknot_module_expand,
                                           ilqr_alknot_module_task_knot_cost, ilqr_alknot_module_task_shift, ilqr_alknot_module_task_points,
                                           ilqr_alknot_module_plant_task_score, ilqr_alknot_module_task_velocities};
  return &table;
}
}
// a state family brings a window of the joint / torque bounds with it (al_plan.h): both windows or the first alone
// ... and each of the two with the task family on top (AlDev::tbounds)
extern "C" void ilqr_alknot_module_al_update(const ilqr::DevState* S, const ilqr::AlDev* A, int round, int masked, hipStream_t st) {
  if (A->tbounds) {
    if (A->sbounds) hipLaunchKernelGGL((ilqr::k_al_update<true, true, true, true>), dim3(S->B), dim3(64), 0, st, *S, *A, round, masked);
    else hipLaunchKernelGGL((ilqr::k_al_update<true, false, true, true>), dim3(S->B), dim3(64), 0, st, *S, *A, round, masked);
  }
  else if (A->sbounds) hipLaunchKernelGGL((ilqr::k_al_update<true, true, true>), dim3(S->B), dim3(64), 0, st, *S, *A, round, masked);
  else hipLaunchKernelGGL((ilqr::k_al_update<true, false, true>), dim3(S->B), dim3(64), 0, st, *S, *A, round, masked);
}
extern "C" void ilqr_alknot_module_task_shift(const ilqr::AlDev* A, int B, int N, int shift, hipStream_t st) {
  hipLaunchKernelGGL(ilqr::k_al_task_shift, dim3(B), dim3(64), 0, st, *A, N, shift);
}
extern "C" void ilqr_alknot_module_task_points(const ilqr::DevState* S, double* out, hipStream_t st) {
  const long total = (long)S->B * (S->N + 1);
  hipLaunchKernelGGL(ilqr::k_al_task_points, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, st, *S, out);
}
extern "C" void ilqr_alknot_module_task_velocities(const ilqr::DevState* S, double* out, hipStream_t st) {
  const long total = (long)S->B * (S->N + 1);
  hipLaunchKernelGGL(ilqr::k_al_task_velocities, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, st, *S, out);
}
