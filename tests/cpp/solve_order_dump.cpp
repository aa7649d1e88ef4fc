// Prints resolve_solve_order / rolls_aside / iteration_order (csrc/solve_order.h) over the combinations tests/test_solve_order_cpu.py asks for.
// Two tables, each a text line "<name> <rows> <column> <column> ...\n" followed by rows x columns int16 values (native byte order):
//   resolve    one row per combination of settings, presence flags and plan: the inputs, every field of the SolveOrder, rolls_aside(0 / 1 / 2)
//   iteration  for every distinct (SolveOrder, max_iter, B) of the first table: every iteration, pass_bound in {spec_max, spec_max + 1, 4 spec_max,
//              4 spec_max + 1, B}, both values of prev_seq -> kind, first_listed, pair
// The full cross product of all inputs is ~5e9 rows, so the first table is four blocks (column `block`), each a full cross product of some
// inputs around named bases:
//   0  every combination of the 13 switches that enter resolve_solve_order x {all buffers present, none, each one absent}, default plan, B = 4096, 10 iterations
//   1  overlap_rollout x reuse_rollout x first_aside x plan.reroll_aside x plan.cold_start_aside, both bases
//   2  every combination of the 11 presence flags x the 32 plans x 4 bases (fixed iterations / convergence exit, each with ILQR_SPLIT either way)
//   3  B in {1, 512, 513, 4096} x max_iter in {1, 2, 10} x spec_list_from in {0, 1, 4} x the 32 plans x both bases, each as it is and with each switch flipped
#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>

#include "solve_order.h"

using namespace ilqr;

namespace {
const char* const RESOLVE_COLUMNS =
    "block early_exit early_exit_gate split spec spec_dual spec_max spec_lists listed_spec spec_list_max spec_list_from dedup relin repass overlap_rollout reuse_rollout "
    "max_iter B slices analytic_jacobians first_aside lists chg chg_f kr ls_list ls_kind lgate grp_a stream_a adopt_events twin "
    "L.spec_dual L.lin_lists L.two_lane_line_search L.reroll_aside L.cold_start_aside "
    "o.sel_active o.gate o.dedup_bit o.cache o.lin_listed o.can_split o.skip_first o.retry_gated o.twin_order o.dual_order o.spec_max o.listed_wanted o.listed "
    "o.listed_from o.twin_wanted o.overlap_rollout o.reuse_rollout o.first_aside rolls_aside0 rolls_aside1 rolls_aside2";
const char* const ITERATION_COLUMNS =
    "o.sel_active o.gate o.dedup_bit o.cache o.lin_listed o.can_split o.skip_first o.retry_gated o.twin_order o.dual_order o.spec_max o.listed_wanted o.listed "
    "o.listed_from o.twin_wanted o.overlap_rollout o.reuse_rollout o.first_aside max_iter B iter pass_bound prev_seq kind first_listed pair";
constexpr int SWITCHES = 13, PRESENCE = 11, PLANS = 32;

// fixed iterations on the whole batch with every buffer, as the benchmark's headline runs; exit: the same with the convergence exit
SolveSettings base(bool exit) {
  SolveSettings s{};
  s.early_exit = exit; s.early_exit_gate = true; s.split = exit; s.spec = true; s.spec_dual = true; s.spec_max = 512; s.spec_lists = true; s.listed_spec = true;
  s.spec_list_max = 1024; s.spec_list_from = 0; s.dedup = true; s.relin = false; s.repass = false; s.overlap_rollout = true; s.reuse_rollout = false;
  s.max_iter = 10; s.B = 4096; s.slices = 1; s.analytic_jacobians = true; s.first_aside = true;
  s.lists = s.chg = s.chg_f = s.kr = s.ls_list = s.ls_kind = s.lgate = s.grp_a = s.stream_a = s.adopt_events = s.twin = true;
  return s;
}
void flip_switch(SolveSettings& s, int i) {
  bool* const b[] = {&s.early_exit, &s.early_exit_gate, &s.split, &s.spec, &s.spec_dual, &s.spec_lists, &s.listed_spec, &s.dedup, &s.relin, &s.repass, &s.analytic_jacobians};
  if (i < 11) *b[i] = !*b[i];
  else if (i == 11) s.spec_list_max = s.spec_list_max ? 0 : 1024;
  else s.slices = 3 - s.slices;
}
void flip_presence(SolveSettings& s, int i) {
  bool* const b[] = {&s.lists, &s.chg, &s.chg_f, &s.kr, &s.ls_list, &s.ls_kind, &s.lgate, &s.grp_a, &s.stream_a, &s.adopt_events, &s.twin};
  *b[i] = !*b[i];
}
// the plans differ in the five fields the order reads: bits 0 .. 4 CLEAR spec_dual, lin_lists, the two-lane line search, reroll_aside, cold_start_aside
LaunchPlan plan(int bits) {
  LaunchPlan L{};
  L.spec_dual = !(bits & 1); L.lin_lists = !(bits & 2); L.line_search = (bits & 4) ? DYN_ONE_LANE : DYN_TWO_LANE; L.reroll_aside = !(bits & 8); L.cold_start_aside = !(bits & 16);
  return L;
}

std::vector<int16_t> resolve_rows, iteration_rows;
std::set<std::vector<int16_t>> orders;

std::vector<int16_t> order_fields(const SolveOrder& o) {
  return {o.sel_active, o.gate, (int16_t)o.dedup_bit, o.cache, o.lin_listed, o.can_split, o.skip_first, o.retry_gated, o.twin_order, o.dual_order, (int16_t)o.spec_max, o.listed_wanted,
          o.listed, (int16_t)o.listed_from, o.twin_wanted, o.overlap_rollout, o.reuse_rollout, o.first_aside};
}
void row(int block, const SolveSettings& s, const LaunchPlan& L) {
  const SolveOrder o = resolve_solve_order(s, L);
  const std::vector<int16_t> in = {(int16_t)block, s.early_exit, s.early_exit_gate, s.split, s.spec, s.spec_dual, (int16_t)s.spec_max, s.spec_lists, s.listed_spec, (int16_t)s.spec_list_max,
                                   (int16_t)s.spec_list_from, s.dedup, s.relin, s.repass, s.overlap_rollout, s.reuse_rollout, (int16_t)s.max_iter, (int16_t)s.B, (int16_t)s.slices, s.analytic_jacobians,
                                   s.first_aside, s.lists, s.chg, s.chg_f, s.kr, s.ls_list, s.ls_kind, s.lgate, s.grp_a, s.stream_a, s.adopt_events, s.twin,
                                   L.spec_dual, L.lin_lists, L.line_search == DYN_TWO_LANE, L.reroll_aside, L.cold_start_aside};
  std::vector<int16_t> of = order_fields(o);
  resolve_rows.insert(resolve_rows.end(), in.begin(), in.end());
  resolve_rows.insert(resolve_rows.end(), of.begin(), of.end());
  for (int it = 0; it < 3; ++it) resolve_rows.push_back(rolls_aside(o, L, it));
  of.push_back((int16_t)s.max_iter); of.push_back((int16_t)s.B);
  if (!orders.insert(of).second) return;
  const int bounds[] = {o.spec_max, o.spec_max + 1, 4 * o.spec_max, 4 * o.spec_max + 1, s.B};
  for (int it = 0; it < s.max_iter; ++it) for (int i = 0; i < 5; ++i) for (int prev = 0; prev < 2; ++prev) {
    const int pb = bounds[i];
    if (i == 4 && (pb == bounds[0] || pb == bounds[1] || pb == bounds[2] || pb == bounds[3])) continue;      // (B is one of the thresholds: once)
    const IterationOrder io = iteration_order(o, it, pb, prev != 0);
    iteration_rows.insert(iteration_rows.end(), of.begin(), of.end());
    const int16_t tail[] = {(int16_t)it, (int16_t)pb, (int16_t)prev, (int16_t)io.kind, io.first_listed, io.pair};
    iteration_rows.insert(iteration_rows.end(), tail, tail + 6);
  }
}
void table(const char* name, const char* columns, const std::vector<int16_t>& v) {
  int n = 1;
  for (const char* p = columns; *p; ++p) n += *p == ' ';
  std::printf("%s %zu %s\n", name, v.size() / n, columns);
  std::fwrite(v.data(), sizeof(int16_t), v.size(), stdout);
}
}  // namespace

int main() {
  for (int sw = 0; sw < (1 << SWITCHES); ++sw) for (int pres = -1; pres <= PRESENCE; ++pres) {
    SolveSettings s = base(false);
    for (int i = 0; i < SWITCHES; ++i) if (sw >> i & 1) flip_switch(s, i);
    if (pres == PRESENCE) for (int i = 0; i < PRESENCE; ++i) flip_presence(s, i);      // none
    else if (pres >= 0) flip_presence(s, pres);
    row(0, s, plan(0));
  }
  for (int exit = 0; exit < 2; ++exit) for (int bits = 0; bits < 32; ++bits) {
    SolveSettings s = base(exit != 0);
    s.overlap_rollout = !(bits & 1); s.reuse_rollout = bits & 2; s.first_aside = !(bits & 4);
    row(1, s, plan(bits & 24));
  }
  for (int b = 0; b < 4; ++b) for (int pres = 0; pres < (1 << PRESENCE); ++pres) for (int p = 0; p < PLANS; ++p) {
    SolveSettings s = base((b & 1) != 0);
    if (b & 2) s.split = !s.split;
    for (int i = 0; i < PRESENCE; ++i) if (pres >> i & 1) flip_presence(s, i);
    row(2, s, plan(p));
  }
  for (int B : {1, 512, 513, 4096}) for (int mi : {1, 2, 10}) for (int from : {0, 1, 4}) for (int p = 0; p < PLANS; ++p)
  for (int exit = 0; exit < 2; ++exit) for (int f = -1; f < SWITCHES; ++f) {
    if (f == 0) continue;      // (early_exit flipped: the other base with ILQR_SPLIT flipped, which is there)
    SolveSettings s = base(exit != 0);
    s.B = B; s.max_iter = mi; s.spec_list_from = from;
    if (f > 0) flip_switch(s, f);
    row(3, s, plan(p));
  }
  table("resolve", RESOLVE_COLUMNS, resolve_rows);
  table("iteration", ITERATION_COLUMNS, iteration_rows);
  return 0;
}
