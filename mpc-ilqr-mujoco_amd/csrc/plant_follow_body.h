// k_plant_follow of plant_kernels.hip, as source that file includes once per family -- inside namespace ilqr, behind the helpers and layouts it uses:
//   PLANT_TABLE 0  k_plant_follow: every rollout under the DynParams of the launch.  What the preprocessor leaves of this file is then the
//                  text the kernel has always had: the fast path keeps its machine code.
//   PLANT_TABLE 1  k_plant_follow_p: each rollout steps with its own record of a plant parameter table (ilqr_hip_plant_set_params) -- two
//                  more kernel arguments, RPW more rows of LDS behind the layout, plant_step_table in the place of step_any.
//   PLANT_TABLE 2  k_plant_follow_w: as 1 (it always reads a parameter record), and each rollout steps under the external wrench of its
//                  record of a wrench table (ilqr_hip_plant_set_wrench) in the intervals of the record's window -- three more kernel
//                  arguments, RPW + 1 more rows of LDS (the last one zero: the wrench outside the window), the wrench-carrying steps.
//   PLANT_TABLE 3  k_plant_follow_m: as 2, and each rollout's pelvis carries the payload of its record of a payload table
//                  (ilqr_hip_plant_set_payload) in every substep -- two more kernel arguments; the rollout has two widened disturbance rows in
//                  LDS, wrench and payload / zero wrench and payload, and a substep hands the step the offset of one of them.  wtab may be
//                  null: no wrench.
//   PLANT_TABLE 4  k_plant_follow_o: as 3 with either of wtab / mtab null or both (both null: the step of family 1), and the control law sees
//                  a MEASUREMENT of the state (ilqr_hip_plant_set_observation): one more kernel argument, the error rows dobs[count][B][51]
//                  of the call's intervals, and RPW more rows of LDS, XO = XS [+] delta_j, written in front of every control law.  Ring,
//                  alive, the guards and the step stay on the true state XS.
//   PLANT_TABLE 5  k_plant_follow_a: as 4 with dobs null as well (then the law reads XS itself), and an ACTUATOR between the law and the joints
//                  (ilqr_hip_plant_set_actuator): nine more kernel arguments and RPW more rows of LDS, UA -- in every substep the actuator stage
//                  turns the command rows US into the applied rows UA (delay line and lag state in memory, actuator_stage), and the step
//                  loads UA.  What the interval reports stays the command: it is loaded again from US at the interval's end, so no second
//                  control vector is live across the step.
//   PLANT_TABLE 6  k_plant_follow_j: as 5 with atab null as well (then the step loads the command rows US behind the guard, as family 4), and
//                  each rollout steps with the joints of its record of a joint table (ilqr_hip_plant_set_joints): two more kernel arguments
//                  and RPW more rows of LDS, JR -- ONE record of h1s::JOINT_REC doubles per rollout, staged once per launch -- whose offset
//                  the step gets beside the disturbance row's (step_any_j).  Without a wrench and a payload table the disturbance rows
//                  hold zeros: the step is the one of family 3 under no wrench and no payload.
//   PLANT_TABLE 7  k_plant_follow_t: as 6 with jtab null as well (then the step of family 5: under the disturbance rows if either table is there,
//                  else the step of family 1), and the FLOOR under each foot of a rollout has the height of its record of a terrain table
//                  (ilqr_hip_plant_set_terrain): two more kernel arguments and RPW more rows of LDS, TR -- one record of TERRAIN_REC doubles per
//                  rollout, staged once per launch.  Per substep the kernel decides the stance flags itself (terrain_stance: foot_contact at
//                  pz - floor) where the other families decide the reported ones, and hands them to the step with geom = 0: the non-inlined
//                  steps are the ones of the families below and decide nothing.
#ifndef PLANT_TABLE
#error "define PLANT_TABLE (0, 1, 2, 3, 4, 5, 6 or 7) before including plant_follow_body.h"
#endif
#if PLANT_TABLE == 7
#define K_PLANT_FOLLOW k_plant_follow_t
#define PLANT_TABLE_PARAMS , const double* ptab, int rec_stride, const double* wtab, int wr_stride, long interval0, const double* mtab, int m_stride, const double* dobs, \
                           const double* atab, int a_stride, const double* abeta, int ab_stride, const double* az, double* afifo, double* ay, double* aapplied, long substep0, \
                           const double* jtab, int j_stride, const double* ttab, int t_stride
#elif PLANT_TABLE == 6
#define K_PLANT_FOLLOW k_plant_follow_j
#define PLANT_TABLE_PARAMS , const double* ptab, int rec_stride, const double* wtab, int wr_stride, long interval0, const double* mtab, int m_stride, const double* dobs, \
                           const double* atab, int a_stride, const double* abeta, int ab_stride, const double* az, double* afifo, double* ay, double* aapplied, long substep0, \
                           const double* jtab, int j_stride
#elif PLANT_TABLE == 5
#define K_PLANT_FOLLOW k_plant_follow_a
#define PLANT_TABLE_PARAMS , const double* ptab, int rec_stride, const double* wtab, int wr_stride, long interval0, const double* mtab, int m_stride, const double* dobs, \
                           const double* atab, int a_stride, const double* abeta, int ab_stride, const double* az, double* afifo, double* ay, double* aapplied, long substep0
#elif PLANT_TABLE == 4
#define K_PLANT_FOLLOW k_plant_follow_o
#define PLANT_TABLE_PARAMS , const double* ptab, int rec_stride, const double* wtab, int wr_stride, long interval0, const double* mtab, int m_stride, const double* dobs
#elif PLANT_TABLE == 3
#define K_PLANT_FOLLOW k_plant_follow_m
#define PLANT_TABLE_PARAMS , const double* ptab, int rec_stride, const double* wtab, int wr_stride, long interval0, const double* mtab, int m_stride
#elif PLANT_TABLE == 2
#define K_PLANT_FOLLOW k_plant_follow_w
#define PLANT_TABLE_PARAMS , const double* ptab, int rec_stride, const double* wtab, int wr_stride, long interval0
#elif PLANT_TABLE
#define K_PLANT_FOLLOW k_plant_follow_p
#define PLANT_TABLE_PARAMS , const double* ptab, int rec_stride
#else
#define K_PLANT_FOLLOW k_plant_follow
#define PLANT_TABLE_PARAMS
#endif
template <int KIND, int FB>
__global__ void __launch_bounds__(64) K_PLANT_FOLLOW(DevState S, PlantDev Pl, DynParams dyn, const int* sched, long sched_stride, int geom, int substeps, int kick, int k0, int count,
                                                     long hist_row0, long hist_cap PLANT_TABLE_PARAMS) {
  extern __shared__ double lds[];
  typedef FollowLayout<FB> Lay;
  constexpr int n = PLANT_NX, m = PLANT_NU, RPW = Lay::RPW;
  const int tid = threadIdx.x;
  const int pr = tid >> 1;
  const bool side = (tid & 1) != 0;
  const int b0 = blockIdx.x * RPW;
  const bool owner = pr < RPW && b0 + pr < S.B;      // (lane pairs stay together: every flag below is the same on both lanes of a pair)
  const int b = owner ? b0 + pr : S.B - 1;
  const int N = S.N;
  h1s::HalfX h; h1s::load_half(side, Pl.x + (size_t)b * n, h);
  bool run = owner && Pl.alive[b] != 0;      // alive, as the advances would hand it from one to the next
  bool moved = false;                        // an interval of this launch ran to its end: state and stance are written back
  int st[2] = {1, 1}, st_done[2] = {1, 1};
  h1s::HalfU u;
#if PLANT_TABLE
  stage_plant_records<RPW>(S, lds + Lay::DOUBLES, b0, ptab, rec_stride);      // (once for all intervals; the fence at the head of interval 0 orders it)
#endif
#if PLANT_TABLE == 7
  constexpr int WR0 = Lay::DOUBLES + RPW * PLANT_REC;      // the rows of family 6, then the terrain records
  constexpr int XO0 = WR0 + 2 * RPW * h1s::DIST_REC;
  constexpr int UA0 = XO0 + RPW * n;
  constexpr int JR0 = UA0 + RPW * m;
  constexpr int TR0 = JR0 + RPW * h1s::JOINT_REC;
  stage_disturbance_records<RPW, true>(S, lds + WR0, b0, wtab, wr_stride, mtab, m_stride);
  if (jtab) stage_joint_records<RPW>(S, lds + JR0, b0, jtab, j_stride);      // (wave-uniform: a kernel argument)
  stage_terrain_records<RPW>(S, lds + TR0, b0, ttab, t_stride);
  const bool disturbed = wtab != nullptr || mtab != nullptr;
#elif PLANT_TABLE == 6
  constexpr int WR0 = Lay::DOUBLES + RPW * PLANT_REC;      // the rows of family 5, then the joint records
  constexpr int XO0 = WR0 + 2 * RPW * h1s::DIST_REC;
  constexpr int UA0 = XO0 + RPW * n;
  constexpr int JR0 = UA0 + RPW * m;
  stage_disturbance_records<RPW, true>(S, lds + WR0, b0, wtab, wr_stride, mtab, m_stride);
  stage_joint_records<RPW>(S, lds + JR0, b0, jtab, j_stride);
#elif PLANT_TABLE == 5
  constexpr int WR0 = Lay::DOUBLES + RPW * PLANT_REC;      // the rows of family 4, then the applied rows
  constexpr int XO0 = WR0 + 2 * RPW * h1s::DIST_REC;
  constexpr int UA0 = XO0 + RPW * n;
  stage_disturbance_records<RPW, true>(S, lds + WR0, b0, wtab, wr_stride, mtab, m_stride);
  const bool disturbed = wtab != nullptr || mtab != nullptr;      // (wave-uniform: kernel arguments)
#elif PLANT_TABLE == 4
  constexpr int WR0 = Lay::DOUBLES + RPW * PLANT_REC;      // disturbance rows as in family 3 (a null payload table stages zeros), then the observed rows
  constexpr int XO0 = WR0 + 2 * RPW * h1s::DIST_REC;
  stage_disturbance_records<RPW, true>(S, lds + WR0, b0, wtab, wr_stride, mtab, m_stride);
  const bool disturbed = wtab != nullptr || mtab != nullptr;      // (wave-uniform: kernel arguments)
#elif PLANT_TABLE == 3
  constexpr int WR0 = Lay::DOUBLES + RPW * PLANT_REC;      // disturbance rows behind the parameter rows: RPW with the wrench, RPW with a zero wrench
  stage_disturbance_records<RPW>(S, lds + WR0, b0, wtab, wr_stride, mtab, m_stride);
#elif PLANT_TABLE == 2
  constexpr int WR0 = Lay::DOUBLES + RPW * PLANT_REC;      // wrench rows behind the parameter rows, then the zero row
  stage_wrench_records<RPW>(S, lds + WR0, b0, wtab, wr_stride);
#endif
  for (int j = 0; j < count; ++j) {
    const int kt = k0 + j;
    const long hist_row = hist_cap > 0 ? (hist_row0 + j) % hist_cap : -1L;
    wave_lds_fence();      // (the previous interval is done with its policy rows and has stored its last state)
    // ---- knot kt of the policy -> LDS, consecutive lanes on consecutive doubles
    for (int r = 0; r < RPW; ++r) {
      const int br = b0 + r < S.B ? b0 + r : S.B - 1;
      const double* xb = S.xbar + ((size_t)br * (N + 1) + kt) * n;
      const double* ub = S.ubar + ((size_t)br * N + kt) * m;
      if (tid < n) lds[Lay::Base::XB + r * n + tid] = xb[tid];
      if (tid < m) lds[Lay::UB + r * m + tid] = ub[tid];
      if constexpr (FB != 0) {
        const double* Kt = S.K + ((size_t)br * N + kt) * m * n;
        for (int e = tid; e < m * n; e += 64) lds[Lay::KS + r * m * n + e] = Kt[e];
      }
    }
    // ---- the state this interval starts from, kick, the guards of main:134-137
    const bool was_alive = run;
    if (j > 0 && was_alive) h1s::load_half(side, lds + Lay::XS + pr * n, h);
    if (j == 0 && kick && was_alive) kick_half(side, h, Pl.dv + (size_t)b * H1_NV);
    bool fin = finite_half(h);
    fin = h1s::xch_flag(fin) && fin;
    run = was_alive && fin;
    if (owner && hist_row >= 0) h1s::store_half(side, h, Pl.hist_x + ((size_t)hist_row * S.B + b) * n);      // x the control law sees (after the kick); a frozen rollout logs the state it stopped in
    if (pr < RPW) h1s::store_half(side, h, lds + Lay::XS + pr * n);
    if (owner) { st[0] = sched[b * sched_stride + 2 * kt]; st[1] = sched[b * sched_stride + 2 * kt + 1]; }
    for (int k = 0; k < substeps; ++k) {
      // the lane index is opaque per substep, as in k_plant_advance (see there what it costs to lose it)
      int lane = tid; asm volatile("" : "+v"(lane));
      const bool side_t = (lane & 1) != 0;
      const int prt = lane >> 1;
      if (FB != 0 || k == 0) {
        wave_lds_fence();
#if PLANT_TABLE >= 5
        if (dobs) {      // (wave-uniform: a kernel argument) as family 4; without observation rows the law on XS itself, as families 0 to 3
          observe_rows<RPW>(S, lds + Lay::XS, dobs + (size_t)j * S.B * n, b0, lds + XO0);
          wave_lds_fence();
          control_law<FB, XO0>(S, lds, b0, kt);
        } else {
          control_law<FB>(S, lds, b0, kt);
        }
#elif PLANT_TABLE == 4
        // what the controller is told of the state: the interval's error on the rows as they stand (FB = 1: the substep's), the law on XO
        observe_rows<RPW>(S, lds + Lay::XS, dobs + (size_t)j * S.B * n, b0, lds + XO0);
        wave_lds_fence();
        control_law<FB, XO0>(S, lds, b0, kt);
#else
        control_law<FB>(S, lds, b0, kt);
#endif
        wave_lds_fence();
      }
#if PLANT_TABLE >= 6
      if (atab) {      // (wave-uniform: a kernel argument) the actuator as in family 5
        wave_lds_fence();
        actuator_stage<FB>(S, lds, b0, UA0, atab, a_stride, abeta, ab_stride, az + (size_t)j * S.B * m, afifo, ay, aapplied, substep0 + (long)j * substeps + k,
                           j == count - 1 && k == substeps - 1);
        wave_lds_fence();
      }
#elif PLANT_TABLE == 5
      // the actuator, in every substep (FB = 0: the command rows are the interval's, the delay line and the lag still move): US -> UA.  Its
      // lanes are dealt out over the RPW x 19 entries as the law's; the guard of main:162-165 acts in it, in front of the delay line
      wave_lds_fence();      // (the previous substep's readers of UA are done)
      actuator_stage<FB>(S, lds, b0, UA0, atab, a_stride, abeta, ab_stride, az + (size_t)j * S.B * m, afifo, ay, aapplied, substep0 + (long)j * substeps + k,
                         j == count - 1 && k == substeps - 1);
      wave_lds_fence();
#endif
      if (k == 0 && prt < RPW) h1s::store_half(side_t, h, lds + Lay::XK + prt * n);      // keep row (FB = 0: over xbar_k, behind its last reader)
      const int pc = prt < RPW ? prt : 0;
#if PLANT_TABLE >= 6
      load_half_u(side_t, lds + (atab ? UA0 : Lay::US) + pc * m, u);      // the applied torque, or without an actuator the command, behind the guard
      if (!atab) {
        bool ufin = finite_half_u(u);
        ufin = h1s::xch_flag(ufin) && ufin;
        if (!ufin) zero_half_u(u);      // main:162-165
      }
#elif PLANT_TABLE == 5
      load_half_u(side_t, lds + UA0 + pc * m, u);      // the APPLIED torque (guarded in the stage); the command is loaded again at the interval's end
#else
      load_half_u(side_t, lds + Lay::US + pc * m, u);
      bool ufin = finite_half_u(u);
      ufin = h1s::xch_flag(ufin) && ufin;
      if (!ufin) zero_half_u(u);      // main:162-165
#endif
      wave_lds_fence();      // (the odd lane reads the shared coordinates its partner stored at the end of the previous substep)
      if (run) {
        const h1s::LaneLds L{lds, 64, lane};
        h1s::load_half(side_t, lds + Lay::XS + prt * n, h);
#if PLANT_TABLE == 7
        // the flags of this substep, decided HERE on the state it starts from: each foot against the floor of the rollout's record in this
        // interval.  The record is read from LDS behind the opaque lane index; only the two flags leave the decision.
        if constexpr (KIND >= 1 && KIND <= 4) {
          if (geom) terrain_stance(side_t, h, lds + TR0 + pc * TERRAIN_REC, (double)(interval0 + j), st[0], st[1]);
        }
#else
        if constexpr (KIND >= 1 && KIND <= 4) {
          if (geom) h1s::geom_stance(side_t, h, st[0], st[1]);      // (reported; the step decides again behind its call boundary)
        }
#endif
#if PLANT_TABLE == 7
        // the step of the families below under the flags decided above (geom = 0): with a joint record family 6's, else family 5's
        const double* wrow = lds + WR0 + pc * h1s::DIST_REC;
        const double iv = (double)(interval0 + j);
        const int wro = (wrow[h1s::DIST_FIRST] <= iv && iv < wrow[h1s::DIST_END]) ? WR0 + pc * h1s::DIST_REC : WR0 + (RPW + pc) * h1s::DIST_REC;
        if (jtab) plant_step_table_j<KIND>(side_t, h, u, dyn, st, L, 0, lds + Lay::DOUBLES + pc * PLANT_REC, wro, JR0 + pc * h1s::JOINT_REC);
        else if (disturbed) plant_step_table<KIND, true>(side_t, h, u, dyn, st, L, 0, lds + Lay::DOUBLES + pc * PLANT_REC, wro);
        else plant_step_table<KIND>(side_t, h, u, dyn, st, L, 0, lds + Lay::DOUBLES + pc * PLANT_REC);
#elif PLANT_TABLE == 6
        // the disturbance row as in family 3 (zeros without the tables), the joint record of the rollout beside it
        const double* wrow = lds + WR0 + pc * h1s::DIST_REC;
        const double iv = (double)(interval0 + j);
        const int wro = (wrow[h1s::DIST_FIRST] <= iv && iv < wrow[h1s::DIST_END]) ? WR0 + pc * h1s::DIST_REC : WR0 + (RPW + pc) * h1s::DIST_REC;
        plant_step_table_j<KIND>(side_t, h, u, dyn, st, L, geom, lds + Lay::DOUBLES + pc * PLANT_REC, wro, JR0 + pc * h1s::JOINT_REC);
#elif PLANT_TABLE >= 4
        // without a wrench and a payload table the step of k_plant_follow_p (under the handle's own record: the plant without a table, bit
        // for bit); with either the step of k_plant_follow_m
        if (disturbed) {
          const double* wrow = lds + WR0 + pc * h1s::DIST_REC;
          const double iv = (double)(interval0 + j);
          const int wro = (wrow[h1s::DIST_FIRST] <= iv && iv < wrow[h1s::DIST_END]) ? WR0 + pc * h1s::DIST_REC : WR0 + (RPW + pc) * h1s::DIST_REC;
          plant_step_table<KIND, true>(side_t, h, u, dyn, st, L, geom, lds + Lay::DOUBLES + pc * PLANT_REC, wro);
        } else {
          plant_step_table<KIND>(side_t, h, u, dyn, st, L, geom, lds + Lay::DOUBLES + pc * PLANT_REC);
        }
#elif PLANT_TABLE == 3
        // the wrench's window as in k_plant_follow_w; the payload has none: both rows of the rollout carry it
        const double* wrow = lds + WR0 + pc * h1s::DIST_REC;
        const double iv = (double)(interval0 + j);
        const int wro = (wrow[h1s::DIST_FIRST] <= iv && iv < wrow[h1s::DIST_END]) ? WR0 + pc * h1s::DIST_REC : WR0 + (RPW + pc) * h1s::DIST_REC;
        plant_step_table<KIND, true>(side_t, h, u, dyn, st, L, geom, lds + Lay::DOUBLES + pc * PLANT_REC, wro);
#elif PLANT_TABLE == 2
        // interval interval0 + j, counted from ilqr_hip_plant_reset; the window's bounds are integers stored as doubles (end may be +inf)
        const double* wrow = lds + WR0 + pc * WRENCH_REC;
        const double iv = (double)(interval0 + j);
        const int wro = (wrow[9] <= iv && iv < wrow[10]) ? WR0 + pc * WRENCH_REC : WR0 + RPW * WRENCH_REC;
        plant_step_table<KIND, true>(side_t, h, u, dyn, st, L, geom, lds + Lay::DOUBLES + pc * PLANT_REC, wro);
#elif PLANT_TABLE
        plant_step_table<KIND>(side_t, h, u, dyn, st, L, geom, lds + Lay::DOUBLES + pc * PLANT_REC);
#else
        step_any<KIND>(side_t, h, u, dyn, st, L, geom);
#endif
        wave_lds_fence();
        h1s::store_half(side_t, h, lds + Lay::XS + prt * n);
      }
    }
    // ---- end of the interval: a rollout whose state is or became non-finite keeps the state it had, reports zero control and never runs again
    fin = finite_half(h);
    fin = h1s::xch_flag(fin) && fin;
    run = run && fin;
#if PLANT_TABLE >= 5
    {      // what the interval reports is the COMMAND of its last substep, behind the guard: the rows US still hold it
      load_half_u(side, lds + Lay::US + (pr < RPW ? pr : 0) * m, u);
      bool ufin = finite_half_u(u);
      ufin = h1s::xch_flag(ufin) && ufin;
      if (!ufin) zero_half_u(u);
    }
#endif
    if (!run) zero_half_u(u);
    if (owner && hist_row >= 0) store_half_u(side, u, Pl.hist_u + ((size_t)hist_row * S.B + b) * m);
    if (run) { moved = true; st_done[0] = st[0]; st_done[1] = st[1]; }
    else if (was_alive) {      // frozen in this interval: back to what the advance would have left in Pl.x
      if (j == 0) h1s::load_half(side, Pl.x + (size_t)b * n, h);
      else h1s::load_half(side, lds + Lay::XK + pr * n, h);
    }
  }
  if (!owner) return;
  store_half_u(side, u, Pl.u + (size_t)b * m);
  if (moved) {
    h1s::store_half(side, h, Pl.x + (size_t)b * n);
    if (!side) { Pl.stance[2 * (size_t)b] = st_done[0]; Pl.stance[2 * (size_t)b + 1] = st_done[1]; }
  }
  if (!side) Pl.alive[b] = run ? 1 : 0;
}
#undef K_PLANT_FOLLOW
#undef PLANT_TABLE_PARAMS
#undef PLANT_TABLE
