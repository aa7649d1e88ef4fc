// Solve groups (include/ilqr_hip.h ilqr_hip_set_groups): the batch as M groups of G consecutive rollouts that solve one problem from G starts.
//   k_group_perturb  adds sigma o z to the controls of the members g >= 1 (member 0, the incumbent, is never touched)
//   k_group_select   the member with the smallest finite key per group, ties to the lowest index
//   k_group_adopt    the winner's solution state copied over the other members of its group, slab by slab: a streaming copy, no arithmetic
// A translation unit and a module of its own (libilqr_hip_groups.so, csrc/Makefile): no kernel of the solve or of the plant shares a
// compilation with it.  ilqr_capi.hip calls the entry points at the end of this file through the table ilqr_groups_module() returns.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>

#include "group_kernels.h"
#include "philox_dev.h"

namespace ilqr {

#define GRP_NU 19
typedef double grp_v2d __attribute__((ext_vector_type(2)));

// ---- perturb.  One lane per (rollout, Philox block): block k of rollout b -- counter (stream lo, stream hi, draw, k), key (seed lo, seed hi), stream =
// stream0 + b -- yields the normals 2k and 2k + 1 of the rollout's sequence by the Box-Muller construction of k_observation_draw (plant_kernels.hip);
// normal i = seg 19 + j belongs to actuator j in the knots seg hold .. seg hold + hold - 1.  The product sigma z is rounded on its own and then
// added (__dmul_rn / __dadd_rn: never a fused multiply-add).  A sigma of exactly zero writes nothing, so the controls keep their bits (a -0.0 too).
__global__ void __launch_bounds__(256) k_group_perturb(double* __restrict__ ubar, GroupPerturbDev Pd, int B, int N, int G) {
  const int segs = (N + Pd.hold - 1) / Pd.hold;
  const int normals = segs * GRP_NU, blocks = (normals + 1) / 2;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)B * blocks) return;
  const int b = (int)(idx / blocks), k = (int)(idx - (long)b * blocks);
  const int g = b % G;
  if (g == 0) return;
  const unsigned long long s = Pd.stream0 + (unsigned long long)b;
  unsigned w[4];
  philox4x32_10((unsigned)s, (unsigned)(s >> 32), (unsigned)Pd.draw, (unsigned)k, (unsigned)Pd.seed, (unsigned)(Pd.seed >> 32), w);
  const double u1 = ((double)((((unsigned long long)w[0] << 32) | w[1]) >> 11) + 0.5) * 0x1p-53;
  const double u2 = ((double)((((unsigned long long)w[2] << 32) | w[3]) >> 11) + 0.5) * 0x1p-53;
  const double rad = sqrt(-2.0 * log(u1));
  const double ang = 6.283185307179586 * u2;
  double sn, cs;
  sincos(ang, &sn, &cs);
  const double z0 = rad * cs, z1 = rad * sn;
  const double* sig = Pd.sigma + (size_t)(Pd.rows == 1 ? 0 : g) * GRP_NU;
  double* ub = ubar + (size_t)b * N * GRP_NU;
  for (int e = 0; e < 2; ++e) {
    const int i = 2 * k + e;
    if (i >= normals) break;
    const int seg = i / GRP_NU, j = i - seg * GRP_NU;
    const double sg = sig[j];
    if (sg == 0.0) continue;
    const double p = __dmul_rn(sg, e ? z1 : z0);
    const int t1 = (seg + 1) * Pd.hold < N ? (seg + 1) * Pd.hold : N;
    for (int t = seg * Pd.hold; t < t1; ++t) ub[(size_t)t * GRP_NU + j] = __dadd_rn(ub[(size_t)t * GRP_NU + j], p);
  }
}

// ---- select.  One lane per member; the order is lexicographic on (key', index) with key' = key where it is finite and +inf elsewhere: a finite key
// beats every other, equal keys go to the lower index, and a group without a finite key goes to its lowest index, member 0.  Reduced across the
// lanes with __shfl_xor -- no atomics, nothing that depends on the grid.  SEG = G where G divides 64 (64 / G groups per wave, the butterfly
// stays inside aligned runs of G lanes), else SEG = 64: one group per wave, each lane folding the members lane, lane + 64, ... first.
struct GrpBest { double key; int idx; double count, top; };
__device__ __forceinline__ void grp_fold(GrpBest& a, double key, int idx, double count, double top) {
  if (key < a.key || (key == a.key && idx < a.idx)) { a.key = key; a.idx = idx; }
  a.count += count;
  a.top = top > a.top ? top : a.top;
}
__global__ void __launch_bounds__(256) k_group_select(const double* __restrict__ key, int B, int G, int* __restrict__ winner, double* __restrict__ rec) {
  const int M = B / G;
  const int lane = threadIdx.x & 63, wave = blockIdx.x * 4 + (threadIdx.x >> 6);
  const bool packed = (64 % G) == 0;
  const int seg = packed ? G : 64;
  const int m = packed ? wave * (64 / G) + lane / G : wave;
  GrpBest best{HUGE_VAL, INT_MAX, 0.0, -HUGE_VAL};
  if (m < M)
    for (int g = packed ? lane % G : lane; g < G; g += 64) {
      const double kv = key[(size_t)m * G + g];
      const bool fin = isfinite(kv);
      grp_fold(best, fin ? kv : HUGE_VAL, m * G + g, fin ? 1.0 : 0.0, fin ? kv : -HUGE_VAL);
    }
  for (int off = 1; off < seg; off <<= 1) {
    const double ok = __shfl_xor(best.key, off), oc = __shfl_xor(best.count, off), ot = __shfl_xor(best.top, off);
    const int oi = __shfl_xor(best.idx, off);
    grp_fold(best, ok, oi, oc, ot);
  }
  if (m < M && (lane % seg) == 0) {
    // (a group of lanes whose members all lie past G holds INT_MAX: not reachable, member 0 is always folded in)
    const int wdx = (best.idx >= m * G && best.idx < m * G + G) ? best.idx : m * G;
    winner[m] = wdx;
    rec[4 * (size_t)m + 0] = key[wdx];
    rec[4 * (size_t)m + 1] = key[(size_t)m * G];
    rec[4 * (size_t)m + 2] = best.count;
    rec[4 * (size_t)m + 3] = best.count > 0.0 ? best.top : __longlong_as_double(0x7FF8000000000000LL);
  }
}

// ---- adopt.  grid (chunks of all slabs, groups), 256 lanes, no LDS.  A workgroup finds its slab in the by-value table, reads its chunk of the
// winner's rollout ONCE into registers and stores it to the other G - 1 members of the group.
// Slabs of doubles move in 16-byte pieces.  A rollout of n doubles whose slab starts on a 16-byte boundary (parity 0) is the pieces (2i, 2i + 1)
// and, n odd, the single double n - 1; one that starts 8 bytes off (parity 1: every second rollout of a slab with an odd n -- xbar at N = 6, 357
// doubles; the gains [N][19][51] at odd N, 24225 doubles at N = 25) is the single double 0, the pieces (2i - 1, 2i) and, n even, the single n - 1.
// Lane i therefore holds the three doubles a = s[2i - 1], b = s[2i], c = s[2i + 1] of the winner -- one 16-byte load on the winner's own parity
// and, only where the slab mixes parities, one 8-byte load of the third, which hits the line the neighbour lane has just fetched -- and stores
// (b, c) to a member of parity 0 and (a, b) to a member of parity 1, 16 bytes either way; i runs over 0 .. n / 2.  Slabs of 4-byte words (the
// iteration counts, the done flags) move word by word.  Every index formed lies inside [0, n) of a rollout of the group, and the group inside
// the batch: the winner is checked against its group before anything is read.
__global__ void __launch_bounds__(GROUP_ADOPT_THREADS) k_group_adopt(GroupSlabs T, const int* __restrict__ winner, int G, int m0) {
  const int m = m0 + (int)blockIdx.y;
  const int w = winner[m];
  if (w < m * G || w >= m * G + G) return;
  int s = 0;
  while (s + 1 < T.n && blockIdx.x >= T.chunk0[s + 1]) ++s;
  const unsigned bytes = T.bytes[s];
  const unsigned piece0 = (blockIdx.x - T.chunk0[s]) * GROUP_CHUNK_PAIRS + threadIdx.x;
  char* const base = T.base[s];
  const char* const srcb = base + (size_t)w * bytes;
  if (bytes & 7u) {
    const unsigned words = bytes / 4u;
    const unsigned* src = (const unsigned*)srcb;
#pragma clang loop unroll(disable) vectorize(disable)
    for (unsigned i = piece0; i < words && i < piece0 + GROUP_CHUNK_PAIRS; i += GROUP_ADOPT_THREADS) {
      const unsigned v = src[i];
#pragma clang loop unroll(disable) vectorize(disable)
      for (int g = 0; g < G; ++g)
        if (m * G + g != w) ((unsigned*)(base + (size_t)(m * G + g) * bytes))[i] = v;
    }
    return;
  }
  const unsigned n = bytes / 8u;      // (a rollout's doubles and every index below fit 32 bits: bytes does)
  const double* src = (const double*)srcb;
  const bool ps = (((uintptr_t)srcb >> 3) & 1u) != 0;
  const bool mixed = (bytes & 8u) != 0;
  // (a rolled loop over the lane's pieces: three doubles live at a time, the register count stays at full occupancy)
#pragma clang loop unroll(disable) vectorize(disable)
  for (int u = 0; u < GROUP_ADOPT_UNROLL; ++u) {
    const unsigned e = 2u * (piece0 + (unsigned)u * GROUP_ADOPT_THREADS);      // the even double of the piece: a = s[e - 1], b = s[e], c = s[e + 1]
    if (e > n) break;
    double a = 0.0, b = 0.0, c = 0.0;
    if (!ps) {
      if (e + 1 < n) { const grp_v2d v = *(const grp_v2d*)(src + e); b = v.x; c = v.y; }
      else if (e < n) b = src[e];
      if (mixed && e >= 2) a = src[e - 1];
    } else {
      if (e >= 2 && e < n) { const grp_v2d v = *(const grp_v2d*)(src + e - 1); a = v.x; b = v.y; }
      else if (e >= 2) a = src[e - 1];
      else if (n > 0) b = src[0];
      if (mixed && e + 1 < n) c = src[e + 1];
    }
#pragma clang loop unroll(disable) vectorize(disable)
    for (int g = 0; g < G; ++g) {
      if (m * G + g == w) continue;
      char* const dstb = base + (size_t)(m * G + g) * bytes;
      double* dst = (double*)dstb;
      if ((((uintptr_t)dstb >> 3) & 1u) == 0) {
        if (e + 1 < n) { grp_v2d v; v.x = b; v.y = c; *(grp_v2d*)(dst + e) = v; }
        else if (e < n) dst[e] = b;
      } else {
        if (e >= 2 && e < n) { grp_v2d v; v.x = a; v.y = b; *(grp_v2d*)(dst + e - 1) = v; }
        else if (e >= 2) dst[e - 1] = a;
        else if (n > 0) dst[0] = b;
      }
    }
  }
}

}  // namespace ilqr

extern "C" {
void ilqr_groups_module_select(const double* key, int B, int G, int* winner, double* rec, hipStream_t st) {
  const int M = B / G;
  const int waves = (64 % G) == 0 ? (M + 64 / G - 1) / (64 / G) : M;
  hipLaunchKernelGGL(ilqr::k_group_select, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, key, B, G, winner, rec);
}
void ilqr_groups_module_adopt(const ilqr::GroupSlabs* T, const int* winner, int B, int G, hipStream_t st) {
  if (T->n < 1 || G < 2) return;
  const int M = B / G;      // (the grid's y extent holds 65535 groups: more take another launch)
  for (int m0 = 0; m0 < M; m0 += 65535)
    hipLaunchKernelGGL(ilqr::k_group_adopt, dim3(T->chunk0[T->n], (unsigned)(M - m0 < 65535 ? M - m0 : 65535)), dim3(ilqr::GROUP_ADOPT_THREADS), 0, st, *T, winner, G, m0);
}
void ilqr_groups_module_perturb(double* ubar, const ilqr::GroupPerturbDev* Pd, int B, int N, int G, hipStream_t st) {
  const int segs = (N + Pd->hold - 1) / Pd->hold;
  const long lanes = (long)B * ((segs * GRP_NU + 1) / 2);
  hipLaunchKernelGGL(ilqr::k_group_perturb, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, ubar, *Pd, B, N, G);
}
// the one symbol the library resolves: the table of the module's entry points (group_kernels.h GroupModule)
const ilqr::GroupModule* ilqr_groups_module() {
  static const ilqr::GroupModule table = {ilqr_groups_module_select, ilqr_groups_module_adopt, ilqr_groups_module_perturb};
  return &table;
}
}
