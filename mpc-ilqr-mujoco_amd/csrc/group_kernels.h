// Solve groups (include/ilqr_hip.h ilqr_hip_set_groups; group_kernels.hip): a batch B = M G is cut into M groups of G consecutive rollouts that
// solve one problem from G starts.  Three kernels, in a module of their own (libilqr_hip_groups.so, csrc/Makefile), which the C API opens on
// first use as it opens the per-knot module; group state lives in the handle and travels in these arguments, never in ProblemDev.
// Host-only declarations: ilqr_capi.hip includes this without a kernel.
#pragma once

#include <hip/hip_runtime.h>

namespace ilqr {

// What k_group_adopt copies: per-rollout slabs, each `bytes` per rollout from `base` (rollout b at base + b bytes), bytes a multiple of 4.  The work
// of all slabs is one run of chunks -- slab i owns the chunks chunk0[i] .. chunk0[i + 1] - 1, GROUP_CHUNK_PAIRS 16-byte pieces each.
constexpr int GROUP_SLABS_MAX = 16;
constexpr int GROUP_ADOPT_THREADS = 256;
constexpr int GROUP_ADOPT_UNROLL = 4;
constexpr int GROUP_CHUNK_PAIRS = GROUP_ADOPT_THREADS * GROUP_ADOPT_UNROLL;
struct GroupSlabs {
  char* base[GROUP_SLABS_MAX];
  unsigned bytes[GROUP_SLABS_MAX];
  unsigned chunk0[GROUP_SLABS_MAX + 1];
  int n;
};
// chunks of a slab of `bytes` per rollout: doubles in pairs (one more piece than pairs: a rollout 8 bytes off a 16-byte boundary has a single
// double at either end), anything else in 4-byte words
inline unsigned group_slab_chunks(unsigned bytes) {
  const unsigned pieces = (bytes & 7u) ? bytes / 4u : bytes / 16u + 1u;
  return (pieces + GROUP_CHUNK_PAIRS - 1) / GROUP_CHUNK_PAIRS;
}
// appends a slab (null base or no bytes: nothing); false: the table is full
inline bool group_slabs_add(GroupSlabs& T, void* base, size_t bytes) {
  if (!base || !bytes) return true;
  if (T.n >= GROUP_SLABS_MAX) return false;
  T.base[T.n] = (char*)base; T.bytes[T.n] = (unsigned)bytes;
  T.chunk0[T.n + 1] = T.chunk0[T.n] + group_slab_chunks((unsigned)bytes);
  ++T.n;
  return true;
}

// the perturbation as the kernel reads it: sigma [rows][19] on the device, rows 1 or G
struct GroupPerturbDev {
  const double* sigma;
  int rows, hold;
  unsigned long long seed, stream0, draw;
};

// the module's entry points (C linkage, ilqr_groups_module_<name>; ilqr_groups_module() returns this table of them)
struct GroupModule {
  void (*select)(const double* key, int B, int G, int* winner, double* rec, hipStream_t st);
  void (*adopt)(const GroupSlabs* T, const int* winner, int B, int G, hipStream_t st);
  void (*perturb)(double* ubar, const GroupPerturbDev* Pd, int B, int N, int G, hipStream_t st);
};

}  // namespace ilqr
