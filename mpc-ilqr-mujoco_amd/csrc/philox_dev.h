// The counter-based generator of the device-side draws: plant_kernels.hip (k_observation_draw, k_actuator_draw) and group_kernels.hip
// (k_group_perturb) include this one body, so every stream of normals in the tree comes from the same words.
#pragma once

#ifndef DEVFN
#define DEVFN __device__ __forceinline__
#endif

// Philox4x32-10 (Salmon et al., SC'11), the counter-based generator: ten rounds of two 32 x 32 -> 64 bit products, the key bumped by the
// Weyl constants between rounds.  Integer arithmetic only: every implementation gives the same words.
DEVFN void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned w[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const unsigned n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}
