// Counter-based Philox4x32-10 noise shared by the device samplers (sample.hip: word sampling, sbs.hip: stochastic beam search).
// Counter (v / 4, step, row, 0), key = the 64-bit seed, word v % 4 for token v; tests/samplerref.py restates it on the host.
// The last counter word names the stream: 0 the word draws, 1 the scheduled-sampling coin, 0 .. 31 the sampled-node beam's draw
// index, 0x41524954 the lattice shifts of arithmetic sampling (arith.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC 2011)
static __device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t lo0 = 0xD2511F53u * c[0], hi0 = __umulhi(0xD2511F53u, c[0]);
    const uint32_t lo1 = 0xCD9E8D57u * c[2], hi1 = __umulhi(0xCD9E8D57u, c[2]);
    const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
    c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}
// 32 random bits -> u in the open interval (0, 1): the odd multiples of 2^-24 below 1 (exact in fp32)
static __device__ __forceinline__ float sample_uniform(uint32_t x) { return (float)(((x >> 9) << 1) | 1u) * 5.9604644775390625e-08f; }
static __device__ __forceinline__ float sample_gumbel(uint32_t x) { return -logf(-logf(sample_uniform(x))); }
