// noise.h -- the counter-based sampler noise of the seeded entry points (the contract: include/flowdec_hip.h, "Seeded noise").
// z(seed, draw, f, t) is a pure function: Philox4x32-10 (Random123) keyed by the clip's 64-bit seed, counter (t >> 1, f, draw, 0);
// an even frame takes the words (r0, r1), an odd one (r2, r3); Box-Muller on u1 in (0, 1), u2 in [0, 1) gives a complex normal with
// E|z|^2 = 1.  Every kernel that inlines fd_noise_at gets the same float32 bits: integer arithmetic, the accurate logf / sqrtf /
// sincospif (sincospif(2 u2): the argument 2 u2 is exact, 2 pi u2 in float32 would not be), one rounding per product, and no
// contraction with the caller's arithmetic (the pragma below; the callers use z only as a factor or convert it first).
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned (&r)[4]) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const unsigned h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const unsigned h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

// the pair of 32-bit words of frame t (frames 2k and 2k + 1 share one Philox call)
__device__ __forceinline__ uint2 fd_noise_bits_at(unsigned long long seed, int draw, int f, int t) {
  unsigned r[4];
  philox4x32_10((unsigned)t >> 1, (unsigned)f, (unsigned)draw, 0u, (unsigned)seed, (unsigned)(seed >> 32), r);
  return (t & 1) ? uint2{r[2], r[3]} : uint2{r[0], r[1]};
}

__device__ __forceinline__ float2 fd_noise_from_bits(uint2 b) {
#pragma clang fp contract(off)
  const float u1 = ((float)(b.x >> 9) + 0.5f) * 1.1920928955078125e-07f;   // 2^-23: in (0, 1), exact
  const float u2x2 = (float)(b.y >> 8) * 1.1920928955078125e-07f;          // 2 u2 = (rb >> 8) 2^-23: in [0, 2), exact
  const float rad = sqrtf(-logf(u1));
  float s, c;
  sincospif(u2x2, &s, &c);
  return float2{rad * c, rad * s};
}

__device__ __forceinline__ float2 fd_noise_at(unsigned long long seed, int draw, int f, int t) {
  return fd_noise_from_bits(fd_noise_bits_at(seed, draw, f, t));
}

// Element i of a [B][F][T] plane of Gaussian noise: read from the caller's buffer, or (SEEDED) generated in registers from the clip's
// seed.  A thread recomputes the Philox call it shares with the neighbouring frame instead of handling a frame pair: the consumers
// (init_state / caxpy in solver_ops.hip, score_update in net_edges.hip) stay one element per thread like their unseeded forms (one grid,
// one index map), and the ~150 integer / float operations per element hide behind the 24-40 bytes each of them moves (they replace an
// 8-byte load).
// frame0 (int32 [B], may be null = zeros): the absolute frame of every row's first column (rows that are chunks of longer recordings).
template <bool SEEDED>
__device__ __forceinline__ float2 noise_elem(const float2* __restrict__ z, const unsigned long long* __restrict__ seeds, int draw, long long i,
                                             int F, int T, const int* __restrict__ frame0 = nullptr) {
  if constexpr (SEEDED) {
    const long long row = i / T;
    const long long b = row / F;
    return fd_noise_at(seeds[b], draw, (int)(row % F), (frame0 ? frame0[b] : 0) + (int)(i - row * T));
  } else {
    return z[i];
  }
}
