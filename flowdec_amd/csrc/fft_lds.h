// fft_lds.h -- the power-of-two complex FFT in LDS that specdist.hip and segsnr.hip share: N = 2^LOG2N points of one padded row, float32,
// radix-2 decimation-in-time butterflies u +- W v, two stages per LDS pass (N / 4 four-point groups a pass; one two-point pass first where
// log2 N is odd), in place, bit-reversed order in, natural order out.  Twiddles W_N^m = (cos, -sin)(2 pi m / N), m < N / 2, from a table
// (fd_specdist_tables).  Element i sits at padi(i) = i + i / 32 (one float2 of padding per 32): the early passes, whose threads stand 4
// or 16 elements apart, would otherwise fold onto a quarter or a sixteenth of the banks.
//
// Two real signals go in as z = p + i q and come apart as P_k = (Z_k + conj Z_{N-k}) / 2, Q_k = (Z_k - conj Z_{N-k}) / 2i (fft_unpack_*).
// p == q gives P_k == Q_k BIT FOR BIT: with equal real and imaginary parts going in, Z_{N-k} is Z_k with its parts exchanged at every
// level of the decimation-in-time recursion (X_k = E_k + W^k O_k, X_{N-k} = E_{N/2-k} - W^{N/2-k} O_{N/2-k}): sums are componentwise, the
// table has W^{N/2-m} = (-re, im) of W^m exactly, and cmul below forms re = fma(wr, vr, -(wi vi)), im = fma(wr, vi, wi vr), which the
// exchange maps onto each other.  This is why the butterflies are the plain radix-2 ones, fused by two, and why cmul is written with
// explicit roundings.
//
// Around the transform: the run-time choice of LOG2N (dispatch, both files) and the reduction over the threads of one frame that leaves
// the result in all of them (frame_all, segsnr.hip).
#pragma once
#include <type_traits>

#include "common.h"

namespace fft_lds {

constexpr int MIN_LOG2N = 7, MAX_LOG2N = 12;                // the transform lengths 128 .. 4096 that dispatch() instantiates

template <int LOG2N>
struct Geo {
  static constexpr int N = 1 << LOG2N;
  static constexpr int TPF = N / 4 < 256 ? N / 4 : 256;     // threads per frame pair
  static constexpr int FPB = 256 / TPF;                     // frame pairs per workgroup of 256 threads
  static constexpr int NP = N + N / 32;                     // padded row
};

// f(std::integral_constant<int, LOG2N>()) for the run-time log2n in [MIN_LOG2N, MAX_LOG2N] (host; the callers have checked the range)
template <typename F>
inline void dispatch(int log2n, F&& f) {
  switch (log2n) {
    case 7: f(std::integral_constant<int, 7>()); break;
    case 8: f(std::integral_constant<int, 8>()); break;
    case 9: f(std::integral_constant<int, 9>()); break;
    case 10: f(std::integral_constant<int, 10>()); break;
    case 11: f(std::integral_constant<int, 11>()); break;
    default: f(std::integral_constant<int, 12>()); break;
  }
}

// The sums (and the maxima) of one frame over its TPF threads, the result in every thread of the frame: a butterfly over the frame's
// lanes of a wave (v_i + v_{i ^ o} is the same number on both sides), then the frame's waves in index order through red[wave][q].
// Every thread of the workgroup calls it.  segsnr_kernel needs the result in every thread (each divides by the frame's sums and scales
// by its peaks).  specdist_kernel deliberately does not call it: only lane 0 of a frame stores there, so it runs the same order as a
// one-sided tree without the broadcast.
template <int TPF, int Q, bool MAX>
__device__ __forceinline__ void frame_all(double (&v)[Q], double (*red)[4], int fr) {
  static_assert(Q <= 4, "red holds four quantities a wave");
  constexpr int W = TPF < 64 ? TPF : 64, WPF = TPF / W;      // lanes of a frame in one wave, waves of a frame
#pragma unroll
  for (int q = 0; q < Q; ++q) {
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) {
      const double u = __shfl_xor(v[q], o, 64);
      v[q] = MAX ? fmax(v[q], u) : v[q] + u;
    }
  }
  if (WPF > 1) {
    __syncthreads();                                          // the last readers of red are done
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int q = 0; q < Q; ++q) red[threadIdx.x >> 6][q] = v[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      double r = red[fr * WPF][q];
#pragma unroll
      for (int w = 1; w < WPF; ++w) r = MAX ? fmax(r, red[fr * WPF + w][q]) : r + red[fr * WPF + w][q];
      v[q] = r;
    }
  }
}

__device__ __forceinline__ int padi(int i) { return i + (i >> 5); }

// where sample n of a frame goes before the passes
template <int LOG2N>
__device__ __forceinline__ int bitrev_slot(int n) { return padi((int)(__brev((unsigned)n) >> (32 - LOG2N))); }

__device__ __forceinline__ float2 cmul(float2 w, float2 v) {
  return make_float2(__fmaf_rn(w.x, v.x, -__fmul_rn(w.y, v.y)), __fmaf_rn(w.x, v.y, __fmul_rn(w.y, v.x)));
}
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(__fadd_rn(a.x, b.x), __fadd_rn(a.y, b.y)); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(__fsub_rn(a.x, b.x), __fsub_rn(a.y, b.y)); }

// The passes over one row z (bit-reversed samples at padi positions, written and made visible by a __syncthreads() before the call) by
// the TPF threads lt = 0 .. TPF - 1 of its frame.  EVERY thread of the workgroup calls it (the barriers are the workgroup's); the last
// barrier is behind the last pass.
template <int LOG2N>
__device__ __forceinline__ void passes(float2* __restrict__ z, const float2* __restrict__ tw, int lt) {
  constexpr int N = Geo<LOG2N>::N, TPF = Geo<LOG2N>::TPF;
  if (LOG2N & 1) {                                            // the stage of span 1 alone: W = 1
    for (int j = lt; j < N / 2; j += TPF) {
      const int i0 = padi(2 * j), i1 = padi(2 * j + 1);
      const float2 u = z[i0], v = z[i1];
      z[i0] = cadd(u, v);
      z[i1] = csub(u, v);
    }
    __syncthreads();
  }
#pragma unroll
  for (int lh = LOG2N & 1; lh < LOG2N; lh += 2) {             // the stages of span h and 2 h in one pass
    const int h = 1 << lh;
    for (int j = lt; j < N / 4; j += TPF) {
      const int pos = j & (h - 1);
      const int base = ((j - pos) << 2) + pos;
      const int i0 = padi(base), i1 = padi(base + h), i2 = padi(base + 2 * h), i3 = padi(base + 3 * h);
      const float2 w1 = tw[pos << (LOG2N - 1 - lh)];          // W_{2h}^pos
      const float2 w2 = tw[pos << (LOG2N - 2 - lh)];          // W_{4h}^pos
      const float2 w3 = tw[(pos + h) << (LOG2N - 2 - lh)];    // W_{4h}^{pos + h}
      const float2 x0 = z[i0], x2 = z[i2];
      const float2 v1 = cmul(w1, z[i1]), v3 = cmul(w1, z[i3]);
      const float2 s0 = cadd(x0, v1), s1 = csub(x0, v1);
      const float2 q2 = cmul(w2, cadd(x2, v3)), q3 = cmul(w3, csub(x2, v3));
      z[i0] = cadd(s0, q2);
      z[i2] = csub(s0, q2);
      z[i1] = cadd(s1, q3);
      z[i3] = csub(s1, q3);
    }
    __syncthreads();
  }
}

// bin k of the signal that went in as the real part (re, im) and of the one that went in as the imaginary part, from zk = Z_k and
// zn = Z_{(N - k) mod N}
__device__ __forceinline__ float2 unpack_re(float2 zk, float2 zn) { return make_float2(0.5f * __fadd_rn(zk.x, zn.x), 0.5f * __fsub_rn(zk.y, zn.y)); }
__device__ __forceinline__ float2 unpack_im(float2 zk, float2 zn) { return make_float2(0.5f * __fadd_rn(zk.y, zn.y), 0.5f * __fsub_rn(zn.x, zk.x)); }

}  // namespace fft_lds
