// Stand-alone A/B of the two slice kernels of the bounded-lag cross-correlation (csrc/xcorr.hip): plain v_fma_f64 from LDS (8 lags per
// thread as ascending fma chains over a register window of b; not kept) against the v_mfma_f64_16x16x4_f64 mapping A[i][k] = a[s + k - i],
// B[k][j] = b[s + k + 16 j] (the library's).  Eight ragged pairs of about 4 s at 48 kHz, integer data: both must give the same c bit for
// bit, and 41 lags of three pairs are checked against a plain loop on the host.  Prints the best of three timed launches of each.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-slp-vectorize scripts/xcorr_variants.hip -o scripts/bin/xcorr_variants
// -> profiles/xcorr_variants.txt, MEASUREMENTS.md "Alignment"
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) double f64x4;

constexpr int LAGS = 8, LAG_TILE = 2048, CHUNK = 2048, SLICE = 16 * CHUNK;

#define CK(e)                                                                          \
  do {                                                                                 \
    hipError_t _e = (e);                                                               \
    if (_e != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(_e), __LINE__); exit(2); } \
  } while (0)

__device__ __forceinline__ int clip_len(const int* lens, int b, int L) {
  const int l = lens[b];
  return l < 0 ? 0 : (l > L ? L : l);
}

__global__ __launch_bounds__(256) void fma_kernel(const float* __restrict__ a, const float* __restrict__ bsig, const int* __restrict__ lens_a,
                                                  const int* __restrict__ lens_b, int La, int Lb, int M, int slices, double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float sa[CHUNK];
  __shared__ __attribute__((aligned(16))) float sb[CHUNK + LAG_TILE];
  const int j = blockIdx.x, tile = blockIdx.y, b = blockIdx.z, t = threadIdx.x;
  const long long la = clip_len(lens_a, b, La), lb = clip_len(lens_b, b, Lb);
  const long long slice_lo = (long long)j * SLICE;
  if (slice_lo >= la) return;
  const long long W = 2LL * M + 1;
  const long long l0 = -(long long)M + (long long)tile * LAG_TILE;
  const long long n_first = l0 + LAG_TILE - 1 < 0 ? -(l0 + LAG_TILE - 1) : 0;
  const long long n_end = la < lb - l0 ? la : lb - l0;
  const float* arow = a + (size_t)b * La;
  const float* brow = bsig + (size_t)b * Lb;
  double acc[LAGS];
#pragma unroll
  for (int r = 0; r < LAGS; ++r) acc[r] = 0.0;
  for (int c = 0; c < SLICE / CHUNK; ++c) {
    const long long n0 = slice_lo + (long long)c * CHUNK;
    if (n0 >= n_end) break;
    if (n0 + CHUNK <= n_first) continue;
    __syncthreads();
    for (int i = t; i < CHUNK; i += 256) { const long long n = n0 + i; sa[i] = n < la ? arow[n] : 0.f; }
    for (int i = t; i < CHUNK + LAG_TILE; i += 256) { const long long m = n0 + l0 + i; sb[i] = (m >= 0 && m < lb) ? brow[m] : 0.f; }
    __syncthreads();
    const float* wb = sb + LAGS * t;
    double w[2 * LAGS];
    {
      const f32x4 v0 = *reinterpret_cast<const f32x4*>(wb), v1 = *reinterpret_cast<const f32x4*>(wb + 4);
#pragma unroll
      for (int q = 0; q < 4; ++q) { w[q] = (double)v0[q]; w[4 + q] = (double)v1[q]; }
    }
#pragma unroll 2
    for (int k = 0; k < CHUNK; k += 8) {
      const f32x4 a0 = *reinterpret_cast<const f32x4*>(sa + k), a1 = *reinterpret_cast<const f32x4*>(sa + k + 4);
      const f32x4 b0 = *reinterpret_cast<const f32x4*>(wb + k + 8), b1 = *reinterpret_cast<const f32x4*>(wb + k + 12);
#pragma unroll
      for (int q = 0; q < 4; ++q) { w[8 + q] = (double)b0[q]; w[12 + q] = (double)b1[q]; }
      double av[8];
#pragma unroll
      for (int q = 0; q < 4; ++q) { av[q] = (double)a0[q]; av[4 + q] = (double)a1[q]; }
#pragma unroll
      for (int s = 0; s < 8; ++s) {
#pragma unroll
        for (int r = 0; r < LAGS; ++r) acc[r] = fma(av[s], w[s + r], acc[r]);
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) w[q] = w[8 + q];
    }
  }
  double* out = part + ((size_t)b * slices + j) * (size_t)W;
#pragma unroll
  for (int r = 0; r < LAGS; ++r) {
    const long long idx = (long long)tile * LAG_TILE + LAGS * t + r;
    if (idx < W) out[idx] = acc[r];
  }
}

// MFMA form.  A step s covers, for the lag offset i = 0 .. 15 inside a block of 16 lags, the samples n = s - i .. s - i + 3: the slice of
// offset i is [j SLICE - i, (j + 1) SLICE - i), so a clip has ceil((la + 15) / SLICE) slices.  Wave w owns the lags 512 w .. 512 w + 511 of
// the tile as two 256-lag blocks (lag 16 j + i of a block sits in lane j + 16 (i & 3), register i >> 2).
constexpr int APAD = 16;
__global__ __launch_bounds__(256) void mfma_kernel(const float* __restrict__ a, const float* __restrict__ bsig, const int* __restrict__ lens_a,
                                                   const int* __restrict__ lens_b, int La, int Lb, int M, int slices, double* __restrict__ part) {
  __shared__ float sa[CHUNK + APAD];            // sa[i] = a[n0 - APAD + i]
  __shared__ float sb[CHUNK + LAG_TILE];        // sb[i] = b[n0 + l0 + i]
  const int j = blockIdx.x, tile = blockIdx.y, b = blockIdx.z, t = threadIdx.x;
  const long long la = clip_len(lens_a, b, La), lb = clip_len(lens_b, b, Lb);
  const long long slice_lo = (long long)j * SLICE;
  if (slice_lo >= la + 15) return;
  const long long W = 2LL * M + 1;
  const long long l0 = -(long long)M + (long long)tile * LAG_TILE;
  const long long n_first = l0 + LAG_TILE - 1 < 0 ? -(l0 + LAG_TILE - 1) : 0;
  const long long n_end = la < lb - l0 ? la : lb - l0;
  const float* arow = a + (size_t)b * La;
  const float* brow = bsig + (size_t)b * Lb;
  const int lane = t & 63, wv = t >> 6;
  const int lo = lane & 15, hi = lane >> 4;     // A: row i = lo, k = hi;  B: col j = lo, k = hi
  f64x4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
  for (int c = 0; c < SLICE / CHUNK; ++c) {
    const long long n0 = slice_lo + (long long)c * CHUNK;
    if (n0 - 15 >= n_end) break;                 // the chunk's samples are n0 - 15 .. n0 + CHUNK - 1
    if (n0 + CHUNK <= n_first) continue;
    __syncthreads();
    for (int i = t; i < CHUNK + APAD; i += 256) { const long long n = n0 - APAD + i; sa[i] = (n >= 0 && n < la) ? arow[n] : 0.f; }
    for (int i = t; i < CHUNK + LAG_TILE; i += 256) { const long long m = n0 + l0 + i; sb[i] = (m >= 0 && m < lb) ? brow[m] : 0.f; }
    __syncthreads();
    const float* pa = sa + APAD + hi - lo;                       // + s: index in [1, CHUNK + APAD - 1]
    const float* pb = sb + hi + 16 * lo + 512 * wv;              // + s (+ 256): index at most CHUNK - 4 + 3 + 240 + 1536 + 256 = CHUNK + 2031
#pragma unroll 4
    for (int s = 0; s < CHUNK; s += 4) {
      const double av = (double)pa[s], b0 = (double)pb[s], b1 = (double)pb[s + 256];
      acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, b0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, b1, acc1, 0, 0, 0);
    }
  }
  double* out = part + ((size_t)b * slices + j) * (size_t)W;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long long base = (long long)tile * LAG_TILE + 512 * wv + 16 * lo + hi + 4 * r;     // C/D: col = lane & 15, row = (lane >> 4) + 4 r
    if (base < W) out[base] = acc0[r];
    if (base + 256 < W) out[base + 256] = acc1[r];
  }
}

int main() {
  const int B = 8, La = 192000, Lb = 191000;
  std::vector<float> ha((size_t)B * La), hb((size_t)B * Lb);
  std::vector<int> la(B), lb(B);
  srand(1);
  for (auto& v : ha) v = (float)(rand() % 129 - 64);
  for (auto& v : hb) v = (float)(rand() % 129 - 64);
  for (int b = 0; b < B; ++b) { la[b] = La - 4099 * b; lb[b] = Lb - 1001 * (B - 1 - b); }
  la[3] = 3 * SLICE;           // a clip that ends exactly on a slice boundary
  float *da, *db;
  int *dla, *dlb;
  CK(hipMalloc(&da, ha.size() * 4)); CK(hipMalloc(&db, hb.size() * 4)); CK(hipMalloc(&dla, B * 4)); CK(hipMalloc(&dlb, B * 4));
  CK(hipMemcpy(da, ha.data(), ha.size() * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(db, hb.data(), hb.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(dla, la.data(), B * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(dlb, lb.data(), B * 4, hipMemcpyHostToDevice));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  const int Ms[2] = {4800, 48000};
  for (int mi = 0; mi < 2; ++mi) {
    const int M = Ms[mi];
    const size_t W = 2 * (size_t)M + 1;
    const int tiles = (int)((W + LAG_TILE - 1) / LAG_TILE);
    const int slices[2] = {(La + SLICE - 1) / SLICE, (La + 15 + SLICE - 1) / SLICE};
    std::vector<std::vector<double>> c(2, std::vector<double>((size_t)B * W, 0.0));
    for (int v = 0; v < 2; ++v) {
      const size_t n = (size_t)B * slices[v] * W;
      double* dp;
      CK(hipMalloc(&dp, n * 8));
      CK(hipMemset(dp, 0xff, n * 8));                          // NaN: a slice that was not written shows
      float ms = 0.f, best = 1e30f;
      for (int rep = 0; rep < 4; ++rep) {
        CK(hipEventRecord(e0, 0));
        if (v == 0) hipLaunchKernelGGL(fma_kernel, dim3(slices[v], tiles, B), dim3(256), 0, 0, da, db, dla, dlb, La, Lb, M, slices[v], dp);
        else hipLaunchKernelGGL(mfma_kernel, dim3(slices[v], tiles, B), dim3(256), 0, 0, da, db, dla, dlb, La, Lb, M, slices[v], dp);
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        CK(hipGetLastError());
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (rep > 0 && ms < best) best = ms;
      }
      std::vector<double> hp(n);
      CK(hipMemcpy(hp.data(), dp, n * 8, hipMemcpyDeviceToHost));
      CK(hipFree(dp));
      for (int b = 0; b < B; ++b) {
        const int ns = v == 0 ? (la[b] + SLICE - 1) / SLICE : (la[b] + 15 + SLICE - 1) / SLICE;
        for (int s = 0; s < ns; ++s)
          for (size_t l = 0; l < W; ++l) c[v][b * W + l] += hp[((size_t)b * slices[v] + s) * W + l];
      }
      double fmas = 0;
      for (int b = 0; b < B; ++b) fmas += (double)W * (la[b] < lb[b] ? la[b] : lb[b]);
      printf("M %d %s: best of 3 %.3f ms, %.2f T fma/s\n", M, v == 0 ? "fma " : "mfma", best, fmas / best / 1e9);
    }
    size_t differ = 0, nan = 0;
    for (size_t i = 0; i < c[0].size(); ++i) { differ += c[0][i] != c[1][i]; nan += c[0][i] != c[0][i] || c[1][i] != c[1][i]; }
    // spot check against a plain loop on the host
    size_t wrong = 0;
    for (int b = 0; b < B; b += 3)
      for (long long l = -M; l <= M; l += (2 * M) / 40) {
        double s = 0;
        for (long long n = 0; n < la[b]; ++n) { const long long m = n + l; if (m >= 0 && m < lb[b]) s += (double)ha[(size_t)b * La + n] * (double)hb[(size_t)b * Lb + m]; }
        wrong += s != c[1][b * W + (l + M)];
        wrong += s != c[0][b * W + (l + M)];
      }
    printf("M %d: %zu of %zu values differ between the kernels, %zu NaN, %zu spot checks wrong\n", M, differ, c[0].size(), nan, wrong);
  }
  return 0;
}
