// measure_common.h -- what the measurement kernels share (metrics.hip, specdist.hip, segsnr.hip, stoi.hip, xcorr.hip; estimate.hip and
// loss.hip take the workspace base from here).  Every reduction here runs in one fixed order: the entry points' contract is a clip's
// result in the same BITS alone, in a batch and at any batch position.
#pragma once
#include "common.h"

// the 256-byte aligned base of a caller's workspace (the *_workspace_bytes functions count the 256 bytes this may skip)
inline char* aligned(void* ws) { return reinterpret_cast<char*>(((uintptr_t)ws + 255) / 256 * 256); }

const double PI = 3.14159265358979323846;

// a host table on the device; n == 0 gives a null pointer and success
template <typename T>
hipError_t upload(T** dst, const T* src, size_t n) {
  *dst = nullptr;
  if (n == 0) return hipSuccess;
  hipError_t e = hipMalloc(reinterpret_cast<void**>(dst), sizeof(T) * n);
  if (e == hipSuccess) e = hipMemcpy(*dst, src, sizeof(T) * n, hipMemcpyHostToDevice);
  return e;
}

// clip b's length clamped into its row of L samples: a wrong length gives a wrong number, never an out-of-bounds read
__device__ __forceinline__ int fd_clip_len(const int* __restrict__ lens, int b, int L) {
  const int l = lens[b];
  return l < 0 ? 0 : (l > L ? L : l);
}

// the quiet NaN the measurements give for a clip they cannot take
__device__ __forceinline__ double fd_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// acc[q] summed over the 256 threads of the workgroup, left in acc[] of EVERY thread: wave reduction, then the four waves in index order.
// Every thread calls it; a caller that calls it again puts a __syncthreads() in between (the last readers of red).
template <int Q>
__device__ __forceinline__ void fd_block_sums(double (&acc)[Q]) {
  __shared__ double red[4][Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const double v = fd_wave_sum(acc[q]);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][q] = v;
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < Q; ++q) acc[q] = ((red[0][q] + red[1][q]) + red[2][q]) + red[3][q];
}
