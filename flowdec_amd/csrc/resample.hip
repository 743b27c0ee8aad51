// resample.hip -- torchaudio's polyphase sinc resampler (include/flowdec_hip.h "Resampling") with an order of summation that is part of
// the contract: with o = orig / gcd, n = new / gcd, K = 2 width + o and the caller's float32 bank h[n][K], output m = q n + i is
//   acc = 0.0 (double);  for k = 0 .. K-1 ascending: j = q o + k - width;  if 0 <= j < L: acc += (double)h[i][k] * (double)x[j];  y[m] = (float)acc
// The product of two float32 values is exact in float64, so the float64 add in ascending k is the only rounding of the loop and a
// fused and an unfused multiply-add give the same bits.  One thread owns an output's whole sum: no matrix instruction, no atomics, no
// split K -- a sample's bits do not depend on the launch geometry, the batch or the cut of a stream into spans.
//
// One kernel serves the ragged batch and the streaming span.  A thread takes ONE phase i and RQ consecutive periods q (outputs q n + i):
// consecutive threads read consecutive phases of the bank, stored [K][n] (coalesced, through L2; each tap feeds RQ sums), and the
// periods of a workgroup read one window of the input, staged once in LDS with the zero padding and every bound already applied (a tap
// outside [0, L) multiplies a zero: acc starts at +0.0, so the bits are those of skipping it).  A rate pair whose window does not fit
// the LDS budget (n small beside o) runs the same loop on global memory with the bounds checked per tap.
//
// -DFD_RESAMPLE_ACC=float builds the float32-accumulating variant of the same kernel (timing only: scripts/resample_timing.py).
#include <limits.h>

#include <vector>

#include "common.h"
#include "internal.h"

#ifndef FD_RESAMPLE_ACC
#define FD_RESAMPLE_ACC double
#endif

struct fd_resample_plan {
  int o, n, width, K;
  float* bank;        // device, [K][n]
};

namespace {

typedef FD_RESAMPLE_ACC acc_t;

constexpr int RS_THREADS = 256;
constexpr int RQ = 4;                              // periods per thread
constexpr long long RS_BANK_CAP = 1LL << 24;       // n * K
constexpr size_t RS_LDS_BYTES = 48 * 1024;         // window budget of the LDS path
constexpr long long RS_NO_END = LLONG_MAX;

// ceil(n * L / o) without forming n * L: (L / o) n + ceil((L % o) n / o); o, n <= 2^24
__host__ __device__ inline long long out_length(long long L, int o, int n) {
  return (L / o) * n + ((L % o) * n + o - 1) / o;
}

struct resample_args {
  const float* x;        // row b starts at x + b * x_stride and holds the samples [x0, x0 + nx) of its recording
  float* y;              // row b starts at y + b * y_stride and takes the outputs [m0, m0 + count)
  const float* bank;     // [K][n]
  const int* lengths;    // per-row length (clamped into [0, nx]) or null
  long long x_stride, y_stride, x0, nx, total, m0, count;   // total: the recording's length when `lengths` is null, RS_NO_END while unknown
  int o, n, width, K, win;                                   // win: floats of the LDS window (LDS path)
};

// grid (ceil(n * ceil(periods / RQ) / 256), rows).  Item w = blockIdx.x * 256 + thread: phase w % n, periods q_first + (w / n) RQ + r.
template <bool LDS>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const resample_args a) {
  extern __shared__ __attribute__((aligned(16))) float win[];
  const int b = blockIdx.y;
  const float* __restrict__ x = a.x + (long long)b * a.x_stride;
  float* __restrict__ y = a.y + (long long)b * a.y_stride;
  long long len = a.total, M = RS_NO_END;
  if (a.lengths) {
    const long long l = a.lengths[b];
    len = l < 0 ? 0 : (l > a.nx ? a.nx : l);
  }
  if (len != RS_NO_END) M = out_length(len, a.o, a.n);
  const long long m_end = a.m0 + a.count;
  const long long q_first = a.m0 / a.n;
  const long long w0 = (long long)blockIdx.x * RS_THREADS, w = w0 + threadIdx.x;
  const long long g_lo = w0 / a.n, g = w / a.n;
  const int i = (int)(w % a.n);
  const long long q_lo = q_first + g_lo * RQ;          // the workgroup's first period
  const long long q0 = q_first + g * RQ;               // this thread's first period
  // the samples a tap may read: inside the recording AND inside what x holds (the host has checked that the first implies the second)
  const long long lo = a.x0 > 0 ? a.x0 : 0;
  const long long hi = (a.x0 + a.nx < len) ? a.x0 + a.nx : len;

  if (LDS) {
    const long long j0 = q_lo * a.o - a.width;
    // a workgroup whose outputs all lie behind the row's end only writes zeros: skip the staging
    if (q_lo * a.n < M) {
      for (int t = threadIdx.x; t < a.win; t += RS_THREADS) {
        const long long j = j0 + t;
        win[t] = (j >= lo && j < hi) ? x[j - a.x0] : 0.f;
      }
    }
    __syncthreads();
  }

  acc_t acc[RQ];
#pragma unroll
  for (int r = 0; r < RQ; ++r) acc[r] = (acc_t)0;
  // nothing to sum for a thread whose outputs are all outside [m0, min(m_end, M))
  const long long m_first = q0 * a.n + i, m_last = (q0 + RQ - 1) * a.n + i;
  const bool live = m_last >= a.m0 && m_first < m_end && m_first < M;
  if (live) {
    const float* __restrict__ h = a.bank + i;
    if (LDS) {
      const float* __restrict__ xw = win + (int)(q0 - q_lo) * a.o;
      for (int k = 0; k < a.K; ++k) {
        const acc_t hk = (acc_t)h[(size_t)k * a.n];
#pragma unroll
        for (int r = 0; r < RQ; ++r) acc[r] += hk * (acc_t)xw[r * a.o + k];
      }
    } else {
      const long long j0 = q0 * a.o - a.width;
      for (int k = 0; k < a.K; ++k) {
        const acc_t hk = (acc_t)h[(size_t)k * a.n];
#pragma unroll
        for (int r = 0; r < RQ; ++r) {
          const long long j = j0 + (long long)r * a.o + k;
          const float xv = (j >= lo && j < hi) ? x[j - a.x0] : 0.f;
          acc[r] += hk * (acc_t)xv;
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < RQ; ++r) {
    const long long m = (q0 + r) * a.n + i;
    if (m >= a.m0 && m < m_end) y[m - a.m0] = m < M ? (float)acc[r] : 0.f;
  }
}

// floats of the largest window a workgroup stages: its 256 items span at most 255 / n + 2 groups of RQ periods
inline long long window_floats(int o, int n, int K) { return ((long long)(255 / n + 2) * RQ - 1) * o + K; }

int launch(const fd_resample_plan* p, resample_args a, int rows, hipStream_t st) {
  if (a.count <= 0 || rows <= 0) return FD_OK;
  a.bank = p->bank; a.o = p->o; a.n = p->n; a.width = p->width; a.K = p->K;
  // every sample index the kernel forms, (q + RQ) o + K, stays far inside 64 bits
  FD_REQUIRE((a.m0 + a.count) / a.n + 2 * RS_THREADS * RQ <= (1LL << 61) / a.o, "fd_resample: output %lld of a %d -> %d resampler is beyond 64-bit sample indices",
             a.m0 + a.count, a.o, a.n);
  const long long periods = (a.m0 + a.count - 1) / a.n - a.m0 / a.n + 1;
  const long long items = ((periods + RQ - 1) / RQ) * a.n;
  const long long blocks = (items + RS_THREADS - 1) / RS_THREADS;
  FD_REQUIRE(blocks <= 0x7fffffffLL, "fd_resample: %lld outputs are too many for one call", a.count);
  const long long win = window_floats(a.o, a.n, a.K);
  if ((size_t)win * sizeof(float) <= RS_LDS_BYTES) {
    a.win = (int)win;
    hipLaunchKernelGGL(resample_kernel<true>, dim3((unsigned)blocks, rows), dim3(RS_THREADS), (size_t)win * sizeof(float), st, a);
  } else {
    a.win = 0;
    hipLaunchKernelGGL(resample_kernel<false>, dim3((unsigned)blocks, rows), dim3(RS_THREADS), 0, st, a);
  }
  FD_LAUNCH_CHECK();
  return FD_OK;
}

}  // namespace

extern "C" long long fd_resample_out_length(long long L, int o, int n) {
  if (L < 0 || o < 1 || n < 1) return -1;
  return out_length(L, o, n);
}

extern "C" int fd_resample_plan_create(const float* bank_host, int o, int n, int width, fd_resample_plan** out) {
  FD_REQUIRE(out, "fd_resample_plan_create: null out");
  *out = nullptr;
  FD_REQUIRE(bank_host, "fd_resample_plan_create: null bank");
  FD_REQUIRE(o >= 1 && n >= 1 && width >= 0, "fd_resample_plan_create: bad rates o %d n %d width %d (o, n >= 1, width >= 0)", o, n, width);
  const long long K = 2LL * width + o;
  FD_REQUIRE((long long)n * K <= RS_BANK_CAP, "fd_resample_plan_create: a bank of %d phases x %lld taps is over the cap of 2^24 coefficients", n, K);
  std::vector<float> t((size_t)n * K);              // [n][K] -> [K][n]
  for (int i = 0; i < n; ++i)
    for (long long k = 0; k < K; ++k) t[(size_t)k * n + i] = bank_host[(size_t)i * K + k];
  fd_resample_plan* p = new fd_resample_plan();
  p->o = o; p->n = n; p->width = width; p->K = (int)K; p->bank = nullptr;
  hipError_t e = hipMalloc(&p->bank, sizeof(float) * t.size());
  if (e == hipSuccess) e = hipMemcpy(p->bank, t.data(), sizeof(float) * t.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    if (p->bank) (void)hipFree(p->bank);
    delete p;
    return fd_set_error(FD_ERUNTIME, "fd_resample_plan_create: uploading the bank failed: %s", hipGetErrorString(e));
  }
  *out = p;
  return FD_OK;
}

void fd_resample_plan_dims(const fd_resample_plan* p, int* o, int* n, int* width, int* K) {
  if (o) *o = p->o;
  if (n) *n = p->n;
  if (width) *width = p->width;
  if (K) *K = p->K;
}

extern "C" void fd_resample_plan_destroy(fd_resample_plan* p) {
  if (!p) return;
  (void)hipFree(p->bank);
  delete p;
}

extern "C" int fd_resample(const fd_resample_plan* plan, const float* x, const int* lengths, int B, int L, float* y, long long L_out, void* stream) {
  FD_REQUIRE(plan && x && y, "fd_resample: null pointer");
  FD_REQUIRE(B >= 1 && B <= 65535 && L >= 1, "fd_resample: bad batch B %d L %d (1 <= B <= 65535, L >= 1)", B, L);
  const long long M = out_length(L, plan->o, plan->n);
  FD_REQUIRE(L_out >= M && L_out <= (1LL << 40), "fd_resample: L_out %lld is smaller than the %lld outputs of a row of %d samples (or beyond 2^40)", L_out,
             M, L);
  resample_args a = {};
  a.x = x; a.y = y; a.lengths = lengths;
  a.x_stride = L; a.y_stride = L_out; a.x0 = 0; a.nx = L; a.total = L; a.m0 = 0; a.count = L_out;
  return launch(plan, a, B, fd_stream(stream));
}

extern "C" int fd_resample_span(const fd_resample_plan* plan, const float* x, long long x0, long long nx, long long total, long long m0, long long count,
                                float* y, void* stream) {
  FD_REQUIRE(plan, "fd_resample_span: null plan");
  FD_REQUIRE(x0 >= 0 && nx >= 0 && total >= -1 && m0 >= 0 && count >= 0, "fd_resample_span: negative index (x0 %lld nx %lld total %lld m0 %lld count %lld)",
             x0, nx, total, m0, count);
  FD_REQUIRE(x0 <= (1LL << 46) && nx <= (1LL << 46) && total <= (1LL << 46) && m0 <= (1LL << 46) && count <= (1LL << 46),
             "fd_resample_span: an index is beyond 2^46");
  if (count == 0) return FD_OK;
  FD_REQUIRE(y && (x || nx == 0), "fd_resample_span: null pointer");
  const int o = plan->o, n = plan->n;
  if (total >= 0) {
    const long long M = out_length(total, o, n);
    FD_REQUIRE(m0 + count <= M, "fd_resample_span: outputs [%lld, %lld) reach past the %lld outputs of %lld samples", m0, m0 + count, M, total);
  }
  // the samples the span reads: [q(m0) o - width, q(m0 + count - 1) o + K - 1 - width], cut to the recording
  long long first = (m0 / n) * o - plan->width, last = ((m0 + count - 1) / n) * o + plan->K - 1 - plan->width;
  if (first < 0) first = 0;
  if (total >= 0 && last > total - 1) last = total - 1;
  FD_REQUIRE(first > last || (first >= x0 && last < x0 + nx), "fd_resample_span: outputs [%lld, %lld) read the samples [%lld, %lld], x holds [%lld, %lld)",
             m0, m0 + count, first, last, x0, x0 + nx);
  resample_args a = {};
  a.x = x; a.y = y; a.lengths = nullptr;
  a.x_stride = 0; a.y_stride = 0; a.x0 = x0; a.nx = nx; a.total = total >= 0 ? total : RS_NO_END; a.m0 = m0; a.count = count;
  return launch(plan, a, 1, fd_stream(stream));
}
