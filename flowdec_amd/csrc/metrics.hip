// metrics.hip -- evaluation metrics of a triples list on the GPU (include/flowdec_hip.h "Evaluation metrics").
//
// SI-SDR / SI-SIR / SI-SAR (flowdec/eval/metrics.py:256-270, components :554-563) and the log-spectral MSE (:333-372) over ragged
// batches: rows [B][L] float32, clip b = the first lengths[b] samples of its row.  The invariant of the ragged entry points holds here
// too: a clip's result has the same BITS alone, in a batch, at any batch position and next to clips of any other lengths.  Every
// partition and every order of summation below is a function of the clip's own length only (never of B or L), every reduction runs in a
// fixed order, and there are no floating-point atomics.
//
// SI-SxR is the reference's algorithm in float64, in two passes over x_hat, x, y (the samples are float32, so every first-level product
// is exact in float64):
//   pass 1   x.y, x.x, x_hat.x and, for BOTH signs n = y -+ x (formed per sample in float64), x_hat.n and n.n
//   finalise the reference takes n = y + x when ||y + x|| < ||y - x||, which is x.y < 0: decided from the finished x.y; then
//            alpha_s = x_hat.x / x.x, alpha_n = x_hat.n / n.n
//   pass 2   per sample s_target = alpha_s x, e_noise = alpha_n n, e_art = x_hat - s_target - e_noise; sums of s_target^2, e_noise^2,
//            e_art^2, (e_noise + e_art)^2.  The residual norms are NOT expanded out of a Gram matrix (that cancels when e_art is small).
// Each clip is cut into PARTS contiguous slices [j n / P, (j + 1) n / P) of its own n samples; workgroup (j, b) sums its slice
// (thread, then wave, then the four waves in order) and writes one float64 partial per quantity; the finalise kernels add a clip's
// partials in index order.
//
// The log-spectral MSE reuses the DFT-as-GEMM front end of stft.hip (framing without normalisation, each clip's own reflect boundary,
// the exact-f32 MFMA GEMM whose rows do not depend on the batch: tests/test_hip_stft.py (b)), then an epilogue per (clip, tile of
// LOGSPEC_TILE_T frames): |X|^2 = re^2 + im^2 in float32 (the spectrum is float32), float64 from there: clamp, 10 log10, squared
// difference, fixed-order sums.  A clip's tiles are a function of its own frame count only.
#include <limits.h>
#include <math.h>

#include <algorithm>

#include "internal.h"
#include "measure_common.h"

namespace {

constexpr int PARTS = 128;          // slices per clip of the SI-SxR passes (a 30 s clip at 48 kHz: 11250 samples per workgroup)
constexpr int Q1 = 7, Q2 = 4;       // quantities of pass 1 / pass 2
constexpr int LOGSPEC_TILE_T = 8;   // frames per epilogue workgroup

// acc[q] of the 256 threads -> out[q] (fd_block_sums' fixed order)
template <int Q>
__device__ __forceinline__ void block_sums(double (&acc)[Q], double* __restrict__ out) {
  fd_block_sums<Q>(acc);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < Q; ++q) out[q] = acc[q];
  }
}

// part1[b][j][0..6] = x.y, x.x, x_hat.x, x_hat.(y - x), |y - x|^2, x_hat.(y + x), |y + x|^2 over slice j of clip b
__global__ __launch_bounds__(256) void sisxr_pass1_kernel(const float* __restrict__ xh, const float* __restrict__ x, const float* __restrict__ y,
                                                          const int* __restrict__ lens, int L, double* __restrict__ part1) {
  const int b = blockIdx.y, j = blockIdx.x;
  const long long n = fd_clip_len(lens, b, L);
  const long long lo = j * n / PARTS, hi = (j + 1) * n / PARTS;
  const size_t row = (size_t)b * L;
  double acc[Q1] = {0, 0, 0, 0, 0, 0, 0};
  for (long long i = lo + threadIdx.x; i < hi; i += 256) {
    const double dx = (double)x[row + i], dy = (double)y[row + i], dh = (double)xh[row + i];
    const double nm = dy - dx, np = dy + dx;
    acc[0] += dx * dy;
    acc[1] += dx * dx;
    acc[2] += dh * dx;
    acc[3] += dh * nm;
    acc[4] += nm * nm;
    acc[5] += dh * np;
    acc[6] += np * np;
  }
  block_sums<Q1>(acc, part1 + ((size_t)b * PARTS + j) * Q1);
}

// the clip's partials in index order; the sign of n from x.y; sums[b][0..3] = x.x, x_hat.x, x_hat.n, n.n; coef[b] = alpha_s, alpha_n, sign
__global__ __launch_bounds__(64) void sisxr_finalise1_kernel(const double* __restrict__ part1, double* __restrict__ sums, double* __restrict__ coef) {
  const int b = blockIdx.x;
  __shared__ double s[Q1];
  if (threadIdx.x < Q1) {
    double v = 0.0;
    for (int j = 0; j < PARTS; ++j) v += part1[((size_t)b * PARTS + j) * Q1 + threadIdx.x];
    s[threadIdx.x] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const bool flip = s[0] < 0.0;               // ||y + x|| < ||y - x||  <=>  x.y < 0
    const double hn = flip ? s[5] : s[3], nn = flip ? s[6] : s[4];
    sums[b * 8 + 0] = s[1];
    sums[b * 8 + 1] = s[2];
    sums[b * 8 + 2] = hn;
    sums[b * 8 + 3] = nn;
    coef[b * 4 + 0] = s[2] / s[1];
    coef[b * 4 + 1] = hn / nn;
    coef[b * 4 + 2] = flip ? 1.0 : -1.0;
  }
}

// part2[b][j][0..3] = |s_target|^2, |e_noise|^2, |e_art|^2, |e_noise + e_art|^2 over slice j of clip b
__global__ __launch_bounds__(256) void sisxr_pass2_kernel(const float* __restrict__ xh, const float* __restrict__ x, const float* __restrict__ y,
                                                          const int* __restrict__ lens, int L, const double* __restrict__ coef,
                                                          double* __restrict__ part2) {
  const int b = blockIdx.y, j = blockIdx.x;
  const long long n = fd_clip_len(lens, b, L);
  const long long lo = j * n / PARTS, hi = (j + 1) * n / PARTS;
  const size_t row = (size_t)b * L;
  const double as = coef[b * 4 + 0], an = coef[b * 4 + 1], sgn = coef[b * 4 + 2];
  double acc[Q2] = {0, 0, 0, 0};
  for (long long i = lo + threadIdx.x; i < hi; i += 256) {
    const double dx = (double)x[row + i], dy = (double)y[row + i], dh = (double)xh[row + i];
    const double nv = dy + sgn * dx;            // sgn = +-1: one rounding, as y - x / y + x
    const double st = as * dx, en = an * nv;
    const double ea = dh - st - en, r = en + ea;
    acc[0] += st * st;
    acc[1] += en * en;
    acc[2] += ea * ea;
    acc[3] += r * r;
  }
  block_sums<Q2>(acc, part2 + ((size_t)b * PARTS + j) * Q2);
}

__global__ __launch_bounds__(64) void sisxr_finalise2_kernel(const double* __restrict__ part2, double* __restrict__ sums) {
  const int b = blockIdx.x;
  if (threadIdx.x < Q2) {
    double v = 0.0;
    for (int j = 0; j < PARTS; ++j) v += part2[((size_t)b * PARTS + j) * Q2 + threadIdx.x];
    sums[b * 8 + 4 + threadIdx.x] = v;
  }
}

// ---- log-spectral MSE ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float power_of(float2 v) { return v.x * v.x + v.y * v.y; }

// a clip's own frame count, 0 for a length the transform cannot take (shorter than the reflect padding needs, or longer than the row)
__device__ __forceinline__ int logspec_frames(const int* __restrict__ lens, int b, int L, int n_fft, int hop) {
  const int l = lens[b];
  return (l <= n_fft / 2 || l > L) ? 0 : 1 + l / hop;
}

__device__ __forceinline__ double log_power_db(float p, double eps) {
  const double d = (double)p;
  return 10.0 * log10(d < eps ? eps : d);       // torch.clamp(min = eps): NaN stays NaN
}

// partial[b][j] = sum over frames [8 j, 8 j + 8) below the clip's own T_b and all F bins of (10 log10 Pa - 10 log10 Pb)^2
__global__ __launch_bounds__(256) void logspec_tile_kernel(const float* __restrict__ spec_a, const float* __restrict__ spec_b, const int* __restrict__ lens,
                                                           int L, int T, int n_fft, int hop, int F, int kpad, double eps, int tiles,
                                                           double* __restrict__ partial) {
  const int b = blockIdx.y, j = blockIdx.x;
  const int Tb = logspec_frames(lens, b, L, n_fft, hop);
  const int t0 = j * LOGSPEC_TILE_T;
  double acc[1] = {0.0};
  for (int idx = threadIdx.x; idx < LOGSPEC_TILE_T * F; idx += 256) {
    const int t = t0 + idx / F, f = idx % F;
    if (t < Tb) {
      const size_t o = ((size_t)b * T + t) * kpad + 2 * f;
      const double da = log_power_db(power_of(*reinterpret_cast<const float2*>(spec_a + o)), eps);
      const double db = log_power_db(power_of(*reinterpret_cast<const float2*>(spec_b + o)), eps);
      const double d = da - db;
      acc[0] += d * d;
    }
  }
  block_sums<1>(acc, partial + (size_t)b * tiles + j);
}

// mse[b] = (the clip's tile partials in index order) / (F T_b); NaN for a length the transform cannot take
__global__ __launch_bounds__(64) void logspec_finalise_kernel(const double* __restrict__ partial, const int* __restrict__ lens, int L, int n_fft, int hop,
                                                              int F, int tiles, double* __restrict__ mse) {
  const int b = blockIdx.x;
  if (threadIdx.x != 0) return;
  const int Tb = logspec_frames(lens, b, L, n_fft, hop);
  if (Tb == 0) { mse[b] = fd_nan(); return; }
  const int nt = (Tb + LOGSPEC_TILE_T - 1) / LOGSPEC_TILE_T;
  double v = 0.0;
  for (int j = 0; j < nt; ++j) v += partial[(size_t)b * tiles + j];
  mse[b] = v / ((double)F * (double)Tb);
}

// P[b][t][f] = re^2 + im^2 (the epilogue's float32 arithmetic), zero in the frames a shorter clip does not have
__global__ void power_spec_kernel(const float* __restrict__ spec, const int* __restrict__ lens, int B, int L, int T, int n_fft, int hop, int F, int kpad,
                                  float* __restrict__ P) {
  const long long total = (long long)B * T * F;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int f = (int)(i % F);
    const long long fr = i / F;
    const int t = (int)(fr % T), b = (int)(fr / T);
    float v = 0.f;
    if (t < logspec_frames(lens, b, L, n_fft, hop)) v = power_of(*reinterpret_cast<const float2*>(spec + (size_t)fr * kpad + 2 * f));
    P[i] = v;
  }
}

size_t sisxr_bytes(int B) {
  return fd_align(sizeof(double) * (size_t)B * PARTS * Q1) + fd_align(sizeof(double) * (size_t)B * PARTS * Q2) + fd_align(sizeof(double) * (size_t)B * 4);
}

struct spec_layout { size_t plane, partial, total; int T, tiles; };

spec_layout spec_bytes(int B, int L, int n_fft, int hop) {
  spec_layout s;
  s.T = 1 + L / hop;
  s.tiles = (s.T + LOGSPEC_TILE_T - 1) / LOGSPEC_TILE_T;
  s.plane = fd_align(sizeof(float) * (size_t)B * s.T * fd_stft_kpad(n_fft));
  s.partial = fd_align(sizeof(double) * (size_t)B * s.tiles);
  s.total = 3 * s.plane + s.partial;
  return s;
}

inline bool batch_ok(int B, int L) { return B > 0 && B <= 65535 && L > 0; }

// the checks shared by the two spectral entry points; -> FD_OK and the layout
int spec_check(const char* who, const fd_stft_plan* plan, int B, int L, size_t ws_bytes, spec_layout* out) {
  int n_fft, hop, F, K;
  fd_stft_plan_dims(plan, &n_fft, &hop, &F, &K);
  FD_REQUIRE(L > n_fft / 2, "%s: a clip of %d samples cannot be reflect-padded by %d (n_fft %d needs at least %d samples)", who, L, n_fft / 2, n_fft,
             n_fft / 2 + 1);
  FD_REQUIRE((long long)B * (1 + L / hop) <= 65535LL * 128, "%s: %d clips of %d samples are too many frames for one call (the DFT GEMM takes "
             "65535 * 128 rows)", who, B, L);
  const size_t need = fd_metrics_workspace_bytes(B, L, n_fft, hop);
  FD_REQUIRE(ws_bytes >= need, "%s: workspace too small (%zu < %zu bytes, fd_metrics_workspace_bytes)", who, ws_bytes, need);
  *out = spec_bytes(B, L, n_fft, hop);
  return FD_OK;
}

inline int grid_cap(long long n) { long long g = (n + 255) / 256; return (int)(g > 16384 ? 16384 : (g < 1 ? 1 : g)); }

}  // namespace

extern "C" size_t fd_metrics_workspace_bytes(int B, int L, int n_fft, int hop) {
  if (!batch_ok(B, L)) return 0;
  size_t need = sisxr_bytes(B);
  if (n_fft > 0 && n_fft % 2 == 0 && hop > 0) need = std::max(need, spec_bytes(B, L, n_fft, hop).total);
  return need + 256;    // (the entry points align the base themselves)
}

extern "C" int fd_metrics_sisxr(const float* x_hat, const float* x, const float* y, const int* lengths, int B, int L, double* sums_out, void* ws,
                                size_t ws_bytes, void* stream) {
  FD_REQUIRE(x_hat && x && y && lengths && sums_out && ws, "fd_metrics_sisxr: null pointer");
  FD_REQUIRE(batch_ok(B, L), "fd_metrics_sisxr: bad batch B %d L %d (1 <= B <= 65535, L >= 1)", B, L);
  const size_t need = sisxr_bytes(B) + 256;
  FD_REQUIRE(ws_bytes >= need, "fd_metrics_sisxr: workspace too small (%zu < %zu bytes, fd_metrics_workspace_bytes)", ws_bytes, need);
  hipStream_t st = fd_stream(stream);
  double* part1 = reinterpret_cast<double*>(aligned(ws));
  double* part2 = reinterpret_cast<double*>(reinterpret_cast<char*>(part1) + fd_align(sizeof(double) * (size_t)B * PARTS * Q1));
  double* coef = reinterpret_cast<double*>(reinterpret_cast<char*>(part2) + fd_align(sizeof(double) * (size_t)B * PARTS * Q2));
  hipLaunchKernelGGL(sisxr_pass1_kernel, dim3(PARTS, B), dim3(256), 0, st, x_hat, x, y, lengths, L, part1);
  hipLaunchKernelGGL(sisxr_finalise1_kernel, dim3(B), dim3(64), 0, st, part1, sums_out, coef);
  hipLaunchKernelGGL(sisxr_pass2_kernel, dim3(PARTS, B), dim3(256), 0, st, x_hat, x, y, lengths, L, coef, part2);
  hipLaunchKernelGGL(sisxr_finalise2_kernel, dim3(B), dim3(64), 0, st, part2, sums_out);
  FD_LAUNCH_CHECK();
  return FD_OK;
}

extern "C" int fd_metrics_logspec_mse(const fd_stft_plan* plan, const float* x_hat, const float* x, const int* lengths, int B, int L, double eps,
                                      double* mse_out, void* ws, size_t ws_bytes, void* stream) {
  FD_REQUIRE(plan && x_hat && x && lengths && mse_out && ws, "fd_metrics_logspec_mse: null pointer");
  FD_REQUIRE(batch_ok(B, L), "fd_metrics_logspec_mse: bad batch B %d L %d (1 <= B <= 65535, L >= 1)", B, L);
  FD_REQUIRE(eps > 0.0, "fd_metrics_logspec_mse: eps must be positive");
  spec_layout s;
  FD_TRY(spec_check("fd_metrics_logspec_mse", plan, B, L, ws_bytes, &s));
  int n_fft, hop, F, K;
  fd_stft_plan_dims(plan, &n_fft, &hop, &F, &K);
  hipStream_t st = fd_stream(stream);
  char* base = aligned(ws);
  float* frames = reinterpret_cast<float*>(base);
  float* spec_a = reinterpret_cast<float*>(base + s.plane);
  float* spec_b = reinterpret_cast<float*>(base + 2 * s.plane);
  double* partial = reinterpret_cast<double*>(base + 3 * s.plane);
  fd_stft_plan* p = const_cast<fd_stft_plan*>(plan);
  FD_TRY(fd_stft_raw_spectrum(p, x_hat, lengths, B, L, frames, spec_a, st));
  FD_TRY(fd_stft_raw_spectrum(p, x, lengths, B, L, frames, spec_b, st));
  hipLaunchKernelGGL(logspec_tile_kernel, dim3(s.tiles, B), dim3(256), 0, st, spec_a, spec_b, lengths, L, s.T, n_fft, hop, F, K, eps, s.tiles, partial);
  hipLaunchKernelGGL(logspec_finalise_kernel, dim3(B), dim3(64), 0, st, partial, lengths, L, n_fft, hop, F, s.tiles, mse_out);
  FD_LAUNCH_CHECK();
  return FD_OK;
}

extern "C" int fd_metrics_power_spec(const fd_stft_plan* plan, const float* x, const int* lengths, int B, int L, float* P_out, void* ws,
                                     size_t ws_bytes, void* stream) {
  FD_REQUIRE(plan && x && lengths && P_out && ws, "fd_metrics_power_spec: null pointer");
  FD_REQUIRE(batch_ok(B, L), "fd_metrics_power_spec: bad batch B %d L %d (1 <= B <= 65535, L >= 1)", B, L);
  spec_layout s;
  FD_TRY(spec_check("fd_metrics_power_spec", plan, B, L, ws_bytes, &s));
  int n_fft, hop, F, K;
  fd_stft_plan_dims(plan, &n_fft, &hop, &F, &K);
  hipStream_t st = fd_stream(stream);
  char* base = aligned(ws);
  float* frames = reinterpret_cast<float*>(base);
  float* spec = reinterpret_cast<float*>(base + s.plane);
  FD_TRY(fd_stft_raw_spectrum(const_cast<fd_stft_plan*>(plan), x, lengths, B, L, frames, spec, st));
  hipLaunchKernelGGL(power_spec_kernel, dim3(grid_cap((long long)B * s.T * F)), dim3(256), 0, st, spec, lengths, B, L, s.T, n_fft, hop, F, K, P_out);
  FD_LAUNCH_CHECK();
  return FD_OK;
}
