// estimate.hip -- the statistics behind FlowDec's two data-dependent parameters (include/flowdec_hip.h "Parameter estimation"):
// beta = 1 / q(|X_c|) of the compressed clean spectra and sigma_y = q(RMSE(Y_c, X_c)) / 3 of coded against clean, global or per band
// (scripts/estimate_flowdec_params.py of the reference; flowdec_amd/estimate.py drives the two calls below).
//
// fd_estimate_pair_stats, per pair (x clean, y coded) of one row length L:
//   normfac = max|y| + 1e-5 in float32 (normalize_noisy of the script: no zero guard), x / normfac and y / normfac sample by sample,
//   framing + the exact-f32 DFT GEMM of stft.hip on both (fd_stft_raw_spectrum), then ONE epilogue that reads both raw spectra once:
//   amplitude compression |.|^alpha e^{j angle} of both (compress_kernel's arithmetic, beta = 1), |X_c| -> absx_out, and
//   sum_t |Y_c - X_c|^2 per band: the difference per component in float32 (complex64 subtraction), squared and summed in float64.
//   A workgroup owns BAND_F bands of one pair; thread (f, lane) sums frames lane, lane + BAND_TL, ... and a band's BAND_TL partials are
//   added in index order: the order depends on T only, there are no atomics, and a pair's bits do not depend on the batch.
//
// fd_select_f32: exact order statistics of n non-negative float32 values by a most-significant-digit radix select on the bit pattern
// (monotone for non-negative floats, denormals and +inf included): four passes of 8 bits.  Each pass builds per-workgroup LDS histograms
// with integer atomics, flushes them to 64-bit global counters with integer atomics (integer adds commute: the counts do not depend on
// the order of the workgroups), and a one-workgroup kernel picks every rank's bucket and residual rank on the device -- no host
// synchronisation between the passes.  Ranks that still share their prefix share one histogram (`leader`).
#include <limits.h>

#include "internal.h"
#include "measure_common.h"

namespace {

// ---- pair statistics ------------------------------------------------------------------------------------------------------------------
constexpr int BAND_F = 16;       // bands per epilogue workgroup
constexpr int BAND_TL = 16;      // frame lanes per band: thread (f, lane) takes frames lane, lane + 16, ...
constexpr int BAND_TT = 64;      // frames per LDS tile of the |X_c| transpose

// normfac[b] = max|y[b]| + 1e-5 (float32); xs = x / normfac, ys = y / normfac.  One workgroup per pair.
__global__ __launch_bounds__(1024) void normalize_pair_kernel(const float* __restrict__ x, const float* __restrict__ y, int L, float* __restrict__ normfac,
                                                              float* __restrict__ xs, float* __restrict__ ys) {
  const int b = blockIdx.x;
  const size_t row = (size_t)b * L;
  float m = 0.f;
  for (int i = threadIdx.x; i < L; i += 1024) m = fmaxf(m, fabsf(y[row + i]));
  m = fd_wave_max(m);
  __shared__ float red[16];
  __shared__ float nf_s;
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    float r = 0.f;
    for (int i = 0; i < 16; ++i) r = fmaxf(r, red[i]);
    nf_s = r + 1e-5f;
    normfac[b] = nf_s;
  }
  __syncthreads();
  const float nf = nf_s;
  for (int i = threadIdx.x; i < L; i += 1024) {
    xs[row + i] = x[row + i] / nf;
    ys[row + i] = y[row + i] / nf;
  }
}

// compress_kernel's arithmetic (stft.hip) with beta = 1
__device__ __forceinline__ float2 compress1(float2 v, float alpha) {
  float re = v.x, im = v.y;
  if (alpha != 1.0f) {
    const float mag = powf(hypotf(re, im), alpha);
    const float th = atan2f(im, re);
    float sn, cs;
    sincosf(th, &sn, &cs);
    re = mag * cs; im = mag * sn;
  }
  return float2{re * 1.0f, im * 1.0f};
}

// spec_x / spec_y [b*T + t][2f, 2f+1] -> absx[b][f][t] = |X_c| (sqrt of re^2 + im^2 in float64, rounded to float32; absx may be null) and
// band_sq[b][f] = sum_t |Y_c - X_c|^2.  grid (ceil(F / BAND_F), B), 256 threads = BAND_F bands x BAND_TL frame lanes
__global__ __launch_bounds__(256) void pair_epilogue_kernel(const float* __restrict__ spec_x, const float* __restrict__ spec_y, int F, int T, int kpad,
                                                            float alpha, float* __restrict__ absx, double* __restrict__ band_sq) {
  __shared__ float tile[BAND_F][BAND_TT + 1];
  __shared__ double part[BAND_F][BAND_TL + 1];
  const int b = blockIdx.y, f0 = blockIdx.x * BAND_F;
  const int fl = threadIdx.x % BAND_F, tl = threadIdx.x / BAND_F;
  const int f = f0 + fl;
  double acc = 0.0;
  for (int t0 = 0; t0 < T; t0 += BAND_TT) {
#pragma unroll
    for (int q = 0; q < BAND_TT / BAND_TL; ++q) {
      const int tt = q * BAND_TL + tl, t = t0 + tt;
      float a = 0.f;
      if (f < F && t < T) {
        const size_t o = ((size_t)b * T + t) * kpad + 2 * f;
        const float2 xc = compress1(*reinterpret_cast<const float2*>(spec_x + o), alpha);
        const float2 yc = compress1(*reinterpret_cast<const float2*>(spec_y + o), alpha);
        a = (float)__dsqrt_rn((double)xc.x * (double)xc.x + (double)xc.y * (double)xc.y);
        const float dr = yc.x - xc.x, di = yc.y - xc.y;
        acc += (double)dr * (double)dr + (double)di * (double)di;
      }
      tile[fl][tt] = a;
    }
    if (absx) {
      __syncthreads();
      const int tt = threadIdx.x % BAND_TT;
      for (int r = threadIdx.x / BAND_TT; r < BAND_F; r += 256 / BAND_TT)
        if (f0 + r < F && t0 + tt < T) absx[((size_t)b * F + f0 + r) * T + t0 + tt] = tile[r][tt];
      __syncthreads();
    }
  }
  part[fl][tl] = acc;
  __syncthreads();
  if (threadIdx.x < BAND_F && f0 + threadIdx.x < F) {
    double v = 0.0;
    for (int j = 0; j < BAND_TL; ++j) v += part[threadIdx.x][j];
    band_sq[(size_t)b * F + f0 + threadIdx.x] = v;
  }
}

struct pair_layout { size_t clip, plane, total; int T; };

pair_layout pair_bytes(int B, int L, int n_fft, int hop) {
  pair_layout s;
  s.T = 1 + L / hop;
  s.clip = fd_align(sizeof(float) * (size_t)B * L);
  s.plane = fd_align(sizeof(float) * (size_t)B * s.T * fd_stft_kpad(n_fft));
  s.total = 2 * s.clip + 3 * s.plane;      // x / normfac, y / normfac; frames, spec_x, spec_y
  return s;
}

// ---- radix select ---------------------------------------------------------------------------------------------------------------------
constexpr int SEL_MAX_R = 8, SEL_PASSES = 4, SEL_BINS = 256;
constexpr int SEL_GRID_CAP = 2048;

struct select_ranks { long long r[SEL_MAX_R]; };

// what the pick kernel hands from pass to pass (global memory, in the workspace)
struct select_state {
  unsigned long long residual[SEL_MAX_R];   // rank among the values that share `prefix` in the bits already fixed
  unsigned int prefix[SEL_MAX_R];
  int leader[SEL_MAX_R];                    // the lowest rank index with the same prefix: its histogram serves this rank too
};

// the key of a value: its bit pattern, -0.0 as +0.0.  A set sign bit or a NaN is `bad` (and still counted in a bucket: the totals stay n)
__device__ __forceinline__ unsigned int select_key(unsigned int bits, unsigned int& bad) {
  if (bits == 0x80000000u) return 0u;
  bad += (bits > 0x7f800000u) ? 1u : 0u;
  return bits;
}

__global__ __launch_bounds__(256) void select_init_kernel(select_ranks ranks, int R, unsigned long long* __restrict__ hist, select_state* __restrict__ state,
                                                          long long* __restrict__ bad_out) {
  for (int i = threadIdx.x; i < SEL_PASSES * R * SEL_BINS; i += 256) hist[i] = 0ull;
  if (threadIdx.x < SEL_MAX_R) {
    state->residual[threadIdx.x] = threadIdx.x < R ? (unsigned long long)ranks.r[threadIdx.x] : 0ull;
    state->prefix[threadIdx.x] = 0u;
    state->leader[threadIdx.x] = 0;
  }
  if (threadIdx.x == 0) *bad_out = 0;
}

// pass p looks at bits [24 - 8 p, 32 - 8 p) of the values whose higher bits equal a rank's prefix
template <bool FIRST>
__device__ __forceinline__ void select_count(unsigned int bits, int shift, int R, const unsigned int* __restrict__ prefix, const int* __restrict__ leader,
                                             unsigned int* __restrict__ lh, unsigned int& bad) {
  unsigned int dummy = 0;
  const unsigned int key = select_key(bits, FIRST ? bad : dummy);
  const unsigned int digit = (key >> shift) & 0xffu;
  if (FIRST) {
    atomicAdd(&lh[digit], 1u);               // every rank has the empty prefix: one histogram (leader 0)
  } else {
    const unsigned int high = key >> (shift + 8);
    for (int r = 0; r < R; ++r)
      if (leader[r] == r && (prefix[r] >> (shift + 8)) == high) atomicAdd(&lh[r * SEL_BINS + digit], 1u);
  }
}

template <bool FIRST>
__global__ __launch_bounds__(256) void select_hist_kernel(const float* __restrict__ values, long long n, int pass, int R,
                                                          const select_state* __restrict__ state, unsigned long long* __restrict__ hist,
                                                          long long* __restrict__ bad_out) {
  __shared__ unsigned int lh[SEL_MAX_R * SEL_BINS];
  __shared__ unsigned int prefix[SEL_MAX_R];
  __shared__ int leader[SEL_MAX_R];
  const int rows = FIRST ? 1 : R;
  for (int i = threadIdx.x; i < rows * SEL_BINS; i += 256) lh[i] = 0u;
  if (threadIdx.x < SEL_MAX_R) { prefix[threadIdx.x] = state->prefix[threadIdx.x]; leader[threadIdx.x] = state->leader[threadIdx.x]; }
  __syncthreads();
  const int shift = 24 - 8 * pass;
  const unsigned int* __restrict__ v = reinterpret_cast<const unsigned int*>(values);
  unsigned int bad = 0;
  // scalar head up to the first 16-byte boundary, uint4 body, scalar tail
  long long head = (long long)(((16 - ((uintptr_t)v & 15)) & 15) / 4);
  if (head > n) head = n;
  const long long nvec = (n - head) / 4, tail0 = head + 4 * nvec;
  const long long gtid = blockIdx.x * (long long)blockDim.x + threadIdx.x, gsz = (long long)gridDim.x * blockDim.x;
  if (gtid < head) select_count<FIRST>(v[gtid], shift, R, prefix, leader, lh, bad);
  if (gtid < n - tail0) select_count<FIRST>(v[tail0 + gtid], shift, R, prefix, leader, lh, bad);
  const uint4* __restrict__ v4 = reinterpret_cast<const uint4*>(v + head);
  for (long long i = gtid; i < nvec; i += gsz) {
    const uint4 q = v4[i];
    select_count<FIRST>(q.x, shift, R, prefix, leader, lh, bad);
    select_count<FIRST>(q.y, shift, R, prefix, leader, lh, bad);
    select_count<FIRST>(q.z, shift, R, prefix, leader, lh, bad);
    select_count<FIRST>(q.w, shift, R, prefix, leader, lh, bad);
  }
  __syncthreads();
  unsigned long long* __restrict__ gh = hist + (size_t)pass * R * SEL_BINS;
  for (int i = threadIdx.x; i < rows * SEL_BINS; i += 256)
    if (lh[i]) atomicAdd(&gh[i], (unsigned long long)lh[i]);
  if (FIRST && bad) atomicAdd(reinterpret_cast<unsigned long long*>(bad_out), (unsigned long long)bad);
}

// one workgroup: every rank's bucket of this pass and its rank inside it; after the last pass the prefix is the value's bit pattern
__global__ __launch_bounds__(256) void select_pick_kernel(int pass, int R, const unsigned long long* __restrict__ hist, select_state* __restrict__ state,
                                                          float* __restrict__ out) {
  __shared__ unsigned long long h[SEL_MAX_R * SEL_BINS];
  __shared__ unsigned int prefix[SEL_MAX_R];
  const unsigned long long* __restrict__ gh = hist + (size_t)pass * R * SEL_BINS;
  for (int i = threadIdx.x; i < R * SEL_BINS; i += 256) h[i] = gh[i];
  __syncthreads();
  const int shift = 24 - 8 * pass;
  if (threadIdx.x < R) {
    const int r = threadIdx.x;
    const unsigned long long* row = h + state->leader[r] * SEL_BINS;
    unsigned long long res = state->residual[r];
    int d = 0;
    for (; d < SEL_BINS - 1; ++d) {
      const unsigned long long c = row[d];
      if (res < c) break;
      res -= c;
    }
    const unsigned int p = state->prefix[r] | ((unsigned int)d << shift);
    prefix[r] = p;
    state->prefix[r] = p;
    state->residual[r] = res;
    if (pass == SEL_PASSES - 1) out[r] = __uint_as_float(p);
  }
  __syncthreads();
  if (threadIdx.x < R) {
    int lead = threadIdx.x;
    for (int q = threadIdx.x - 1; q >= 0; --q)
      if (prefix[q] == prefix[threadIdx.x]) lead = q;
    state->leader[threadIdx.x] = lead;
  }
}

inline size_t select_hist_bytes(int R) { return fd_align(sizeof(unsigned long long) * (size_t)SEL_PASSES * R * SEL_BINS); }

}  // namespace

extern "C" size_t fd_estimate_workspace_bytes(int B, int L, int n_fft, int hop) {
  if (B <= 0 || B > 65535 || L <= 0 || n_fft <= 0 || n_fft % 2 != 0 || hop <= 0) return 0;
  return pair_bytes(B, L, n_fft, hop).total + 256;    // (the entry point aligns the base itself)
}

extern "C" int fd_estimate_pair_stats(const fd_stft_plan* plan, const float* x, const float* y, int B, int L, float alpha, float* normfac_out,
                                      float* absx_out, double* band_sq_out, void* ws, size_t ws_bytes, void* stream) {
  FD_REQUIRE(plan && x && y && normfac_out && band_sq_out && ws, "fd_estimate_pair_stats: null pointer");
  FD_REQUIRE(B > 0 && B <= 65535 && L > 0 && L <= 0x7fffffff - 1024, "fd_estimate_pair_stats: bad batch B %d L %d (1 <= B <= 65535, L >= 1)", B, L);
  FD_REQUIRE(alpha > 0.f, "fd_estimate_pair_stats: alpha must be positive");
  int n_fft, hop, F, K;
  fd_stft_plan_dims(plan, &n_fft, &hop, &F, &K);
  FD_REQUIRE(L > n_fft / 2, "fd_estimate_pair_stats: a clip of %d samples cannot be reflect-padded by %d (n_fft %d needs at least %d samples)", L,
             n_fft / 2, n_fft, n_fft / 2 + 1);
  FD_REQUIRE((long long)B * (1 + L / hop) <= 65535LL * 128, "fd_estimate_pair_stats: %d pairs of %d samples are too many frames for one call "
             "(the DFT GEMM takes 65535 * 128 rows)", B, L);
  const size_t need = fd_estimate_workspace_bytes(B, L, n_fft, hop);
  FD_REQUIRE(ws_bytes >= need, "fd_estimate_pair_stats: workspace too small (%zu < %zu bytes, fd_estimate_workspace_bytes)", ws_bytes, need);
  const pair_layout s = pair_bytes(B, L, n_fft, hop);
  hipStream_t st = fd_stream(stream);
  char* base = aligned(ws);
  float* xs = reinterpret_cast<float*>(base);
  float* ys = reinterpret_cast<float*>(base + s.clip);
  float* frames = reinterpret_cast<float*>(base + 2 * s.clip);
  float* spec_x = reinterpret_cast<float*>(base + 2 * s.clip + s.plane);
  float* spec_y = reinterpret_cast<float*>(base + 2 * s.clip + 2 * s.plane);
  fd_stft_plan* p = const_cast<fd_stft_plan*>(plan);
  hipLaunchKernelGGL(normalize_pair_kernel, dim3(B), dim3(1024), 0, st, x, y, L, normfac_out, xs, ys);
  FD_TRY(fd_stft_raw_spectrum(p, xs, nullptr, B, L, frames, spec_x, st));
  FD_TRY(fd_stft_raw_spectrum(p, ys, nullptr, B, L, frames, spec_y, st));
  hipLaunchKernelGGL(pair_epilogue_kernel, dim3(fd_cdiv(F, BAND_F), B), dim3(256), 0, st, spec_x, spec_y, F, s.T, K, alpha, absx_out, band_sq_out);
  FD_LAUNCH_CHECK();
  return FD_OK;
}

extern "C" size_t fd_select_workspace_bytes(int R) {
  if (R < 1 || R > SEL_MAX_R) return 0;
  return select_hist_bytes(R) + fd_align(sizeof(select_state)) + 256;
}

extern "C" int fd_select_f32(const float* values, long long n, const long long* ranks, int R, float* out, long long* bad_out, void* ws, size_t ws_bytes,
                             void* stream) {
  FD_REQUIRE(values && ranks && out && bad_out && ws, "fd_select_f32: null pointer");
  FD_REQUIRE(R >= 1 && R <= SEL_MAX_R, "fd_select_f32: %d ranks (1 <= R <= %d)", R, SEL_MAX_R);
  FD_REQUIRE(n >= 1 && n <= (1LL << 40), "fd_select_f32: n = %lld values (1 <= n <= 2^40)", n);
  FD_REQUIRE((uintptr_t)values % 4 == 0, "fd_select_f32: values must be 4-byte aligned");
  select_ranks rk = {};
  for (int r = 0; r < R; ++r) {
    FD_REQUIRE(ranks[r] >= 0 && ranks[r] < n, "fd_select_f32: rank %d = %lld is outside [0, %lld)", r, ranks[r], n);
    rk.r[r] = ranks[r];
  }
  const size_t need = fd_select_workspace_bytes(R);
  FD_REQUIRE(ws_bytes >= need, "fd_select_f32: workspace too small (%zu < %zu bytes, fd_select_workspace_bytes)", ws_bytes, need);
  hipStream_t st = fd_stream(stream);
  char* base = aligned(ws);
  unsigned long long* hist = reinterpret_cast<unsigned long long*>(base);
  select_state* state = reinterpret_cast<select_state*>(base + select_hist_bytes(R));
  // the grid is capped: a workgroup's 32-bit LDS counters hold its share of n (n / grid < 2^32 for every n this call takes)
  long long g = (n / 4 + 255) / 256;
  const int grid = (int)(g > SEL_GRID_CAP ? SEL_GRID_CAP : (g < 1 ? 1 : g));
  hipLaunchKernelGGL(select_init_kernel, dim3(1), dim3(256), 0, st, rk, R, hist, state, bad_out);
  for (int pass = 0; pass < SEL_PASSES; ++pass) {
    if (pass == 0) hipLaunchKernelGGL(select_hist_kernel<true>, dim3(grid), dim3(256), 0, st, values, n, pass, R, state, hist, bad_out);
    else hipLaunchKernelGGL(select_hist_kernel<false>, dim3(grid), dim3(256), 0, st, values, n, pass, R, state, hist, bad_out);
    hipLaunchKernelGGL(select_pick_kernel, dim3(1), dim3(256), 0, st, pass, R, hist, state, out);
  }
  FD_LAUNCH_CHECK();
  return FD_OK;
}
