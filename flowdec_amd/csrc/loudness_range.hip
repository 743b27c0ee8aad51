// loudness_range.hip -- the two measures that make the loudness of loudness.hip a meter after EBU R 128: the true peak (ITU-R BS.1770-4
// Annex 2) of a ragged batch of mono signals at 48 kHz and the loudness range (EBU Tech 3342) of their sub-block energies
// (include/flowdec_hip.h "Loudness"; host yardsticks and the definitions: flowdec_amd/loudness.py true_peak_lin, range_of).
// eval_cli --true-peak / --loudness-range, loudness.loudness_report_batch and loudness.LoudnessMeter run on them.
//
// fd_true_peak.  With H the host's 4 x 2 W table (align.frac_bank(4, W): row j interpolates at n + j / 4, row 0 is the unit impulse):
//     p_b = max over n in [lo_b, hi_b), j in 0..3 of | sum_{t = 0 .. 2W-1} f64(x_b[n + t - W + 1]) * H[j][t] |
// t ascending, every product and every sum rounded to float64 on its own (no contraction: the pragma below), samples outside [0, len_b)
// zeros from the index alone, never loaded.  The device evaluates no transcendental.  A maximum has no order, so a clip's p has the same
// bits alone, in a batch and at any batch position.  A sum that is not finite (a NaN or Inf sample under some tap: row 0 reads every one
// of the 2 W samples of a position, and Inf * 0 is NaN) would be lost in a comparison: every thread carries a flag beside its maximum,
// and a flagged tile is stored as NaN.
//   tiles     workgroup (tile, b) owns TP_TILE positions: it stages the TP_TILE + 2 W - 1 samples they read once in LDS as float32 and the
//             8 W taps as float64; a thread runs the four chains of its positions t, t + 256, ... (consecutive lanes read consecutive LDS
//             words, a tap is a broadcast) and keeps a running maximum of |acc|; one maximum per tile goes to the workspace.  A tile
//             with no position of the window stores 0.0 and loads nothing.
//   finalise  one wave per clip: the maximum over its tiles, NaN if any tile is NaN or the clip is empty.
//
// fd_loudness_range.  One workgroup per clip, on the energies E of fd_loudness_energies:
//     st_j = (((E[j] + E[j+1]) + ...) + E[j+29]) / 144000,  j = 0 .. nsub - 30                       (kept in the workspace)
//     keep1 = st > ABS_GATE;  thr = 0.01 * (sum1 / n1);  keep2 = keep1 and st > thr;  m = n2
// sum1 in loudness.hip's order: 64 lane sums (lane l adds its windows l, l + 64, ... in ascending order to 0.0) added in ascending l.  The
// two order statistics s[((m - 1) * 10 + 50) / 100] and s[((m - 1) * 95 + 50) / 100] of the kept windows come from a most-significant-
// digit radix select on the 64-bit patterns (positive finite doubles order as their bit patterns; estimate.hip's fd_select_f32 is the
// float32 precedent): eight passes of 8 bits, one LDS histogram of integer counts per rank and pass -- exact, independent of any order,
// and linear in the number of windows (an hour of audio has 36 000).
#include "measure_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int SUB = 4800;
constexpr int MAX_ROW = 0x7fffffff - 1024;
constexpr int MAX_J = MAX_ROW / SUB;
constexpr double ABS_GATE = 1.1724653045822981e-07;   // loudness.hip's: 10^((-70 + 0.691) / 10)

// ---- true peak ----------------------------------------------------------------------------------------------------------------------------
constexpr int TP_TILE = 1024;             // positions per workgroup
constexpr int TP_PHASES = 4;              // 4x oversampling
constexpr int TP_MAX_W = 256;             // W: half the filter length (align.MAX_W)

// the larger of two non-negative maxima and the OR of two flags, over the wave; lane 0 holds the result
__device__ __forceinline__ void wave_max_flag(double& m, int& bad) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double v = __shfl_down(m, o, 64);
    const int f = __shfl_down(bad, o, 64);
    m = v > m ? v : m;
    bad |= f;
  }
}

__global__ __launch_bounds__(256) void true_peak_tiles(const float* __restrict__ x, const int* __restrict__ lens, int L, const int* __restrict__ lo,
                                                       const int* __restrict__ hi, const double* __restrict__ taps, int W, double* __restrict__ tile_max,
                                                       int ntile) {
  __shared__ float span[TP_TILE + 2 * TP_MAX_W];
  __shared__ double h[TP_PHASES * 2 * TP_MAX_W];
  __shared__ double red_m[4];
  __shared__ int red_f[4];
  const int b = blockIdx.y, t = threadIdx.x;
  const int nt = 2 * W;
  const int len = fd_clip_len(lens, b, L);
  int w0 = lo ? lo[b] : 0, w1 = hi ? hi[b] : len;
  w0 = w0 < 0 ? 0 : (w0 > len ? len : w0);
  w1 = w1 < w0 ? w0 : (w1 > len ? len : w1);
  const long long o0 = (long long)blockIdx.x * TP_TILE;                       // the tile's first position
  const long long first = o0 > w0 ? o0 : w0, last = o0 + TP_TILE < w1 ? o0 + TP_TILE : w1;
  double* __restrict__ dst = tile_max + (size_t)b * ntile + blockIdx.x;
  if (last <= first) {                                                        // no position of the window in this tile (the whole workgroup)
    if (t == 0) *dst = 0.0;
    return;
  }
  const long long m0 = o0 - W + 1;                                            // the sample of span[0]
  const float* __restrict__ row = x + (size_t)b * L;
  for (int i = t; i < TP_TILE + nt - 1; i += 256) {
    const long long m = m0 + i;
    span[i] = (m >= 0 && m < len) ? row[m] : 0.f;
  }
  for (int i = t; i < TP_PHASES * nt; i += 256) h[i] = taps[i];
  __syncthreads();
  double best = 0.0;
  int bad = 0;
  for (int i = t; i < TP_TILE; i += 256) {
    const long long o = o0 + i;
    if (o < first || o >= last) continue;
    double acc[TP_PHASES] = {0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < nt; ++k) {
      const double v = (double)span[i + k];
#pragma unroll
      for (int j = 0; j < TP_PHASES; ++j) {
        const double p = v * h[j * nt + k];
        acc[j] = acc[j] + p;
      }
    }
#pragma unroll
    for (int j = 0; j < TP_PHASES; ++j) {
      const double a = fabs(acc[j]);
      if (!(a - a == 0.0)) bad = 1;             // NaN or Inf
      best = a > best ? a : best;
    }
  }
  wave_max_flag(best, bad);
  if ((t & 63) == 0) {
    red_m[t >> 6] = best;
    red_f[t >> 6] = bad;
  }
  __syncthreads();
  if (t == 0) {
    double m = red_m[0];
    int f = red_f[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      m = red_m[w] > m ? red_m[w] : m;
      f |= red_f[w];
    }
    *dst = f ? fd_nan() : m;
  }
}

__global__ __launch_bounds__(64) void true_peak_finalise(const int* __restrict__ lens, int L, const double* __restrict__ tile_max, int ntile,
                                                         double* __restrict__ p_out) {
  const int b = blockIdx.x, t = threadIdx.x;
  const double* __restrict__ src = tile_max + (size_t)b * ntile;
  double best = 0.0;
  int bad = fd_clip_len(lens, b, L) == 0;
  for (int i = t; i < ntile; i += 64) {
    const double v = src[i];
    if (v != v) bad = 1;
    best = v > best ? v : best;
  }
  wave_max_flag(best, bad);
  if (t == 0) p_out[b] = bad ? fd_nan() : best;
}

inline int tp_tiles(int L) { return (int)(((long long)L + TP_TILE - 1) / TP_TILE); }

// ---- loudness range -----------------------------------------------------------------------------------------------------------------------
constexpr int SHORT_SUBS = 30;            // the short-term window: 3 s
constexpr double SHORT_SAMPLES = 144000.0;
constexpr int LANES = 64;                 // the lanes of the gated sum (loudness.py _lane_sum)
constexpr int RADIX_BITS = 8, RADIX_BINS = 1 << RADIX_BITS, RADIX_PASSES = 64 / RADIX_BITS;

inline int range_windows(int J) { return J >= SHORT_SUBS ? J - SHORT_SUBS + 1 : 0; }

__global__ __launch_bounds__(256) void loudness_range_kernel(const double* __restrict__ E, const int* __restrict__ nsub, int J, double* __restrict__ st_ws,
                                                             int wmax, double* __restrict__ st_out, int* __restrict__ counts_out) {
  __shared__ double pa[LANES];
  __shared__ int hist[2][RADIX_BINS];
  __shared__ unsigned long long s_prefix[2];
  __shared__ int s_rank[2];
  __shared__ int s_cnt, s_cnt2, s_bad;    // windows above the first gate, above both, any window not finite: each written in ONE phase only
  const int b = blockIdx.x, t = threadIdx.x;
  int ns = nsub[b];
  ns = ns < 0 ? 0 : (ns > J ? J : ns);
  const int nwin = ns >= SHORT_SUBS ? ns - SHORT_SUBS + 1 : 0;                 // <= wmax
  const double* __restrict__ e = E + (size_t)b * J;
  double* __restrict__ st = st_ws + (size_t)b * wmax;
  if (t == 0) {
    s_cnt = 0;
    s_cnt2 = 0;
    s_bad = 0;
  }
  __syncthreads();
  int cnt = 0, bad = 0;
  for (int j = t; j < nwin; j += 256) {
    double a = e[j] + e[j + 1];
    for (int k = 2; k < SHORT_SUBS; ++k) a = a + e[j + k];
    const double s = a / SHORT_SAMPLES;
    st[j] = s;
    if (!(s - s == 0.0)) bad = 1;               // NaN or Inf
    if (s > ABS_GATE) ++cnt;
  }
  if (cnt) atomicAdd(&s_cnt, cnt);
  if (bad) atomicOr(&s_bad, 1);
  __syncthreads();                              // the counts, and this workgroup's st[] in global memory
  const int n1 = s_cnt, anybad = s_bad;
  double out_lo = fd_nan(), out_hi = fd_nan();
  int c1 = 0, c2 = 0;
  if (nwin > 0 && !anybad && n1 == 0) out_lo = out_hi = 0.0;
  if (nwin > 0 && !anybad && n1 > 0) {          // (uniform over the workgroup)
    if (t < LANES) {
      double acc = 0.0;
      for (int j = t; j < nwin; j += LANES) {
        const double s = st[j];
        if (s > ABS_GATE) acc = acc + s;
      }
      pa[t] = acc;
    }
    __syncthreads();
    double sum1 = pa[0];
    for (int l = 1; l < LANES; ++l) sum1 = sum1 + pa[l];
    const double mean1 = sum1 / (double)n1;
    const double thr = 0.01 * mean1;
    cnt = 0;
    for (int j = t; j < nwin; j += 256) {
      const double s = st[j];
      if (s > ABS_GATE && s > thr) ++cnt;
    }
    if (cnt) atomicAdd(&s_cnt2, cnt);
    __syncthreads();
    const int m = s_cnt2;                       // >= 1: the largest window above the first gate is above 0.01 of their mean
    unsigned long long prefix[2] = {0ull, 0ull};
    int rank[2] = {(int)((((long long)m - 1) * 10 + 50) / 100), (int)((((long long)m - 1) * 95 + 50) / 100)};
    for (int pass = 0; pass < RADIX_PASSES; ++pass) {
      const int shift = 64 - RADIX_BITS * (pass + 1);
      hist[0][t] = 0;
      hist[1][t] = 0;
      __syncthreads();
      for (int j = t; j < nwin; j += 256) {
        const double s = st[j];
        if (s > ABS_GATE && s > thr) {
          const unsigned long long key = (unsigned long long)__double_as_longlong(s);
          const int bin = (int)((key >> shift) & (RADIX_BINS - 1));
#pragma unroll
          for (int r = 0; r < 2; ++r)
            if (pass == 0 || (key >> (shift + RADIX_BITS)) == prefix[r]) atomicAdd(&hist[r][bin], 1);
        }
      }
      __syncthreads();
      if (t < 2) {                              // thread r walks the bins of rank r: the bin that holds it, and its rank inside that bin
        int below = 0, bin = 0;
        for (; bin < RADIX_BINS - 1; ++bin) {
          const int c = hist[t][bin];
          if (rank[t] < below + c) break;
          below += c;
        }
        s_prefix[t] = (prefix[t] << RADIX_BITS) | (unsigned long long)bin;
        s_rank[t] = rank[t] - below;
      }
      __syncthreads();
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        prefix[r] = s_prefix[r];
        rank[r] = s_rank[r];
      }
    }
    out_lo = __longlong_as_double((long long)prefix[0]);
    out_hi = __longlong_as_double((long long)prefix[1]);
    c1 = n1;
    c2 = m;
  }
  if (t == 0) {
    st_out[2 * b] = out_lo;
    st_out[2 * b + 1] = out_hi;
    counts_out[3 * b] = nwin;
    counts_out[3 * b + 1] = c1;
    counts_out[3 * b + 2] = c2;
  }
}

}  // namespace

extern "C" int fd_true_peak_tile(void) { return TP_TILE; }

extern "C" size_t fd_true_peak_workspace_bytes(int B, int L) {
  if (B <= 0 || B > 65535 || L <= 0 || L > MAX_ROW) return 0;
  return fd_align(sizeof(double) * (size_t)B * tp_tiles(L)) + 256;
}

extern "C" int fd_true_peak(const float* x, const int* lengths, int B, int L, const int* lo, const int* hi, const double* taps, int W, double* p_out,
                            void* ws, size_t ws_bytes, void* stream) {
  FD_REQUIRE(x && lengths && p_out, "fd_true_peak: null pointer");
  FD_REQUIRE(taps, "fd_true_peak: null pointer (taps)");
  FD_REQUIRE((lo == nullptr) == (hi == nullptr), "fd_true_peak: lo and hi are both given or both NULL (NULL: every position of the clip)");
  FD_REQUIRE(B > 0 && B <= 65535, "fd_true_peak: bad batch B %d (1 <= B <= 65535)", B);
  FD_REQUIRE(L > 0 && L <= MAX_ROW, "fd_true_peak: bad row length L %d (1 <= L <= %d)", L, MAX_ROW);
  FD_REQUIRE(W >= 1 && W <= TP_MAX_W, "fd_true_peak: bad half width W %d (1 <= W <= %d: 2 W taps per phase)", W, TP_MAX_W);
  FD_REQUIRE(ws, "fd_true_peak: null pointer (ws)");
  const size_t need = fd_true_peak_workspace_bytes(B, L);
  if (ws_bytes < need) return fd_set_error(FD_ENOMEM, "fd_true_peak: workspace too small (%zu bytes, fd_true_peak_workspace_bytes gives %zu)", ws_bytes, need);
  double* tile_max = reinterpret_cast<double*>(aligned(ws));
  const int ntile = tp_tiles(L);
  hipLaunchKernelGGL(true_peak_tiles, dim3(ntile, B), dim3(256), 0, fd_stream(stream), x, lengths, L, lo, hi, taps, W, tile_max, ntile);
  FD_LAUNCH_CHECK();
  hipLaunchKernelGGL(true_peak_finalise, dim3(B), dim3(64), 0, fd_stream(stream), lengths, L, (const double*)tile_max, ntile, p_out);
  FD_LAUNCH_CHECK();
  return FD_OK;
}

extern "C" size_t fd_loudness_range_workspace_bytes(int B, int Jmax) {
  if (B <= 0 || B > 65535 || Jmax < 0 || Jmax > MAX_J) return 0;
  return fd_align(sizeof(double) * (size_t)B * range_windows(Jmax)) + 256;
}

extern "C" int fd_loudness_range(const double* E, const int* nsub, int B, int Jmax, double* st_out, int* counts_out, void* ws, size_t ws_bytes, void* stream) {
  FD_REQUIRE(nsub && st_out && counts_out, "fd_loudness_range: null pointer");
  FD_REQUIRE(B > 0 && B <= 65535, "fd_loudness_range: bad batch B %d (1 <= B <= 65535)", B);
  FD_REQUIRE(Jmax >= 0 && Jmax <= MAX_J, "fd_loudness_range: bad sub-block count Jmax %d (0 <= Jmax <= %d)", Jmax, MAX_J);
  FD_REQUIRE(E || Jmax == 0, "fd_loudness_range: null pointer (E; it may be NULL only when Jmax is 0)");
  FD_REQUIRE(ws, "fd_loudness_range: null pointer (ws)");
  const size_t need = fd_loudness_range_workspace_bytes(B, Jmax);
  if (ws_bytes < need) return fd_set_error(FD_ENOMEM, "fd_loudness_range: workspace too small (%zu bytes, fd_loudness_range_workspace_bytes gives %zu)", ws_bytes, need);
  hipLaunchKernelGGL(loudness_range_kernel, dim3(B), dim3(256), 0, fd_stream(stream), E, nsub, Jmax, reinterpret_cast<double*>(aligned(ws)),
                     range_windows(Jmax), st_out, counts_out);
  FD_LAUNCH_CHECK();
  return FD_OK;
}
