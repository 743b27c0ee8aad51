// specdist.hip -- the multi-scale STFT distance and the multi-scale mel distance of ragged batches on the GPU (include/flowdec_hip.h
// "Spectral distances"; host yardsticks: flowdec_amd/specdist.py).
//
// The contract of metrics.hip holds: a clip's result has the same BITS alone, in a batch, at any batch position and next to clips of any
// other lengths.  Every partition and every order of summation below is a function of the clip's own length only, every reduction runs
// in a fixed order, and there are no atomics.
//
// One kernel per log2 N in 7..12; no spectrum is ever written to memory (the operator-level call aside).  A workgroup of 256 threads takes
// FPB = max(1, 1024 / N) frame pairs of one clip, TPF = 256 / FPB threads each:
//   load      the N samples of frame t of x_hat and x straight from the rows with the clip's own reflect indices, times the periodic Hann
//             window (one rounding), as z = w x_hat + i w x, into LDS at the bit-reversed position
//   FFT       fft_lds.h (shared with segsnr.hip): radix-2 decimation-in-time butterflies u +- W v, two stages per LDS pass, in place,
//             natural order out.  Twiddles W_N^m = (cos, -sin)(2 pi m / N), m < N / 2, from the plan's table.
//   unpack    A_k = (Z_k + conj Z_{N-k}) / 2, R_k = (Z_k - conj Z_{N-k}) / 2i for k = 0..N/2, |.| in float32
//   epilogue  the STFT terms per bin in float64; P = |.|^2 of both signals into LDS; per mel filter the band's weighted sum in float64 in
//             ascending bin order, rounded to float32, the mel term in float64; the frame's three sums by a fixed tree over its threads (then its waves in order)
//   finalise  one workgroup per clip adds the frames' partials scale by scale (thread i: frames i, i + 256, ..; then the tree) and divides
//
// x_hat == x gives exactly 0: with equal real and imaginary parts going in, A_k and R_k come out equal BIT FOR BIT (fft_lds.h says why).
#include <math.h>

#include <vector>

#include "fft_lds.h"
#include "internal.h"
#include "measure_common.h"

namespace {
constexpr int MAX_SCALES = 16;
constexpr double CLAMP = 1e-5;     // clamp_eps of both losses
}  // namespace

struct fd_specdist_plan {
  int sr, n_scales, max_n;
  int log2n[MAX_SCALES], n_mels[MAX_SCALES], stft[MAX_SCALES];
  float* win[MAX_SCALES];      // device [N]
  float2* tw[MAX_SCALES];      // device [N / 2]
  int* band[MAX_SCALES];       // device [3][n_mels]: first bin, count, offset into wgt
  float* wgt[MAX_SCALES];      // device [sum of count]
};

namespace {

using fft_lds::padi;

template <int LOG2N>
struct Geo : fft_lds::Geo<LOG2N> {
  static constexpr int F = fft_lds::Geo<LOG2N>::N / 2 + 1, HOP = fft_lds::Geo<LOG2N>::N / 4;
};

__device__ __forceinline__ float mag_of(float re, float im) { return sqrtf(__fmaf_rn(re, re, __fmul_rn(im, im))); }

__device__ __forceinline__ double log_ratio(double a, double b) {
  return fabs(2.0 * log10((a < CLAMP ? CLAMP : a) / (b < CLAMP ? CLAMP : b)));
}

// a clip's own frame count at hop `hop`, 0 for a length outside (min_len, L]
__device__ __forceinline__ int frames_of(const int* __restrict__ lens, int b, int L, int min_len, int hop) {
  const int l = lens[b];
  return (l <= min_len || l > L) ? 0 : 1 + l / hop;
}

// partial[b][t][0..2] = the frame's sums of the stft log, stft mag and mel log terms (only frames t < T_b are written).
// mag_hat / mag_x [B][T][F], mel_hat / mel_x [B][T][n_mels]: the operator-level outputs (all frames t < T), or null.
template <int LOG2N>
__global__ __launch_bounds__(256) void specdist_kernel(const float* __restrict__ xh, const float* __restrict__ x, const int* __restrict__ lens, int L,
                                                       int min_len, int T, const float* __restrict__ win, const float2* __restrict__ tw,
                                                       const int* __restrict__ band, const float* __restrict__ wgt, int n_mels, int stft,
                                                       double* __restrict__ partial, float* __restrict__ mag_hat, float* __restrict__ mag_x,
                                                       float* __restrict__ mel_hat, float* __restrict__ mel_x) {
  using G = Geo<LOG2N>;
  constexpr int N = G::N, F = G::F, TPF = G::TPF;
  __shared__ float2 buf[G::FPB * G::NP];
  __shared__ float pw[2][G::FPB * F];
  __shared__ double red[4][3];
  const int b = blockIdx.y, t0 = blockIdx.x * G::FPB;
  const int len = lens[b];
  const int Tb = frames_of(lens, b, L, min_len, G::HOP);
  if (t0 >= Tb && !mag_hat) return;                           // (workgroup-uniform)
  const int fr = threadIdx.x / TPF, lt = threadIdx.x % TPF, t = t0 + fr;
  const bool live = t < Tb;
  float2* __restrict__ z = buf + fr * G::NP;
  const float* __restrict__ rh = xh + (size_t)b * L;
  const float* __restrict__ rx = x + (size_t)b * L;

  for (int n = lt; n < N; n += TPF) {
    float2 v = make_float2(0.f, 0.f);
    if (live) {
      int m = t * G::HOP + n - N / 2;                         // t hop <= len and len > N / 2: one reflection lands inside [0, len)
      if (m < 0) m = -m;
      if (m >= len) m = 2 * (len - 1) - m;
      const float w = win[n];
      v = make_float2(__fmul_rn(w, rh[m]), __fmul_rn(w, rx[m]));
    }
    z[fft_lds::bitrev_slot<LOG2N>(n)] = v;
  }
  __syncthreads();

  fft_lds::passes<LOG2N>(z, tw, lt);

  double acc[3] = {0.0, 0.0, 0.0};
  float* __restrict__ ph = pw[0] + fr * F;
  float* __restrict__ px = pw[1] + fr * F;
  const size_t row = (size_t)b * T + t;
  for (int k = lt; k <= N / 2; k += TPF) {
    const float2 zk = z[padi(k)], zn = z[padi((N - k) & (N - 1))];
    const float2 ak = fft_lds::unpack_re(zk, zn), rk = fft_lds::unpack_im(zk, zn);
    const float a = mag_of(ak.x, ak.y), r = mag_of(rk.x, rk.y);
    ph[k] = __fmul_rn(a, a);
    px[k] = __fmul_rn(r, r);
    if (stft) {
      acc[0] += log_ratio((double)a, (double)r);
      acc[1] += fabs((double)a - (double)r);
    }
    if (mag_hat && t < T) {
      mag_hat[row * F + k] = a;
      mag_x[row * F + k] = r;
    }
  }
  if (n_mels > 0) {
    __syncthreads();
    for (int j = lt; j < n_mels; j += TPF) {
      const int f0 = band[j], cnt = band[n_mels + j];
      const float* __restrict__ w = wgt + band[2 * n_mels + j];
      double mh = 0.0, mx = 0.0;
      for (int i = 0; i < cnt; ++i) {
        const double wi = (double)w[i];
        mh += wi * (double)ph[f0 + i];
        mx += wi * (double)px[f0 + i];
      }
      const float Mh = (float)mh, Mx = (float)mx;
      acc[2] += log_ratio((double)Mh, (double)Mx);
      if (mel_hat && t < T) {
        mel_hat[row * n_mels + j] = Mh;
        mel_x[row * n_mels + j] = Mx;
      }
    }
  }
  if (!partial) return;                                       // (uniform)

  // the frame's sums: a tree over its threads within a wave, then the frame's waves in index order.  This is fft_lds::frame_all's order
  // (lane 0 of the frame gets the same operands at every level) written for lane 0 alone: only lane 0 stores, so the sums need not reach
  // the frame's other threads, and that saves frame_all's second barrier and its 3 WPF LDS reads a thread.
  constexpr int W = TPF < 64 ? TPF : 64, WPF = TPF / W;      // lanes of a frame in one wave, waves of a frame
#pragma unroll
  for (int q = 0; q < 3; ++q) {
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) acc[q] += __shfl_down(acc[q], o, 64);
  }
  if (WPF > 1) {
    if ((threadIdx.x & 63) == 0) {
      red[threadIdx.x >> 6][0] = acc[0]; red[threadIdx.x >> 6][1] = acc[1]; red[threadIdx.x >> 6][2] = acc[2];
    }
    __syncthreads();
    if (lt < 3 && live) {
      double v = red[fr * WPF][lt];
#pragma unroll
      for (int w = 1; w < WPF; ++w) v += red[fr * WPF + w][lt];
      partial[row * 3 + lt] = v;
    }
  } else if (lt == 0 && live) {
    partial[row * 3 + 0] = acc[0];
    partial[row * 3 + 1] = acc[1];
    partial[row * 3 + 2] = acc[2];
  }
}

struct fin_args {
  int n_scales, min_len;
  int hop[MAX_SCALES], F[MAX_SCALES], n_mels[MAX_SCALES], stft[MAX_SCALES], T[MAX_SCALES];
  long long off[MAX_SCALES];        // the scale's partials, in doubles from the base
};

// out[b] = msstft, mel; terms[b][s] = the three means of scale s.  NaN in all of it for a length the transforms cannot take.
__global__ __launch_bounds__(256) void specdist_finalise_kernel(fin_args a, const double* __restrict__ partial, const int* __restrict__ lens, int L,
                                                                double* __restrict__ out, double* __restrict__ terms) {
  const int b = blockIdx.x;
  const double nan = fd_nan();
  double msstft = 0.0, mel = 0.0;
  for (int s = 0; s < a.n_scales; ++s) {
    const int Tb = frames_of(lens, b, L, a.min_len, a.hop[s]);
    if (Tb == 0) {                                            // (uniform; the same at every scale)
      if (threadIdx.x == 0) {
        if (terms) for (int q = 0; q < 3; ++q) terms[((size_t)b * a.n_scales + s) * 3 + q] = nan;
        msstft = mel = nan;
      }
      continue;
    }
    const double* __restrict__ p = partial + a.off[s] + (size_t)b * a.T[s] * 3;
    double acc[3] = {0.0, 0.0, 0.0};
    for (int t = threadIdx.x; t < Tb; t += 256) {
      acc[0] += p[(size_t)t * 3 + 0];
      acc[1] += p[(size_t)t * 3 + 1];
      acc[2] += p[(size_t)t * 3 + 2];
    }
    fd_block_sums<3>(acc);
    if (threadIdx.x == 0) {
      double (&m)[3] = acc;
      m[0] = a.stft[s] ? m[0] / ((double)a.F[s] * (double)Tb) : 0.0;
      m[1] = a.stft[s] ? m[1] / ((double)a.F[s] * (double)Tb) : 0.0;
      m[2] = a.n_mels[s] > 0 ? m[2] / ((double)a.n_mels[s] * (double)Tb) : 0.0;
      if (a.stft[s]) msstft += m[0] + m[1];
      if (a.n_mels[s] > 0) mel += m[2];
      if (terms) for (int q = 0; q < 3; ++q) terms[((size_t)b * a.n_scales + s) * 3 + q] = m[q];
    }
    __syncthreads();                                          // the last readers of fd_block_sums' red
  }
  if (threadIdx.x == 0) {
    out[b * 2 + 0] = msstft;
    out[b * 2 + 1] = mel;
  }
}

// ---- host: the tables ---------------------------------------------------------------------------------------------------------------
// cos and sin of 2 pi m / N for 0 <= m <= N / 2, the phase reduced to the first octant in integers
void unit(int m, int N, double* c, double* s) {
  const bool mirror = m > N / 4;                  // pi - theta: cos changes sign
  int r = mirror ? N / 2 - m : m;                 // in [0, N / 4]
  double cr, sr;
  if (r <= N / 8) { cr = cos(2.0 * PI * r / N); sr = sin(2.0 * PI * r / N); }
  else { cr = sin(2.0 * PI * (N / 4 - r) / N); sr = cos(2.0 * PI * (N / 4 - r) / N); }
  if (r == N / 4) { cr = 0.0; sr = 1.0; }
  *c = mirror ? -cr : cr;
  *s = sr;
}

bool size_ok(int N) { return N >= (1 << fft_lds::MIN_LOG2N) && N <= (1 << fft_lds::MAX_LOG2N) && (N & (N - 1)) == 0; }

int log2_of(int N) { int l = 0; while ((1 << l) < N) ++l; return l; }

double hz_to_mel(double f) { return 2595.0 * log10(1.0 + f / 700.0); }

// fb [F][n_mels] in float64 (the header's definition; flowdec_amd/specdist.py mel_filterbank is the same arithmetic, operation by operation)
std::vector<double> mel_bank(int sr, int N, int n_mels) {
  const int F = N / 2 + 1;
  const double fmax = (double)(sr / 2);
  std::vector<double> freqs(F), pts(n_mels + 2);
  const double fstep = fmax / (double)(F - 1);
  for (int f = 0; f < F; ++f) freqs[f] = (double)f * fstep;
  freqs[F - 1] = fmax;
  const double m_max = hz_to_mel(fmax), mstep = m_max / (double)(n_mels + 1);
  for (int i = 0; i < n_mels + 2; ++i) {
    const double m = i == n_mels + 1 ? m_max : (double)i * mstep;
    pts[i] = 700.0 * (pow(10.0, m / 2595.0) - 1.0);
  }
  std::vector<double> fb((size_t)F * n_mels);
  for (int f = 0; f < F; ++f)
    for (int j = 0; j < n_mels; ++j) {
      const double down = (freqs[f] - pts[j]) / (pts[j + 1] - pts[j]);
      const double up = (pts[j + 2] - freqs[f]) / (pts[j + 2] - pts[j + 1]);
      const double v = down < up ? down : up;
      fb[(size_t)f * n_mels + j] = (v > 0.0 ? v : 0.0) * (2.0 / (pts[j + 2] - pts[j]));
    }
  return fb;
}

struct banded { std::vector<int> first, count, off; std::vector<float> w; };

// -> false when a filter is empty or its non-zero weights (as float32) are not one contiguous run
bool band_of(const std::vector<double>& fb, int F, int n_mels, banded* out) {
  out->first.assign(n_mels, 0); out->count.assign(n_mels, 0); out->off.assign(n_mels, 0); out->w.clear();
  for (int j = 0; j < n_mels; ++j) {
    int lo = -1, hi = -1, nz = 0;
    for (int f = 0; f < F; ++f)
      if ((float)fb[(size_t)f * n_mels + j] != 0.f) { if (lo < 0) lo = f; hi = f; ++nz; }
    if (nz == 0 || nz != hi - lo + 1) return false;
    out->first[j] = lo; out->count[j] = nz; out->off[j] = (int)out->w.size();
    for (int f = lo; f <= hi; ++f) out->w.push_back((float)fb[(size_t)f * n_mels + j]);
  }
  return true;
}

int tables_check(const char* who, int sr, int N, int n_mels) {
  FD_REQUIRE(size_ok(N), "%s: the window length must be a power of two in [128, 4096] (got %d)", who, N);
  FD_REQUIRE(n_mels >= 0 && n_mels <= N / 2, "%s: n_mels %d outside [0, N / 2 = %d]", who, n_mels, N / 2);
  FD_REQUIRE(n_mels == 0 || (sr >= 2 && sr <= (1 << 24)), "%s: the rate must be in [2, 2^24] (got %d)", who, sr);
  return FD_OK;
}

struct layout { long long off[MAX_SCALES]; int T[MAX_SCALES]; size_t total; };

bool layout_of(const fd_specdist_plan* p, int B, int L, layout* s) {
  if (!p || B < 1 || B > 65535 || L <= p->max_n / 2) return false;
  long long doubles = 0;
  for (int i = 0; i < p->n_scales; ++i) {
    s->T[i] = 1 + L / ((1 << p->log2n[i]) / 4);
    s->off[i] = doubles;
    doubles += (long long)B * s->T[i] * 3;
  }
  s->total = fd_align(sizeof(double) * (size_t)doubles) + 256;
  return true;
}

void launch(const fd_specdist_plan* p, int i, const float* xh, const float* x, const int* lens, int B, int L, int T, double* partial, float* mag_hat,
            float* mag_x, float* mel_hat, float* mel_x, hipStream_t st) {
  fft_lds::dispatch(p->log2n[i], [&](auto k) {
    constexpr int LOG2N = decltype(k)::value;
    hipLaunchKernelGGL(specdist_kernel<LOG2N>, dim3(fd_cdiv(T, Geo<LOG2N>::FPB), B), dim3(256), 0, st, xh, x, lens, L, p->max_n / 2, T, p->win[i], p->tw[i],
                       p->band[i], p->wgt[i], p->n_mels[i], p->stft[i], partial, mag_hat, mag_x, mel_hat, mel_x);
  });
}

// the checks the two entry points share
int call_check(const char* who, const fd_specdist_plan* plan, int B, int L, size_t ws_bytes, layout* s) {
  FD_REQUIRE(B >= 1 && B <= 65535 && L >= 1, "%s: bad batch B %d L %d (1 <= B <= 65535, L >= 1)", who, B, L);
  FD_REQUIRE(L > plan->max_n / 2, "%s: a clip of %d samples cannot be reflect-padded by %d (the largest window, %d, needs at least %d samples)", who, L,
             plan->max_n / 2, plan->max_n, plan->max_n / 2 + 1);
  layout_of(plan, B, L, s);
  FD_REQUIRE(ws_bytes >= s->total, "%s: workspace too small (%zu < %zu bytes, fd_metrics_specdist_workspace_bytes)", who, ws_bytes, s->total);
  return FD_OK;
}

}  // namespace

extern "C" int fd_specdist_tables(int sr, int N, int n_mels, float* window, float* twiddle, int* first, int* count, float* weights) {
  FD_TRY(tables_check("fd_specdist_tables", sr, N, n_mels));
  banded bd;
  if (n_mels > 0) FD_REQUIRE(band_of(mel_bank(sr, N, n_mels), N / 2 + 1, n_mels, &bd), "fd_specdist_tables: a filter of the (%d Hz, N %d, %d mels) "
                             "bank is empty or not one run of bins", sr, N, n_mels);
  if (!window && !twiddle && !first && !count && !weights) return (int)bd.w.size();
  FD_REQUIRE(window && twiddle && (n_mels == 0 || (first && count && weights)), "fd_specdist_tables: null pointer");
  for (int k = 0; k < N; ++k) {
    double c, s;
    unit(k <= N / 2 ? k : N - k, N, &c, &s);
    window[k] = (float)(0.5 - 0.5 * c);
  }
  for (int m = 0; m < N / 2; ++m) {
    double c, s;
    unit(m, N, &c, &s);
    twiddle[2 * m] = (float)c;
    twiddle[2 * m + 1] = (float)-s;
  }
  for (int j = 0; j < n_mels; ++j) { first[j] = bd.first[j]; count[j] = bd.count[j]; }
  for (size_t i = 0; i < bd.w.size(); ++i) weights[i] = bd.w[i];
  return (int)bd.w.size();
}

extern "C" void fd_specdist_plan_destroy(fd_specdist_plan* p) {
  if (!p) return;
  for (int i = 0; i < p->n_scales; ++i) {
    if (p->win[i]) (void)hipFree(p->win[i]);
    if (p->tw[i]) (void)hipFree(p->tw[i]);
    if (p->band[i]) (void)hipFree(p->band[i]);
    if (p->wgt[i]) (void)hipFree(p->wgt[i]);
  }
  delete p;
}

extern "C" int fd_specdist_plan_create(int sr, int n_scales, const int* window_lengths, const int* n_mels, const int* stft_term, fd_specdist_plan** out) {
  FD_REQUIRE(out, "fd_specdist_plan_create: null out");
  *out = nullptr;
  FD_REQUIRE(window_lengths && n_mels && stft_term, "fd_specdist_plan_create: null pointer");
  FD_REQUIRE(n_scales >= 1 && n_scales <= MAX_SCALES, "fd_specdist_plan_create: n_scales %d outside [1, %d]", n_scales, MAX_SCALES);
  std::vector<banded> bands(n_scales);
  for (int i = 0; i < n_scales; ++i) {
    FD_TRY(tables_check("fd_specdist_plan_create", sr, window_lengths[i], n_mels[i]));
    FD_REQUIRE(n_mels[i] > 0 || stft_term[i], "fd_specdist_plan_create: scale %d (N %d) has neither an STFT term nor a mel term", i, window_lengths[i]);
    if (n_mels[i] > 0)
      FD_REQUIRE(band_of(mel_bank(sr, window_lengths[i], n_mels[i]), window_lengths[i] / 2 + 1, n_mels[i], &bands[i]), "fd_specdist_plan_create: a filter of "
                 "the (%d Hz, N %d, %d mels) bank is empty or not one run of bins", sr, window_lengths[i], n_mels[i]);
  }
  fd_specdist_plan* p = new fd_specdist_plan();
  p->sr = sr; p->n_scales = n_scales; p->max_n = 0;
  for (int i = 0; i < MAX_SCALES; ++i) { p->win[i] = nullptr; p->tw[i] = nullptr; p->band[i] = nullptr; p->wgt[i] = nullptr; }
  hipError_t e = hipSuccess;
  for (int i = 0; i < n_scales && e == hipSuccess; ++i) {
    const int N = window_lengths[i], nm = n_mels[i];
    p->log2n[i] = log2_of(N); p->n_mels[i] = nm; p->stft[i] = stft_term[i] ? 1 : 0;
    p->max_n = N > p->max_n ? N : p->max_n;
    std::vector<float> win(N), tw(N);
    std::vector<int> band(3 * (size_t)nm);
    std::vector<float> w(bands[i].w.size());
    fd_specdist_tables(sr, N, nm, win.data(), tw.data(), band.data(), band.data() + nm, w.data());
    for (int j = 0; j < nm; ++j) band[2 * nm + j] = bands[i].off[j];
    e = upload(&p->win[i], win.data(), win.size());
    if (e == hipSuccess) e = upload(reinterpret_cast<float**>(&p->tw[i]), tw.data(), tw.size());
    if (e == hipSuccess) e = upload(&p->band[i], band.data(), band.size());
    if (e == hipSuccess) e = upload(&p->wgt[i], w.data(), w.size());
  }
  if (e != hipSuccess) {
    fd_specdist_plan_destroy(p);
    return fd_set_error(FD_ERUNTIME, "fd_specdist_plan_create: uploading the tables failed: %s", hipGetErrorString(e));
  }
  *out = p;
  return FD_OK;
}

extern "C" size_t fd_metrics_specdist_workspace_bytes(const fd_specdist_plan* plan, int B, int L) {
  layout s;
  return layout_of(plan, B, L, &s) ? s.total : 0;
}

extern "C" int fd_metrics_specdist(const fd_specdist_plan* plan, const float* x_hat, const float* x, const int* lengths, int B, int L, double* out,
                                   double* terms, void* ws, size_t ws_bytes, void* stream) {
  FD_REQUIRE(plan && x_hat && x && lengths && out && ws, "fd_metrics_specdist: null pointer");
  layout s;
  FD_TRY(call_check("fd_metrics_specdist", plan, B, L, ws_bytes, &s));
  hipStream_t st = fd_stream(stream);
  double* partial = reinterpret_cast<double*>(aligned(ws));
  fin_args a;
  a.n_scales = plan->n_scales; a.min_len = plan->max_n / 2;
  for (int i = 0; i < plan->n_scales; ++i) {
    const int N = 1 << plan->log2n[i];
    a.hop[i] = N / 4; a.F[i] = N / 2 + 1; a.n_mels[i] = plan->n_mels[i]; a.stft[i] = plan->stft[i]; a.T[i] = s.T[i]; a.off[i] = s.off[i];
    launch(plan, i, x_hat, x, lengths, B, L, s.T[i], partial + s.off[i], nullptr, nullptr, nullptr, nullptr, st);
  }
  hipLaunchKernelGGL(specdist_finalise_kernel, dim3(B), dim3(256), 0, st, a, partial, lengths, L, out, terms);
  FD_LAUNCH_CHECK();
  return FD_OK;
}

extern "C" int fd_metrics_specdist_spectra(const fd_specdist_plan* plan, int scale, const float* x_hat, const float* x, const int* lengths, int B, int L,
                                           float* mag_hat, float* mag_x, float* mel_hat, float* mel_x, void* ws, size_t ws_bytes, void* stream) {
  FD_REQUIRE(plan && x_hat && x && lengths && mag_hat && mag_x && ws, "fd_metrics_specdist_spectra: null pointer");
  FD_REQUIRE(scale >= 0 && scale < plan->n_scales, "fd_metrics_specdist_spectra: scale %d outside [0, %d)", scale, plan->n_scales);
  FD_REQUIRE((mel_hat == nullptr) == (mel_x == nullptr), "fd_metrics_specdist_spectra: mel_hat and mel_x go together");
  FD_REQUIRE(!mel_hat || plan->n_mels[scale] > 0, "fd_metrics_specdist_spectra: scale %d has no mel term", scale);
  layout s;
  FD_TRY(call_check("fd_metrics_specdist_spectra", plan, B, L, ws_bytes, &s));
  launch(plan, scale, x_hat, x, lengths, B, L, s.T[scale], nullptr, mag_hat, mag_x, mel_hat, mel_x, fd_stream(stream));
  FD_LAUNCH_CHECK();
  return FD_OK;
}
