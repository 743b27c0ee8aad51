// segsnr.hip -- the segmental SNR and the frequency-weighted segmental SNR (Hu & Loizou's comp_snr.m / comp_fwseg.m as the pysepm package
// restates them; the reference's default metrics `SSNR` and `fwSSNR`) of ragged batches on the GPU (include/flowdec_hip.h "Segmental
// SNRs"; host yardstick and the definitions in full: flowdec_amd/segsnr.py).
//
// The contract of metrics.hip holds: a clip's result has the same BITS alone, in a batch, at any batch position and next to clips of any
// other lengths.  Every partition and every order of summation below is a function of the clip's own length only, every reduction runs
// in a fixed order, and there are no atomics.
//
// Both metrics use the same frames: win = round(0.03 sr) samples at hop skip = floor(0.0075 sr), frame t = samples [t skip, t skip + win),
// T_b = (len - win) / skip of them (no centring, no reflection, the last full frame dropped), n_fft = 2^ceil(log2(2 win)).
//
// One kernel per log2 n_fft in 7..12.  A workgroup of 256 threads takes FPB = max(1, 1024 / n_fft) frame pairs of one clip, TPF = 256 / FPB
// threads each (fft_lds.h):
//   energies  a = w x, b = w x_hat in float64 (each product rounded), sum a^2 and sum (a - b)^2 in float64: thread lt adds its samples
//             n = lt, lt + TPF, .. in ascending order, then a fixed tree over the frame's lanes and its waves in index order
//             -> SSNR_t = clip(10 log10(sum a^2 / (sum (a - b)^2 + eps) + eps), -10, 35)
//   scale     a' = w (x + eps), b' = w (x_hat + eps) in float64; the frame's peak |a'| and |b'| (a maximum: no order to fix); each signal
//             times the exact power of two that brings ITS peak into [1, 2), then rounded to float32.  The measure divides each
//             spectrum by its own sum, so the scale cancels -- and without it the packed transform below would replace the spectrum of a
//             silent (eps w, 1e-16) or very quiet frame by the rounding noise of the other signal, 2^-24 of ITS size
//   FFT       z = b' + i a' through fft_lds.h's float32 passes; unpacked as specdist.hip unpacks
//   spectrum  |.| of bins 0 .. n_fft / 2 - 1 in float64 from the float32 parts, kept in the transform's own LDS row (bin k of x_hat in
//             slot k, bin k of x in slot n_fft - k; bin 0 of x in the slot of the Nyquist bin, which the measure drops); each signal's sum
//             over the bins: thread lt its bins in ascending order, then the same fixed tree
//   bands     thread j < 25: ce_j = sum_i wgt[i] (|X_i| / sum |X|) over the filter's own bins in ascending order, pe_j likewise, float64;
//             W_j = ce_j^0.2, W_j 10 log10(ce_j^2 / max((ce_j - pe_j)^2, eps)); the two sums over j by a fixed tree over 32 lanes
//             -> fwSSNR_t = clip(sum / sum W, -10, 35)
//   finalise  one workgroup per clip adds the frames' values (thread i: frames i, i + 256, ..; then the tree) and divides by T_b
//
// x_hat == x gives equal peaks, equal scales and equal parts, so both spectra come out equal bit for bit (fft_lds.h), err = eps in every
// band and the frame scores 35 exactly unless a band's energy is below 1e-8 or so (a silent frame).
#include <math.h>

#include <vector>

#include "fft_lds.h"
#include "internal.h"
#include "measure_common.h"

struct fd_segsnr_plan {
  int sr, win, skip, log2n;
  double* window;   // device [win]
  float2* tw;       // device [n_fft / 2]
  int* band;        // device [3][25]: first bin, count, offset into wgt
  double* wgt;      // device [sum of count]
};

namespace {

using fft_lds::frame_all;
using fft_lds::padi;

constexpr int NBANDS = 25;
constexpr double EPS = 2.220446049250313e-16;     // 2^-52
constexpr double LO = -10.0, HI = 35.0;

const double CENT[NBANDS] = {50.0, 120.0, 190.0, 260.0, 330.0, 400.0, 470.0, 540.0, 617.372, 703.378, 798.717, 904.128, 1020.38, 1148.30, 1288.72,
                             1442.54, 1610.70, 1794.16, 1993.93, 2211.08, 2446.71, 2701.97, 2978.04, 3276.17, 3597.63};
const double BAND[NBANDS] = {70.0, 70.0, 70.0, 70.0, 70.0, 70.0, 70.0, 77.3724, 86.0056, 95.3398, 105.411, 116.256, 127.914, 140.423,
                             153.823, 168.154, 183.457, 199.776, 217.153, 235.631, 255.255, 276.072, 298.126, 321.465, 346.136};

// a clip's own frame count, 0 for a length outside [win + skip, L]
__device__ __forceinline__ int frames_of(const int* __restrict__ lens, int b, int L, int win, int skip) {
  const int l = lens[b];
  return (l < win + skip || l > L) ? 0 : (l - win) / skip;
}

__device__ __forceinline__ double clip_db(double v) { return v < LO ? LO : (v > HI ? HI : v); }      // (NaN stays NaN)

// the power of two that brings peak into [1, 2); 1 for a peak of 0 (or one that is not a normal number)
__device__ __forceinline__ double pow2_scale(double peak) {
  const int e = (int)((__double_as_longlong(peak) >> 52) & 0x7ff);
  return (e < 1 || e > 2045) ? 1.0 : __longlong_as_double((long long)(2046 - e) << 52);
}

// a double in one float2 slot of the transform's row
__device__ __forceinline__ void put_double(float2* __restrict__ z, int slot, double v) {
  z[slot] = make_float2(__int_as_float(__double2loint(v)), __int_as_float(__double2hiint(v)));
}
__device__ __forceinline__ double get_double(const float2* __restrict__ z, int slot) {
  const float2 v = z[slot];
  return __hiloint2double(__float_as_int(v.y), __float_as_int(v.x));
}

// partial[b][t][0..1] = fwSSNR_t, SSNR_t of the frames t < T_b; frames [B][T][2] (or null): the same, NaN in the frames t >= T_b.
template <int LOG2N>
__global__ __launch_bounds__(256) void segsnr_kernel(const float* __restrict__ xh, const float* __restrict__ x, const int* __restrict__ lens, int L, int win,
                                                     int skip, int T, const double* __restrict__ window, const float2* __restrict__ tw,
                                                     const int* __restrict__ band, const double* __restrict__ wgt, double* __restrict__ partial,
                                                     double* __restrict__ frames) {
  using G = fft_lds::Geo<LOG2N>;
  constexpr int N = G::N, TPF = G::TPF;
  __shared__ float2 buf[G::FPB * G::NP];
  __shared__ double red[4][4];
  const int b = blockIdx.y, t0 = blockIdx.x * G::FPB;
  const int Tb = frames_of(lens, b, L, win, skip);
  const int fr = threadIdx.x / TPF, lt = threadIdx.x % TPF, t = t0 + fr;
  if (t0 >= Tb) {                                             // (workgroup-uniform)
    if (frames && lt == 0 && t < T) {
      frames[((size_t)b * T + t) * 2 + 0] = fd_nan();
      frames[((size_t)b * T + t) * 2 + 1] = fd_nan();
    }
    return;
  }
  const bool live = t < Tb;
  float2* __restrict__ z = buf + fr * G::NP;
  // t < Tb: t skip + win - 1 <= len - skip - 1, inside the clip
  const float* __restrict__ rh = xh + (size_t)b * L + (size_t)(live ? t : 0) * skip;
  const float* __restrict__ rx = x + (size_t)b * L + (size_t)(live ? t : 0) * skip;

  double e[4] = {0.0, 0.0, 0.0, 0.0};                         // sum a^2, sum (a - b)^2 | peak |a'|, peak |b'|
  double pk[2] = {0.0, 0.0};
  if (live) {
    for (int n = lt; n < win; n += TPF) {
      const double w = window[n], xs = (double)rx[n], hs = (double)rh[n];
      const double a = __dmul_rn(w, xs), bb = __dmul_rn(w, hs);
      const double d = __dsub_rn(a, bb);
      e[0] = __dadd_rn(e[0], __dmul_rn(a, a));
      e[1] = __dadd_rn(e[1], __dmul_rn(d, d));
      pk[0] = fmax(pk[0], fabs(__dmul_rn(w, __dadd_rn(xs, EPS))));
      pk[1] = fmax(pk[1], fabs(__dmul_rn(w, __dadd_rn(hs, EPS))));
    }
  }
  {
    double s[2] = {e[0], e[1]};
    frame_all<TPF, 2, false>(s, red, fr);
    e[0] = s[0]; e[1] = s[1];
    frame_all<TPF, 2, true>(pk, red, fr);
  }
  const double sa = pow2_scale(pk[0]), sb = pow2_scale(pk[1]);
  for (int n = lt; n < N; n += TPF) {
    float2 v = make_float2(0.f, 0.f);
    if (live && n < win) {
      const double w = window[n];
      const double ap = __dmul_rn(w, __dadd_rn((double)rx[n], EPS)), bp = __dmul_rn(w, __dadd_rn((double)rh[n], EPS));
      v = make_float2((float)__dmul_rn(bp, sb), (float)__dmul_rn(ap, sa));
    }
    z[fft_lds::bitrev_slot<LOG2N>(n)] = v;
  }
  __syncthreads();
  fft_lds::passes<LOG2N>(z, tw, lt);

  // the magnitudes, in place: the thread of bin k owns the slots k and N - k (bin 0: slots 0 and N / 2)
  double sum[2] = {0.0, 0.0};                                 // sum |X_hat|, sum |X|
  for (int k = lt; k < N / 2; k += TPF) {
    const int sk = padi(k), sn = padi(k == 0 ? N / 2 : N - k);
    const float2 zk = z[sk], zn = z[padi((N - k) & (N - 1))];
    const float2 pk2 = fft_lds::unpack_re(zk, zn), ck = fft_lds::unpack_im(zk, zn);
    const double mp = sqrt(__dadd_rn(__dmul_rn((double)pk2.x, (double)pk2.x), __dmul_rn((double)pk2.y, (double)pk2.y)));
    const double mc = sqrt(__dadd_rn(__dmul_rn((double)ck.x, (double)ck.x), __dmul_rn((double)ck.y, (double)ck.y)));
    put_double(z, sk, mp);
    put_double(z, sn, mc);
    sum[0] = __dadd_rn(sum[0], mp);
    sum[1] = __dadd_rn(sum[1], mc);
  }
  frame_all<TPF, 2, false>(sum, red, fr);
  if (G::TPF <= 64) __syncthreads();                          // (frame_all had no barrier: the magnitudes become visible here)

  double num = 0.0, den = 0.0;
  if (lt < NBANDS) {
    const int f0 = band[lt], cnt = band[NBANDS + lt];
    const double* __restrict__ wj = wgt + band[2 * NBANDS + lt];
    double ce = 0.0, pe = 0.0;
    for (int i = 0; i < cnt; ++i) {
      const int k = f0 + i;
      const double mp = get_double(z, padi(k)), mc = get_double(z, padi(k == 0 ? N / 2 : N - k));
      ce = __dadd_rn(ce, __dmul_rn(wj[i], mc / sum[1]));
      pe = __dadd_rn(pe, __dmul_rn(wj[i], mp / sum[0]));
    }
    const double dd = __dsub_rn(ce, pe);
    double err = __dmul_rn(dd, dd);
    err = err > EPS ? err : EPS;
    den = pow(ce, 0.2);
    num = __dmul_rn(den, 10.0 * log10(__dmul_rn(ce, ce) / err));
  }
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) {                          // lanes 0..31 of the frame's first wave (TPF >= 32)
    num = __dadd_rn(num, __shfl_down(num, o, 32));
    den = __dadd_rn(den, __shfl_down(den, o, 32));
  }
  if (lt == 0 && live) {
    const double fw = clip_db(num / den);
    const double ss = clip_db(10.0 * log10(e[0] / (e[1] + EPS) + EPS));
    const size_t row = (size_t)b * T + t;
    partial[row * 2 + 0] = fw;
    partial[row * 2 + 1] = ss;
    if (frames) {
      frames[row * 2 + 0] = fw;
      frames[row * 2 + 1] = ss;
    }
  } else if (lt == 0 && frames && t < T) {
    frames[((size_t)b * T + t) * 2 + 0] = fd_nan();
    frames[((size_t)b * T + t) * 2 + 1] = fd_nan();
  }
}

// out[b] = mean over the clip's frames of fwSSNR_t, of SSNR_t; NaN for a clip without a frame
__global__ __launch_bounds__(256) void segsnr_finalise_kernel(const double* __restrict__ partial, const int* __restrict__ lens, int L, int win, int skip, int T,
                                                              double* __restrict__ out) {
  const int b = blockIdx.x;
  const int Tb = frames_of(lens, b, L, win, skip);
  if (Tb == 0) {                                              // (uniform)
    if (threadIdx.x == 0) out[b * 2 + 0] = out[b * 2 + 1] = fd_nan();
    return;
  }
  const double* __restrict__ p = partial + (size_t)b * T * 2;
  double acc[2] = {0.0, 0.0};
  for (int t = threadIdx.x; t < Tb; t += 256) {
    acc[0] += p[(size_t)t * 2 + 0];
    acc[1] += p[(size_t)t * 2 + 1];
  }
  fd_block_sums<2>(acc);
  if (threadIdx.x == 0) {
    out[b * 2 + 0] = acc[0] / (double)Tb;
    out[b * 2 + 1] = acc[1] / (double)Tb;
  }
}

// ---- host: the tables ---------------------------------------------------------------------------------------------------------------
struct dims { int win, skip, n_fft, log2n; };

// -> false when n_fft falls outside [128, 4096]
bool dims_of(int sr, dims* d) {
  if (sr < 1 || sr > (1 << 24)) return false;
  d->win = (int)nearbyint(0.03 * (double)sr);                 // round half to even, as Python's round
  d->skip = (int)floor(0.25 * (0.03 * (double)sr));
  if (d->win < 1 || d->skip < 1) return false;
  d->log2n = 0;
  while ((1 << d->log2n) < 2 * d->win) ++d->log2n;
  d->n_fft = 1 << d->log2n;
  return d->log2n >= fft_lds::MIN_LOG2N && d->log2n <= fft_lds::MAX_LOG2N;
}

struct banded { int first[NBANDS], count[NBANDS], off[NBANDS]; std::vector<double> w; };

// the critical-band bank of (sr, n_fft) as runs of non-zero taps (flowdec_amd/segsnr.py critical_band_bank is the same arithmetic,
// operation by operation) over the bins 0 .. n_fft / 2 - 1 -> false when a filter is empty there or not one run of bins
bool bank_of(int sr, int n_fft, banded* out) {
  const int h = n_fft / 2;
  const double max_freq = (double)sr / 2.0, min_factor = exp(-30.0 / (2.0 * 2.303));
  out->w.clear();
  std::vector<double> row(h);
  for (int i = 0; i < NBANDS; ++i) {
    const double f0 = floor(CENT[i] / max_freq * (double)h);
    const double bw = BAND[i] / max_freq * (double)h;
    const double norm = log(BAND[0]) - log(BAND[i]);
    int lo = -1, hi = -1, nz = 0;
    for (int j = 0; j < h; ++j) {
      const double q = ((double)j - f0) / bw;
      const double qq = q * q;
      const double m = -11.0 * qq;
      const double v = exp(m + norm);
      row[j] = v > min_factor ? v : 0.0;
      if (row[j] != 0.0) { if (lo < 0) lo = j; hi = j; ++nz; }
    }
    if (nz == 0 || nz != hi - lo + 1) return false;
    out->first[i] = lo; out->count[i] = nz; out->off[i] = (int)out->w.size();
    for (int j = lo; j <= hi; ++j) out->w.push_back(row[j]);
  }
  return true;
}

struct layout { int T; size_t total; };

bool layout_of(const fd_segsnr_plan* p, int B, int L, layout* s) {
  if (!p || B < 1 || B > 65535 || L < 1) return false;
  s->T = L >= p->win + p->skip ? (L - p->win) / p->skip : 0;
  s->total = fd_align(sizeof(double) * (size_t)B * (size_t)(s->T > 0 ? s->T : 1) * 2) + 256;
  return true;
}

}  // namespace

extern "C" int fd_segsnr_tables(int sr, int* dims_out, double* window, float* twiddle, int* first, int* count, double* weights) {
  dims d;
  FD_REQUIRE(dims_of(sr, &d), "fd_segsnr_tables: at %d Hz the transform length 2^ceil(log2(2 round(0.03 sr))) falls outside [128, 4096]", sr);
  banded bd;
  FD_REQUIRE(bank_of(sr, d.n_fft, &bd), "fd_segsnr_tables: a filter of the critical-band bank at %d Hz (n_fft %d) is empty or not one run of bins (the "
             "bands reach 3.8 kHz)", sr, d.n_fft);
  if (dims_out) { dims_out[0] = d.win; dims_out[1] = d.skip; dims_out[2] = d.n_fft; }
  if (!window && !twiddle && !first && !count && !weights) return (int)bd.w.size();
  FD_REQUIRE(window && twiddle && first && count && weights, "fd_segsnr_tables: null pointer");
  for (int n = 0; n < d.win; ++n) window[n] = 0.5 * (1.0 - cos(2.0 * PI * (double)(n + 1) / (double)(d.win + 1)));
  std::vector<float> hann(d.n_fft);                            // (fd_specdist_tables' window: not used here)
  const int rc = fd_specdist_tables(sr, d.n_fft, 0, hann.data(), twiddle, nullptr, nullptr, nullptr);
  if (rc < 0) return rc;
  for (int i = 0; i < NBANDS; ++i) { first[i] = bd.first[i]; count[i] = bd.count[i]; }
  for (size_t i = 0; i < bd.w.size(); ++i) weights[i] = bd.w[i];
  return (int)bd.w.size();
}

extern "C" void fd_segsnr_plan_destroy(fd_segsnr_plan* p) {
  if (!p) return;
  if (p->window) (void)hipFree(p->window);
  if (p->tw) (void)hipFree(p->tw);
  if (p->band) (void)hipFree(p->band);
  if (p->wgt) (void)hipFree(p->wgt);
  delete p;
}

extern "C" int fd_segsnr_plan_create(int sr, fd_segsnr_plan** out) {
  FD_REQUIRE(out, "fd_segsnr_plan_create: null out");
  *out = nullptr;
  int dm[3];
  const int nw = fd_segsnr_tables(sr, dm, nullptr, nullptr, nullptr, nullptr, nullptr);
  if (nw < 0) return nw;
  std::vector<double> window(dm[0]), w(nw);
  std::vector<float> tw(dm[2]);
  std::vector<int> band(3 * NBANDS);
  const int rc = fd_segsnr_tables(sr, nullptr, window.data(), tw.data(), band.data(), band.data() + NBANDS, w.data());
  if (rc < 0) return rc;
  for (int i = 0, o = 0; i < NBANDS; ++i) { band[2 * NBANDS + i] = o; o += band[NBANDS + i]; }
  fd_segsnr_plan* p = new fd_segsnr_plan();
  p->sr = sr; p->win = dm[0]; p->skip = dm[1]; p->log2n = 0;
  while ((1 << p->log2n) < dm[2]) ++p->log2n;
  p->window = nullptr; p->tw = nullptr; p->band = nullptr; p->wgt = nullptr;
  hipError_t e = upload(&p->window, window.data(), window.size());
  if (e == hipSuccess) e = upload(reinterpret_cast<float**>(&p->tw), tw.data(), tw.size());
  if (e == hipSuccess) e = upload(&p->band, band.data(), band.size());
  if (e == hipSuccess) e = upload(&p->wgt, w.data(), w.size());
  if (e != hipSuccess) {
    fd_segsnr_plan_destroy(p);
    return fd_set_error(FD_ERUNTIME, "fd_segsnr_plan_create: uploading the tables failed: %s", hipGetErrorString(e));
  }
  *out = p;
  return FD_OK;
}

extern "C" size_t fd_metrics_segsnr_workspace_bytes(const fd_segsnr_plan* plan, int B, int L) {
  layout s;
  return layout_of(plan, B, L, &s) ? s.total : 0;
}

extern "C" int fd_metrics_segsnr(const fd_segsnr_plan* plan, const float* x_hat, const float* x, const int* lengths, int B, int L, double* out,
                                 double* frames, void* ws, size_t ws_bytes, void* stream) {
  FD_REQUIRE(plan && x_hat && x && lengths && out && ws, "fd_metrics_segsnr: null pointer");
  FD_REQUIRE(B >= 1 && B <= 65535 && L >= 1, "fd_metrics_segsnr: bad batch B %d L %d (1 <= B <= 65535, L >= 1)", B, L);
  layout s;
  layout_of(plan, B, L, &s);
  FD_REQUIRE(ws_bytes >= s.total, "fd_metrics_segsnr: workspace too small (%zu < %zu bytes, fd_metrics_segsnr_workspace_bytes)", ws_bytes, s.total);
  hipStream_t st = fd_stream(stream);
  double* partial = reinterpret_cast<double*>(aligned(ws));
  if (s.T > 0) {
    fft_lds::dispatch(plan->log2n, [&](auto k) {
      using G = fft_lds::Geo<decltype(k)::value>;
      hipLaunchKernelGGL(segsnr_kernel<decltype(k)::value>, dim3(fd_cdiv(s.T, G::FPB), B), dim3(256), 0, st, x_hat, x, lengths, L, plan->win, plan->skip, s.T,
                         plan->window, plan->tw, plan->band, plan->wgt, partial, frames);
    });
  }
  hipLaunchKernelGGL(segsnr_finalise_kernel, dim3(B), dim3(256), 0, st, partial, lengths, L, plan->win, plan->skip, s.T, out);
  FD_LAUNCH_CHECK();
  return FD_OK;
}
