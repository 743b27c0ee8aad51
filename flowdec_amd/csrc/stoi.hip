// stoi.hip -- extended STOI (ESTOI, Jensen & Taal 2016; the reference's eval/metrics.py:273-283 calls pystoi.stoi(extended=True)) of
// ragged batches on the GPU (include/flowdec_hip.h "ESTOI"; host yardstick: flowdec_amd/metrics.py estoi).
//
// The contract of metrics.hip holds: a clip's result has the same BITS alone, in a batch, at any batch position and next to clips of any
// other lengths.  Every partition and every order of summation below is a function of the clip's own length only, every reduction runs
// in a fixed order, and there are no floating-point atomics (no atomics at all).
//
//   resample    fd_resample with the caller's 10 kHz bank, x and x_hat each into a workspace row (skipped without a resample plan)
//   energy      one wave per frame t of x (256 samples at hop 128, frames start below len - 256): sum of (win x)^2 in float64
//   kept        one workgroup per clip: the clip's maximum, then an ordered compaction of the frames within 40 dB of it -> kept[k]
//   bands       one workgroup per 16 spectral frames of one clip, both signals.  Spectral frame t of the (never stored) compacted signal is
//               a gather: n < 128: win[n] x[128 K[t] + n] + win[n + 128] x[128 K[t-1] + 128 + n] (t >= 1), n >= 128: win[n] x[128 K[t] + n]
//               + win[n - 128] x[128 K[t+1] + n - 128]; times win[n] again; formed in float64 and rounded once into LDS.  [16 x 256] .
//               [256 x cos|sin of bins 7..218] on v_mfma_f32_16x16x4_f32 (an f32 fma chain in ascending k), re^2 + im^2 in float32, the
//               15 band sums in float64 in ascending bin order, sqrt, float32 -> tob[b][signal][t][15]
//   segments    one workgroup per run of 16 segments of one clip, a wave per segment: row statistics on lanes 0..29 (signal, band), the
//               column normalisation and the column's dot product on lanes 0..29 (frame), all float64, then a wave sum
//   final       the clip's segment sums, lane-strided then a wave sum, / 30 / J; 1e-5 below 30 spectral frames
#include <math.h>

#include <vector>

#include "internal.h"
#include "measure_common.h"

struct fd_estoi_plan {
  double* win;     // device [256]: np.hanning(258)[1:-1]
  float* table;    // device [256][TAB_COLS]: group g of 16 bins = 16 cos columns then 16 sin columns
};

namespace {

constexpr int FRAME = 256, HOP = 128, NFFT = 512, NBANDS = 15, NSEG = 30;
constexpr int BIN0 = 7, NBINS = 212;                     // the bins the 15 bands read: [7, 219)
constexpr int GROUPS = (NBINS + 15) / 16;                // 14 groups of 16 bins, the last 12 columns zero
constexpr int TAB_COLS = GROUPS * 32, PW_COLS = GROUPS * 16;
constexpr int TILE_T = 16;                               // spectral frames per bands workgroup
constexpr int SEG_RUN = 16;                              // segments per segment workgroup
constexpr double EPS = 2.220446049250313e-16;            // np.finfo(float).eps
constexpr double TOO_SHORT = 1e-5;
constexpr long long LEN_CAP = 1LL << 30;                 // samples of a 10 kHz row

__constant__ int BAND_EDGE[NBANDS + 1] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};

__host__ __device__ inline long long out_length(long long L, int o, int n) { return (L / o) * n + ((L % o) * n + o - 1) / o; }

// frames of range(0, len - 256, 128): the frame that would end exactly at len is not taken
__host__ __device__ inline int frames_of(long long len) { return len > FRAME ? (int)((len - FRAME + HOP - 1) / HOP) : 0; }

// the clip's own length at 10 kHz (o == 0: the rows are at 10 kHz already); the length is clamped into its row
__device__ __forceinline__ int clip_len10(const int* __restrict__ lens, int b, int L, int o, int n) {
  const int c = fd_clip_len(lens, b, L);
  return o > 0 ? (int)out_length(c, o, n) : c;
}

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_down(v, o, 64));
  return v;
}

// energy[b][t] = sum over the frame of (win[n] x[128 t + n])^2, float64: lane l takes n = l, l + 64, l + 128, l + 192, then the wave tree
__global__ __launch_bounds__(256) void estoi_energy_kernel(const float* __restrict__ x, long long stride, const int* __restrict__ lens, int L, int o, int n,
                                                           const double* __restrict__ win, int Tmax, double* __restrict__ energy) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= frames_of(clip_len10(lens, b, L, o, n))) return;        // (wave-uniform)
  const float* __restrict__ p = x + (long long)b * stride + (long long)t * HOP;
  double acc = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const double v = win[lane + 64 * i] * (double)p[lane + 64 * i];
    acc += v * v;
  }
  acc = fd_wave_sum(acc);
  if (lane == 0) energy[(size_t)b * Tmax + t] = acc;
}

// kept[b][0..k) = the frames with (||.|| + EPS) > (max ||.|| + EPS) 10^-2 in ascending order, -1 behind them; frames[b] = frames, kept,
// spectral frames (kept - 1)
__global__ __launch_bounds__(256) void estoi_kept_kernel(const double* __restrict__ energy, const int* __restrict__ lens, int L, int o, int n, int Tmax,
                                                         int* __restrict__ kept, int* __restrict__ frames) {
  __shared__ double smax[4];
  __shared__ int scount[4];
  __shared__ int sbase;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int F = frames_of(clip_len10(lens, b, L, o, n));
  const double* __restrict__ e = energy + (size_t)b * Tmax;
  int* __restrict__ kp = kept + (size_t)b * Tmax;
  double m = 0.0;
  for (int t = tid; t < F; t += 256) m = fmax(m, e[t]);
  m = wave_max(m);
  if (lane == 0) smax[wv] = m;
  if (tid == 0) sbase = 0;
  __syncthreads();
  const double thr = (sqrt(fmax(fmax(smax[0], smax[1]), fmax(smax[2], smax[3]))) + EPS) * 1e-2;
  for (int t0 = 0; t0 < F; t0 += 256) {
    const int t = t0 + tid;
    const bool keep = t < F && (sqrt(e[t]) + EPS) > thr;
    const unsigned long long bal = __ballot(keep);
    const int pre = __popcll(bal & ((1ULL << lane) - 1ULL));
    if (lane == 0) scount[wv] = __popcll(bal);
    __syncthreads();
    int base = sbase;
    for (int w = 0; w < wv; ++w) base += scount[w];
    if (keep) kp[base + pre] = t;
    __syncthreads();
    if (tid == 0) sbase += scount[0] + scount[1] + scount[2] + scount[3];
    __syncthreads();
  }
  const int k = sbase;
  for (int t = k + tid; t < Tmax; t += 256) kp[t] = -1;
  if (tid == 0) {
    frames[b * 3 + 0] = F;
    frames[b * 3 + 1] = k;
    frames[b * 3 + 2] = k > 0 ? k - 1 : 0;
  }
}

// LDS image of a [16][256] f32 tile: the column XOR-swizzled by the row, so that the 16 rows x 4 columns of one 16x16x4 A operand hit
// distinct banks (attn.hip's layout)
__device__ __forceinline__ int swz(int row, int c) { return row * FRAME + (c ^ ((row & 15) * 4)); }

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// tob[b][s][t][15] for the spectral frames [16 j, 16 j + 16) of clip b; s = 0: x, 1: x_hat; zero at t >= the clip's own count
__global__ __launch_bounds__(256) void estoi_bands_kernel(const float* __restrict__ x, const float* __restrict__ xh, long long stride,
                                                          const int* __restrict__ kept, const int* __restrict__ frames, const double* __restrict__ win,
                                                          const float* __restrict__ table, int Tmax, float* __restrict__ tob) {
  __shared__ __attribute__((aligned(16))) float buf[2 * TILE_T * FRAME];      // the frames, then re^2 + im^2 [2][16][PW_COLS]
  __shared__ int ks[TILE_T + 2];                                               // K[t0 - 1 .. t0 + 16]
  const int b = blockIdx.y, t0 = blockIdx.x * TILE_T, tid = threadIdx.x;
  const int T = frames[b * 3 + 2];
  float* __restrict__ out = tob + (size_t)b * 2 * Tmax * NBANDS;
  if (t0 >= T) {
    for (int i = tid; i < 2 * TILE_T * NBANDS; i += 256) {
      const int s = i / (TILE_T * NBANDS), r = i % (TILE_T * NBANDS);
      if (t0 + r / NBANDS < Tmax) out[((size_t)s * Tmax + t0) * NBANDS + r] = 0.f;
    }
    return;
  }
  if (tid < TILE_T + 2) {
    const int t = t0 - 1 + tid;
    ks[tid] = (t >= 0 && t <= T) ? kept[(size_t)b * Tmax + t] : 0;             // (T = kept - 1: K[T] exists)
  }
  __syncthreads();
  for (int i = tid; i < 2 * TILE_T * FRAME; i += 256) {
    const int s = i / (TILE_T * FRAME), f = (i / FRAME) % TILE_T, n = i % FRAME;
    const int t = t0 + f;
    float v = 0.f;
    if (t < T) {
      const float* __restrict__ p = (s == 0 ? x : xh) + (long long)b * stride;
      double a = win[n] * (double)p[(long long)HOP * ks[f + 1] + n];
      if (n >= HOP) a += win[n - HOP] * (double)p[(long long)HOP * ks[f + 2] + n - HOP];
      else if (t >= 1) a += win[n + HOP] * (double)p[(long long)HOP * ks[f] + HOP + n];
      v = (float)(a * win[n]);
    }
    buf[s * TILE_T * FRAME + swz(f, n)] = v;
  }
  __syncthreads();

  const int lane = tid & 63, wv = tid >> 6, li = lane & 15, lk = lane >> 4;
  f32x4 acc[2][4][2];     // [signal][group wv + 4 u][cos | sin]: 64 accumulator registers
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[s][u][0] = acc[s][u][1] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int step = 0; step < FRAME / 4; ++step) {
    const int k = 4 * step + lk;
    const float a0 = buf[swz(li, k)], a1 = buf[TILE_T * FRAME + swz(li, k)];
    const float* __restrict__ brow = table + (size_t)k * TAB_COLS + li;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int g = wv + 4 * u;
      if (g < GROUPS) {                                                         // (wave-uniform)
        const float bc = brow[32 * g], bs = brow[32 * g + 16];
        acc[0][u][0] = mfma4(a0, bc, acc[0][u][0]);
        acc[0][u][1] = mfma4(a0, bs, acc[0][u][1]);
        acc[1][u][0] = mfma4(a1, bc, acc[1][u][0]);
        acc[1][u][1] = mfma4(a1, bs, acc[1][u][1]);
      }
    }
  }
  __syncthreads();        // every wave has read its last A operand: the buffer now takes the powers
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int g = wv + 4 * u;
      if (g < GROUPS) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float re = acc[s][u][0][r], im = acc[s][u][1][r];
          buf[(s * TILE_T + 4 * lk + r) * PW_COLS + 16 * g + li] = re * re + im * im;
        }
      }
    }
  __syncthreads();
  for (int i = tid; i < 2 * TILE_T * NBANDS; i += 256) {
    const int s = i / (TILE_T * NBANDS), r = i % (TILE_T * NBANDS), f = r / NBANDS, band = r % NBANDS;
    if (t0 + f >= Tmax) continue;
    float v = 0.f;
    if (t0 + f < T) {
      const float* __restrict__ pw = buf + (s * TILE_T + f) * PW_COLS;
      double sum = 0.0;
      for (int c = BAND_EDGE[band] - BIN0; c < BAND_EDGE[band + 1] - BIN0; ++c) sum += (double)pw[c];
      v = (float)sqrt(sum);
    }
    out[((size_t)s * Tmax + t0) * NBANDS + r] = v;
  }
}

// seg[b][m] = sum over the 15 x 30 block of frames [m, m + 30) of x_n y_n after the row and the column normalisation (float64)
__global__ __launch_bounds__(256) void estoi_segment_kernel(const float* __restrict__ tob, const int* __restrict__ frames, int Tmax, double* __restrict__ seg) {
  __shared__ float tile[2][(SEG_RUN + NSEG - 1) * NBANDS];
  const int b = blockIdx.y, j0 = blockIdx.x * SEG_RUN, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int T = frames[b * 3 + 2];
  const int J = T >= NSEG ? T - NSEG + 1 : 0;
  if (j0 >= J) return;
  const int nseg = J - j0 < SEG_RUN ? J - j0 : SEG_RUN, nel = (nseg + NSEG - 1) * NBANDS;
  for (int i = tid; i < 2 * nel; i += 256) {
    const int s = i / nel, r = i % nel;
    tile[s][r] = tob[(((size_t)b * 2 + s) * Tmax + j0) * NBANDS + r];
  }
  __syncthreads();
  for (int j = wv; j < nseg; j += 4) {                                          // (wave-uniform)
    // rows: lane = signal * 15 + band: mean over the 30 frames, 2-norm of the centred row
    double mean = 0.0, nrm = 0.0;
    if (lane < 2 * NBANDS) {
      const float* __restrict__ p = &tile[lane / NBANDS][j * NBANDS + lane % NBANDS];
      double sum = 0.0;
      for (int f = 0; f < NSEG; ++f) sum += (double)p[f * NBANDS];
      mean = sum / NSEG;
      double ss = 0.0;
      for (int f = 0; f < NSEG; ++f) {
        const double d = (double)p[f * NBANDS] - mean;
        ss += d * d;
      }
      nrm = sqrt(ss);
    }
    // columns: lane = frame.  A row or column whose sum of squares is exactly 0 normalises to zeros.
    const int c = lane < NSEG ? lane : NSEG - 1;
    double vx[NBANDS], vy[NBANDS], sx = 0.0, sy = 0.0;
#pragma unroll
    for (int k = 0; k < NBANDS; ++k) {
      const double mx = __shfl(mean, k, 64), nx = __shfl(nrm, k, 64), my = __shfl(mean, NBANDS + k, 64), ny = __shfl(nrm, NBANDS + k, 64);
      vx[k] = nx > 0.0 ? ((double)tile[0][(j + c) * NBANDS + k] - mx) / nx : 0.0;
      vy[k] = ny > 0.0 ? ((double)tile[1][(j + c) * NBANDS + k] - my) / ny : 0.0;
      sx += vx[k];
      sy += vy[k];
    }
    const double cmx = sx / NBANDS, cmy = sy / NBANDS;
    double ssx = 0.0, ssy = 0.0;
#pragma unroll
    for (int k = 0; k < NBANDS; ++k) {
      vx[k] -= cmx;
      vy[k] -= cmy;
      ssx += vx[k] * vx[k];
      ssy += vy[k] * vy[k];
    }
    const double cnx = sqrt(ssx), cny = sqrt(ssy);
    double dot = 0.0;
    if (lane < NSEG && cnx > 0.0 && cny > 0.0) {
#pragma unroll
      for (int k = 0; k < NBANDS; ++k) dot += (vx[k] / cnx) * (vy[k] / cny);
    }
    dot = fd_wave_sum(dot);
    if (lane == 0) seg[(size_t)b * Tmax + j0 + j] = dot;
  }
}

__global__ __launch_bounds__(64) void estoi_final_kernel(const double* __restrict__ seg, const int* __restrict__ frames, int Tmax, double* __restrict__ out) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int T = frames[b * 3 + 2];
  if (T < NSEG) {
    if (lane == 0) out[b] = TOO_SHORT;
    return;
  }
  const int J = T - NSEG + 1;
  double a = 0.0;
  for (int j = lane; j < J; j += 64) a += seg[(size_t)b * Tmax + j];
  a = fd_wave_sum(a);
  if (lane == 0) out[b] = a / NSEG / (double)J;
}

struct estoi_layout { long long L10; int Tmax; size_t rows, energy, kept, tob, seg, total; };

// o == n: the rows are at 10 kHz already (no resampled copy)
bool layout_of(int B, int L, int o, int n, estoi_layout* s) {
  if (B < 1 || B > 65535 || L < 1 || o < 1 || n < 1) return false;
  s->L10 = o == n ? L : out_length(L, o, n);
  if (s->L10 > LEN_CAP) return false;
  s->Tmax = std::max(frames_of(s->L10), 1);
  s->rows = o == n ? 0 : fd_align(sizeof(float) * (size_t)B * s->L10);
  s->energy = fd_align(sizeof(double) * (size_t)B * s->Tmax);
  s->kept = fd_align(sizeof(int) * (size_t)B * s->Tmax);
  s->tob = fd_align(sizeof(float) * (size_t)B * 2 * s->Tmax * NBANDS);
  s->seg = fd_align(sizeof(double) * (size_t)B * s->Tmax);
  s->total = 2 * s->rows + s->energy + s->kept + s->tob + s->seg + 256;
  return true;
}

// the whole chain; kept_out / tob_out: the caller's buffers of the stage call, or null (workspace)
int run(const char* who, const fd_estoi_plan* plan, const fd_resample_plan* rs, const float* x_hat, const float* x, const int* lengths, int B, int L,
        double* estoi_out, int* frames_out, int* kept_out, float* tob_out, void* ws, size_t ws_bytes, void* stream) {
  FD_REQUIRE(B >= 1 && B <= 65535 && L >= 1, "%s: bad batch B %d L %d (1 <= B <= 65535, L >= 1)", who, B, L);
  int o = 1, n = 1;
  if (rs) fd_resample_plan_dims(rs, &o, &n, nullptr, nullptr);
  estoi_layout s;
  FD_REQUIRE(layout_of(B, L, o, n, &s), "%s: rows of %d samples resampled %d -> %d are beyond 2^30 samples", who, L, o, n);
  FD_REQUIRE(ws_bytes >= s.total, "%s: workspace too small (%zu < %zu bytes, fd_metrics_estoi_workspace_bytes)", who, ws_bytes, s.total);
  hipStream_t st = fd_stream(stream);
  char* base = aligned(ws);
  const float* x10 = x;
  const float* xh10 = x_hat;
  const bool resampled = o != n;
  if (resampled) {
    float* r0 = reinterpret_cast<float*>(base);
    float* r1 = reinterpret_cast<float*>(base + s.rows);
    FD_TRY(fd_resample(rs, x, lengths, B, L, r0, s.L10, stream));
    FD_TRY(fd_resample(rs, x_hat, lengths, B, L, r1, s.L10, stream));
    x10 = r0;
    xh10 = r1;
  }
  base += 2 * s.rows;
  double* energy = reinterpret_cast<double*>(base);
  int* kept = kept_out ? kept_out : reinterpret_cast<int*>(base + s.energy);
  float* tob = tob_out ? tob_out : reinterpret_cast<float*>(base + s.energy + s.kept);
  double* seg = reinterpret_cast<double*>(base + s.energy + s.kept + s.tob);
  const int ko = resampled ? o : 0, Tmax = s.Tmax;
  hipLaunchKernelGGL(estoi_energy_kernel, dim3(fd_cdiv(Tmax, 4), B), dim3(256), 0, st, x10, s.L10, lengths, L, ko, n, plan->win, Tmax, energy);
  hipLaunchKernelGGL(estoi_kept_kernel, dim3(B), dim3(256), 0, st, energy, lengths, L, ko, n, Tmax, kept, frames_out);
  hipLaunchKernelGGL(estoi_bands_kernel, dim3(fd_cdiv(Tmax, TILE_T), B), dim3(256), 0, st, x10, xh10, s.L10, kept, frames_out, plan->win, plan->table, Tmax,
                     tob);
  if (estoi_out) {
    hipLaunchKernelGGL(estoi_segment_kernel, dim3(fd_cdiv(Tmax, SEG_RUN), B), dim3(256), 0, st, tob, frames_out, Tmax, seg);
    hipLaunchKernelGGL(estoi_final_kernel, dim3(B), dim3(64), 0, st, seg, frames_out, Tmax, estoi_out);
  }
  FD_LAUNCH_CHECK();
  return FD_OK;
}

}  // namespace

extern "C" int fd_estoi_plan_create(fd_estoi_plan** out) {
  FD_REQUIRE(out, "fd_estoi_plan_create: null out");
  *out = nullptr;
  const double pi = 3.14159265358979323846;
  std::vector<double> win(FRAME);
  for (int i = 0; i < FRAME; ++i) win[i] = 0.5 - 0.5 * cos(2.0 * pi * (i + 1) / (FRAME + 1));      // np.hanning(258)[1:-1]
  std::vector<float> tab((size_t)FRAME * TAB_COLS, 0.f);
  for (int k = 0; k < FRAME; ++k)
    for (int c = 0; c < NBINS; ++c) {
      const double ph = 2.0 * pi * (double)(((BIN0 + c) * k) % NFFT) / NFFT;
      tab[(size_t)k * TAB_COLS + 32 * (c / 16) + c % 16] = (float)cos(ph);
      tab[(size_t)k * TAB_COLS + 32 * (c / 16) + 16 + c % 16] = (float)sin(ph);
    }
  fd_estoi_plan* p = new fd_estoi_plan();
  p->win = nullptr; p->table = nullptr;
  hipError_t e = hipMalloc(&p->win, sizeof(double) * win.size());
  if (e == hipSuccess) e = hipMalloc(&p->table, sizeof(float) * tab.size());
  if (e == hipSuccess) e = hipMemcpy(p->win, win.data(), sizeof(double) * win.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(p->table, tab.data(), sizeof(float) * tab.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    if (p->win) (void)hipFree(p->win);
    if (p->table) (void)hipFree(p->table);
    delete p;
    return fd_set_error(FD_ERUNTIME, "fd_estoi_plan_create: uploading the tables failed: %s", hipGetErrorString(e));
  }
  *out = p;
  return FD_OK;
}

extern "C" void fd_estoi_plan_destroy(fd_estoi_plan* p) {
  if (!p) return;
  (void)hipFree(p->win);
  (void)hipFree(p->table);
  delete p;
}

extern "C" size_t fd_metrics_estoi_workspace_bytes(int B, int L, int o, int n) {
  estoi_layout s;
  return layout_of(B, L, o, n, &s) ? s.total : 0;
}

extern "C" int fd_metrics_estoi_max_frames(int L, int o, int n) {
  estoi_layout s;
  return layout_of(1, L, o, n, &s) ? s.Tmax : 0;
}

extern "C" int fd_metrics_estoi(const fd_estoi_plan* plan, const fd_resample_plan* resample, const float* x_hat, const float* x, const int* lengths, int B,
                                int L, double* estoi_out, int* frames_out, void* ws, size_t ws_bytes, void* stream) {
  FD_REQUIRE(plan && x_hat && x && lengths && estoi_out && frames_out && ws, "fd_metrics_estoi: null pointer");
  return run("fd_metrics_estoi", plan, resample, x_hat, x, lengths, B, L, estoi_out, frames_out, nullptr, nullptr, ws, ws_bytes, stream);
}

extern "C" int fd_metrics_estoi_bands(const fd_estoi_plan* plan, const fd_resample_plan* resample, const float* x_hat, const float* x, const int* lengths,
                                      int B, int L, int* frames_out, int* kept_out, float* tob_out, void* ws, size_t ws_bytes, void* stream) {
  FD_REQUIRE(plan && x_hat && x && lengths && frames_out && kept_out && tob_out && ws, "fd_metrics_estoi_bands: null pointer");
  return run("fd_metrics_estoi_bands", plan, resample, x_hat, x, lengths, B, L, nullptr, frames_out, kept_out, tob_out, ws, ws_bytes, stream);
}
