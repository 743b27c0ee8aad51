// loss.hip -- the kernels behind the validation loss (include/flowdec_hip.h "Validation loss"): what the reference's `_loss` does around
// its one network evaluation (flowdec/model.py:421-468 flow, :590-611 score, :552-559 regression), without gradients.
//
// loss_times_kernel   t[b] = lo + u[b] (hi - lo), u[b] = (r0 >> 8) 2^-24 from Philox4x32-10 keyed by the clip's seed at counter (0, 0, 0, 1)
//                     -- value 1 of the counter word the noise contract reserves, so a clip's time never collides with its noise.
// loss_state_kernel   (Y, X, t) -> the network input Xt and the regression target in ONE pass over the planes; the Gaussian draws are read
//                     from planes or generated in registers from the clip's seed (noise.h).  Every product and sum is rounded on its own
//                     (no contraction), as the reference's tensor expressions round them.
// loss_sqerr_kernel / loss_sqerr_finish_kernel
//                     per-clip sum of |err|^2 in float64 and a count of non-finite err elements.  Stage 1: workgroup j of a clip owns the
//                     elements [j SQ_CHUNK, (j + 1) SQ_CHUNK); thread k adds elements k, k + 256, ... in that order, the 256 thread sums
//                     are added by a fixed LDS tree.  Stage 2: one workgroup per clip adds the partials the same way.  The order depends on
//                     F T_pad only, there is no floating-point atomic, and a clip's bits do not depend on the batch.
#include "internal.h"
#include "measure_common.h"
#include "noise.h"

namespace {

constexpr int SQ_CHUNK = 4096;   // complex elements per stage-1 workgroup: 16 per thread

// ---- times ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void loss_times_kernel(const unsigned long long* __restrict__ seeds, int B, float lo, float hi, float* __restrict__ t_out) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const unsigned long long s = seeds[b];
  unsigned r[4];
  philox4x32_10(0u, 0u, 0u, 1u, (unsigned)s, (unsigned)(s >> 32), r);
  const float u = (float)(r[0] >> 8) * 5.9604644775390625e-08f;   // 2^-24: in [0, 1), exact
  const float span = hi - lo;
  t_out[b] = u * span + lo;                                        // torch.rand(B) * (T - t_eps) + t_eps
}

// ---- state ------------------------------------------------------------------------------------------------------------------------------
struct state_args {
  const float2 *Y, *X;
  const float* t;
  const float2* noise;                 // [n_draws][B][F][T] (not SEEDED)
  const unsigned long long* seeds;     // [B] (SEEDED)
  const double* sigma;                 // flow: sigma_y, [sigma_n]
  int sigma_n;
  float sigma_x;
  float theta, sigma_min, logsig;      // score: OUVE closed forms (sdes.py:178-196)
  float2 *xt, *target, *ys;
  float* std_out;
  long long plane;                     // B F T: elements between two draws of `noise`
  int F, T;
};

template <bool SEEDED>
__device__ __forceinline__ float2 loss_draw(const state_args& a, int draw, int b, int f, int tt, long long idx) {
  if constexpr (SEEDED) return fd_noise_at(a.seeds[b], draw, f, tt);
  else return a.noise[(long long)draw * a.plane + idx];
}

// grid (blocks per clip, B): the clip and with it t[b] and every coefficient are uniform over a workgroup
template <int KIND, bool SEEDED>
__global__ __launch_bounds__(256) void loss_state_kernel(const state_args a) {
#pragma clang fp contract(off)
  const int b = blockIdx.y;
  const int n = a.F * a.T;
  const long long base = (long long)b * n;
  float tb = 0.f, omt = 1.f, ex = 0.f, ome = 0.f, sd = 0.f;
  if constexpr (KIND == FD_LOSS_FLOW) {
    tb = a.t[b];
    omt = 1.0f - tb;
  } else if constexpr (KIND == FD_LOSS_SCORE) {
    tb = a.t[b];
    ex = expf(-a.theta * tb);
    ome = 1.0f - ex;
    const float num = a.sigma_min * a.sigma_min * expf(-2.f * a.theta * tb) * (expf(2.f * (a.theta + a.logsig) * tb) - 1.f) * a.logsig;
    sd = sqrtf(num / (a.theta + a.logsig));
    if (blockIdx.x == 0 && threadIdx.x == 0 && a.std_out) a.std_out[b] = sd;
  }
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const long long idx = base + i;
    const int f = i / a.T, tt = i - f * a.T;
    const float2 yv = a.Y[idx], xv = a.X[idx];
    if constexpr (KIND == FD_LOSS_FLOW) {
      // Ys = Y + (sigma_y z0).type(complex64): init_state_kernel's arithmetic with sigma_fac = 1
      const double s = a.sigma[a.sigma_n == 1 ? 0 : f];
      const float2 z0 = loss_draw<SEEDED>(a, 0, b, f, tt, idx);
      const float2 ys = {yv.x + (float)(s * (double)z0.x), yv.y + (float)(s * (double)z0.y)};
      float2 xs = xv;
      if (a.sigma_x != 0.f) {
        const float2 z1 = loss_draw<SEEDED>(a, 1, b, f, tt, idx);
        xs.x = xv.x + a.sigma_x * z1.x;
        xs.y = xv.y + a.sigma_x * z1.y;
      }
      a.xt[idx] = float2{tb * xs.x + omt * ys.x, tb * xs.y + omt * ys.y};
      a.target[idx] = float2{xs.x - ys.x, xs.y - ys.y};
      if (a.ys) a.ys[idx] = ys;
    } else if constexpr (KIND == FD_LOSS_SCORE) {
      const float2 z0 = loss_draw<SEEDED>(a, 0, b, f, tt, idx);
      const float mx = ex * xv.x + ome * yv.x, my = ex * xv.y + ome * yv.y;
      a.xt[idx] = float2{mx + z0.x * sd, my + z0.y * sd};
      a.target[idx] = z0;
    } else {
      a.xt[idx] = yv;
      a.target[idx] = xv;
    }
  }
}

// ---- squared error ----------------------------------------------------------------------------------------------------------------------
// the sum of the 256 values of a workgroup in a fixed order: halving tree over LDS
__device__ __forceinline__ double block_sum_fixed(double v, double* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}
__device__ __forceinline__ long long block_sum_fixed(long long v, long long* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  const long long r = sh[0];
  __syncthreads();
  return r;
}

__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// grid (ceil(n / SQ_CHUNK), B): psum / pbad [B][gridDim.x]
template <int KIND>
__global__ __launch_bounds__(256) void loss_sqerr_kernel(const float2* __restrict__ V, const float2* __restrict__ target, const float* __restrict__ stdv, int n,
                                                         double* __restrict__ psum, long long* __restrict__ pbad) {
#pragma clang fp contract(off)
  __shared__ double shd[256];
  __shared__ long long shl[256];
  const int b = blockIdx.y;
  const long long base = (long long)b * n;
  const int i0 = blockIdx.x * SQ_CHUNK;
  const int i1 = i0 + SQ_CHUNK < n ? i0 + SQ_CHUNK : n;
  float sd = 1.f;
  if constexpr (KIND == FD_LOSS_SCORE) sd = stdv[b];
  double acc = 0.0;
  long long bad = 0;
  for (int i = i0 + (int)threadIdx.x; i < i1; i += 256) {
    const float2 v = V[base + i], u = target[base + i];
    float er, ei;
    if constexpr (KIND == FD_LOSS_SCORE) {     // std * ((-V / std) - (-z / std)), model.py:601-606, :627
      er = sd * ((-v.x / sd) - (-u.x / sd));
      ei = sd * ((-v.y / sd) - (-u.y / sd));
    } else {
      er = v.x - u.x;
      ei = v.y - u.y;
    }
    acc += (double)er * (double)er + (double)ei * (double)ei;
    bad += (finite_f(er) && finite_f(ei)) ? 0 : 1;
  }
  const double s = block_sum_fixed(acc, shd);
  const long long c = block_sum_fixed(bad, shl);
  if (threadIdx.x == 0) {
    psum[(size_t)b * gridDim.x + blockIdx.x] = s;
    pbad[(size_t)b * gridDim.x + blockIdx.x] = c;
  }
}

// grid B: sums[b] = the clip's nb partials, thread k adding k, k + 256, ... first
__global__ __launch_bounds__(256) void loss_sqerr_finish_kernel(const double* __restrict__ psum, const long long* __restrict__ pbad, int nb,
                                                                double* __restrict__ sums, long long* __restrict__ bad_out) {
  __shared__ double shd[256];
  __shared__ long long shl[256];
  const int b = blockIdx.x;
  double acc = 0.0;
  long long bad = 0;
  for (int j = threadIdx.x; j < nb; j += 256) {
    acc += psum[(size_t)b * nb + j];
    bad += pbad[(size_t)b * nb + j];
  }
  const double s = block_sum_fixed(acc, shd);
  const long long c = block_sum_fixed(bad, shl);
  if (threadIdx.x == 0) {
    sums[b] = s;
    bad_out[b] = c;
  }
}

inline bool plane_ok(int B, int F, int T) { return B >= 1 && B <= 65535 && F >= 1 && T >= 1 && (long long)F * T <= (1LL << 30); }
inline int sq_blocks(int F, int T) { return fd_cdiv((long long)F * T, SQ_CHUNK); }
inline size_t sq_part_bytes(int B, int F, int T) { return fd_align(8 * (size_t)B * sq_blocks(F, T)); }
template <int KIND>
void launch_state(const state_args& a, bool seeded, int B, hipStream_t st) {
  const int n = a.F * a.T;
  int gx = fd_cdiv(n, 256 * 4);
  if (gx > 1024) gx = 1024;
  if (seeded) hipLaunchKernelGGL((loss_state_kernel<KIND, true>), dim3(gx, B), dim3(256), 0, st, a);
  else hipLaunchKernelGGL((loss_state_kernel<KIND, false>), dim3(gx, B), dim3(256), 0, st, a);
}

}  // namespace

extern "C" int fd_loss_num_draws(const fd_loss_config* cfg) {
  if (!cfg) return -1;
  switch (cfg->kind) {
    case FD_LOSS_FLOW: return cfg->sigma_x != 0.f ? 2 : 1;
    case FD_LOSS_SCORE: return 1;
    case FD_LOSS_REGRESSION: return 0;
  }
  return -1;
}

extern "C" int fd_loss_times(const unsigned long long* seeds, int B, float lo, float hi, float* t_out, void* stream) {
  FD_REQUIRE(seeds, "fd_loss_times: null seeds");
  FD_REQUIRE(t_out, "fd_loss_times: null t_out");
  FD_REQUIRE(B >= 1, "fd_loss_times: B = %d (at least one clip)", B);
  FD_REQUIRE(lo >= 0.f && hi > lo && hi <= 1.f, "fd_loss_times: bad range [%g, %g) (0 <= lo < hi <= 1)", (double)lo, (double)hi);
  hipLaunchKernelGGL(loss_times_kernel, dim3(fd_cdiv(B, 256)), dim3(256), 0, fd_stream(stream), seeds, B, lo, hi, t_out);
  FD_LAUNCH_CHECK();
  return FD_OK;
}

extern "C" int fd_loss_state(const fd_loss_config* cfg, const float* Y, const float* X, const float* t, const float* noise, const unsigned long long* seeds,
                             const double* sigma_y, int sigma_n, float* xt_out, float* target_out, float* std_out, float* ys_out, int B, int F, int T_pad,
                             void* stream) {
  FD_REQUIRE(cfg, "fd_loss_state: null cfg");
  FD_REQUIRE(Y, "fd_loss_state: null Y");
  FD_REQUIRE(X, "fd_loss_state: null X");
  FD_REQUIRE(xt_out, "fd_loss_state: null xt_out");
  FD_REQUIRE(target_out, "fd_loss_state: null target_out");
  const int draws = fd_loss_num_draws(cfg);
  FD_REQUIRE(draws >= 0, "fd_loss_state: unknown kind %d (FD_LOSS_FLOW, FD_LOSS_SCORE or FD_LOSS_REGRESSION)", cfg->kind);
  FD_REQUIRE(plane_ok(B, F, T_pad), "fd_loss_state: bad shape B %d F %d T_pad %d (1 <= B <= 65535, F T_pad <= 2^30)", B, F, T_pad);
  if (draws > 0) {
    FD_REQUIRE(t, "fd_loss_state: null t");
    FD_REQUIRE((noise != nullptr) != (seeds != nullptr), "fd_loss_state: exactly one of noise and seeds must be given (got %s)", noise ? "both" : "neither");
  }
  state_args a = {};
  a.Y = (const float2*)Y; a.X = (const float2*)X; a.t = t; a.noise = (const float2*)noise; a.seeds = seeds;
  a.xt = (float2*)xt_out; a.target = (float2*)target_out; a.ys = (float2*)ys_out; a.std_out = std_out;
  a.plane = (long long)B * F * T_pad; a.F = F; a.T = T_pad;
  hipStream_t st = fd_stream(stream);
  if (cfg->kind == FD_LOSS_FLOW) {
    FD_REQUIRE(sigma_y, "fd_loss_state: null sigma_y");
    FD_REQUIRE(sigma_n == 1 || sigma_n == F, "fd_loss_state: sigma_y has %d entries (1 or F = %d)", sigma_n, F);
    FD_REQUIRE(cfg->sigma_x >= 0.f, "fd_loss_state: sigma_x must not be negative");
    a.sigma = sigma_y; a.sigma_n = sigma_n; a.sigma_x = cfg->sigma_x;
    launch_state<FD_LOSS_FLOW>(a, seeds != nullptr, B, st);
  } else if (cfg->kind == FD_LOSS_SCORE) {
    FD_REQUIRE(cfg->sigma_min > 0.f && cfg->sigma_max > cfg->sigma_min && cfg->theta > 0.f, "fd_loss_state: bad OUVE parameters");
    a.theta = cfg->theta; a.sigma_min = cfg->sigma_min; a.logsig = logf(cfg->sigma_max / cfg->sigma_min);
    launch_state<FD_LOSS_SCORE>(a, seeds != nullptr, B, st);
  } else {
    launch_state<FD_LOSS_REGRESSION>(a, false, B, st);
  }
  FD_LAUNCH_CHECK();
  return FD_OK;
}

extern "C" size_t fd_loss_sqerr_workspace_bytes(int B, int F, int T_pad) {
  if (!plane_ok(B, F, T_pad)) return 0;
  return 2 * sq_part_bytes(B, F, T_pad) + 256;
}

extern "C" int fd_loss_sqerr(int kind, const float* V, const float* target, const float* std, double* sums_out, long long* bad_out, int B, int F, int T_pad,
                             void* ws, size_t ws_bytes, void* stream) {
  FD_REQUIRE(V, "fd_loss_sqerr: null V");
  FD_REQUIRE(target, "fd_loss_sqerr: null target");
  FD_REQUIRE(sums_out, "fd_loss_sqerr: null sums_out");
  FD_REQUIRE(bad_out, "fd_loss_sqerr: null bad_out");
  FD_REQUIRE(ws, "fd_loss_sqerr: null ws");
  FD_REQUIRE(kind == FD_LOSS_FLOW || kind == FD_LOSS_SCORE || kind == FD_LOSS_REGRESSION, "fd_loss_sqerr: unknown kind %d", kind);
  FD_REQUIRE(kind != FD_LOSS_SCORE || std, "fd_loss_sqerr: null std (score mode)");
  FD_REQUIRE(plane_ok(B, F, T_pad), "fd_loss_sqerr: bad shape B %d F %d T_pad %d (1 <= B <= 65535, F T_pad <= 2^30)", B, F, T_pad);
  const size_t need = fd_loss_sqerr_workspace_bytes(B, F, T_pad);
  FD_REQUIRE(ws_bytes >= need, "fd_loss_sqerr: workspace too small (%zu < %zu bytes, fd_loss_sqerr_workspace_bytes)", ws_bytes, need);
  hipStream_t st = fd_stream(stream);
  char* base = aligned(ws);
  double* psum = reinterpret_cast<double*>(base);
  long long* pbad = reinterpret_cast<long long*>(base + sq_part_bytes(B, F, T_pad));
  const int n = F * T_pad, nb = sq_blocks(F, T_pad);
  const float2 *v = (const float2*)V, *u = (const float2*)target;
  if (kind == FD_LOSS_SCORE) hipLaunchKernelGGL(loss_sqerr_kernel<FD_LOSS_SCORE>, dim3(nb, B), dim3(256), 0, st, v, u, std, n, psum, pbad);
  else hipLaunchKernelGGL(loss_sqerr_kernel<FD_LOSS_FLOW>, dim3(nb, B), dim3(256), 0, st, v, u, std, n, psum, pbad);
  hipLaunchKernelGGL(loss_sqerr_finish_kernel, dim3(B), dim3(256), 0, st, psum, pbad, nb, sums_out, bad_out);
  FD_LAUNCH_CHECK();
  return FD_OK;
}
