// solver_ops.hip -- the solvers' own arithmetic on the complex [B][F][T] state, apart from the updates fused with the output layer
// (net_edges.hip): the initial state x0 = Y + sigma_y * noise (model.py:512, :530-536) and the prior sample of the ScoreDec sampler
// (sdes.py:197-202), both from a noise buffer or from per-clip seeds (noise.h); the seeded noise as a buffer; the helpers of the adaptive
// Dormand-Prince driver (solve.hip: adaptive_solve), batch-global and per clip; and the stitch of a long recording's overlapping chunks.
#include "common.h"
#include "internal.h"
#include "noise.h"

namespace {

// x0 = Y + sigma_fac * (sigma_y[f] * noise).type(complex64)   (model.py:512, :530-536); sigma is float64
// SEEDED with frame0 (int32 [B], may be null): row b is a chunk of a longer recording that starts at frame frame0[b] of it, and the
// noise is the recording's -- z(seed, draw, f, frame0[b] + t): two chunks that overlap start from the same noise where they do
template <bool SEEDED>
__global__ void init_state_kernel(const float2* __restrict__ Y, const float2* __restrict__ noise, const unsigned long long* __restrict__ seeds,
                                  const int* __restrict__ frame0, int draw, const double* __restrict__ sigma, int sigma_n, float sigma_fac,
                                  float2* __restrict__ x0, int F, int T, long long n) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int f = (int)((i / T) % F);
    const double s = sigma[sigma_n == 1 ? 0 : f];
    const float2 nz = noise_elem<SEEDED>(noise, seeds, draw, i, F, T, frame0), yv = Y[i];
    const float nx = (float)(s * (double)nz.x), ny = (float)(s * (double)nz.y);
    float2 o = {yv.x + sigma_fac * nx, yv.y + sigma_fac * ny};
    x0[i] = o;
  }
}

// dst = a + cq * q  (prior sample x_T = Y + std(T) * z, sdes.py:197-202); q = a [B][F][T] plane of noise (buffer or seeds; SEEDED with
// frame0 as in init_state_kernel: the plane's columns are the absolute frames frame0[b] + t).  AT = false: frame0 is not looked at -- the
// instantiation of the entry points that have none, whose code is what it was before frame0 existed (MEASUREMENTS.md "Baselines: long-form
// and streaming": the one kernel for both cost them 0.03 %)
template <bool SEEDED, bool AT>
__global__ void caxpy_kernel(const float2* __restrict__ a, const float2* __restrict__ q, const unsigned long long* __restrict__ seeds,
                             const int* __restrict__ frame0, int draw, float cq, float2* __restrict__ dst, int F, int T, long long n) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const float2 av = a[i], qv = noise_elem<SEEDED>(q, seeds, draw, i, F, T, AT ? frame0 : nullptr);
    float2 o = {fmaf(cq, qv.x, av.x), fmaf(cq, qv.y, av.y)};
    dst[i] = o;
  }
}

// The planes draw0 .. draw0 + n_draws - 1 of the seeded noise as a buffer: out[d][b][f][t] (complex64; BITS: the two raw words of
// every element as uint32 instead).  One thread = one frame pair = one Philox call; with an even T the pair is one 16-byte store.
// frame0 (int32 [B], may be null = zeros): column t of row b holds absolute frame frame0[b] + t.  A Philox call serves the ABSOLUTE frames
// (2k, 2k + 1): with an odd frame0 a thread's pair of columns straddles two calls -- (r2, r3) of the first, (r0, r1) of the next.
template <bool BITS>
__global__ __launch_bounds__(256) void noise_fill_kernel(float2* __restrict__ out, const unsigned long long* __restrict__ seeds,
                                                         const int* __restrict__ frame0, int B, int F, int T, int draw0, long long npairs) {
  const int tp = (T + 1) >> 1;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < npairs; i += (long long)gridDim.x * 256) {
    const int t = 2 * (int)(i % tp);
    long long q = i / tp;
    const int f = (int)(q % F); q /= F;
    const int b = (int)(q % B), d = (int)(q / B);
    unsigned r[4];
    const unsigned long long seed = seeds[b];
    const unsigned ta = (unsigned)((frame0 ? frame0[b] : 0) + t);   // absolute frame of the first column
    philox4x32_10(ta >> 1, (unsigned)f, (unsigned)(draw0 + d), 0u, (unsigned)seed, (unsigned)(seed >> 32), r);
    if (ta & 1u) {
      unsigned q[4];
      philox4x32_10((ta >> 1) + 1u, (unsigned)f, (unsigned)(draw0 + d), 0u, (unsigned)seed, (unsigned)(seed >> 32), q);
      r[0] = r[2]; r[1] = r[3]; r[2] = q[0]; r[3] = q[1];
    }
    float2 z0, z1;
    if constexpr (BITS) {
      z0 = float2{__uint_as_float(r[0]), __uint_as_float(r[1])};
      z1 = float2{__uint_as_float(r[2]), __uint_as_float(r[3])};
    } else {
      z0 = fd_noise_from_bits(uint2{r[0], r[1]});
      z1 = fd_noise_from_bits(uint2{r[2], r[3]});
    }
    float2* o = out + (((long long)d * B + b) * F + f) * T + t;
    if ((T & 1) == 0) {
      *reinterpret_cast<float4*>(o) = float4{z0.x, z0.y, z1.x, z1.y};
    } else {
      o[0] = z0;
      if (t + 1 < T) o[1] = z1;
    }
  }
}

// ---- adaptive Dormand-Prince driver helpers (solve.hip: adaptive_solve) ------------------------------------
struct fd_lincomb_args { const float2* k[7]; float c[7]; };
// dst = cx * x + dt * sum_i c[i] * k[i]   (null k[i] / zero c[i] are skipped by the host).  One body for the batch-global launch (off = 0,
// n = the whole state) and the per-clip launch (off = the clip's first element, n = one clip): an element's bits depend on its operands only
__device__ __forceinline__ void ode_lincomb_body(const float2* __restrict__ x, float cx, float dt, const fd_lincomb_args& a, int nk, float2* __restrict__ dst,
                                                 long long off, long long n) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    float sx = 0.f, sy = 0.f;
    for (int j = 0; j < nk; ++j) { const float2 kv = a.k[j][off + i]; sx = fmaf(a.c[j], kv.x, sx); sy = fmaf(a.c[j], kv.y, sy); }
    float2 o = {dt * sx, dt * sy};
    if (cx != 0.f) { const float2 xv = x[off + i]; o.x = fmaf(cx, xv.x, o.x); o.y = fmaf(cx, xv.y, o.y); }
    dst[off + i] = o;
  }
}
__global__ void ode_lincomb_kernel(const float2* __restrict__ x, float cx, float dt, fd_lincomb_args a, int nk, float2* __restrict__ dst, long long n) {
  ode_lincomb_body(x, cx, dt, a, nk, dst, 0, n);
}
// per-clip step sizes: grid (blocks, B); clip blockIdx.y = elements [b n, (b + 1) n) takes dt[b] from device memory
__global__ void ode_lincomb_clips_kernel(const float2* __restrict__ x, float cx, const float* __restrict__ dt, fd_lincomb_args a, int nk,
                                         float2* __restrict__ dst, long long n) {
  ode_lincomb_body(x, cx, dt[blockIdx.y], a, nk, dst, (long long)blockIdx.y * n, n);
}
// *out = sum over the block's elements of |p - q|^2 / (atol + rtol * max(|r|, |s|))^2   (complex moduli; q may be null).  The partition
// over (gridDim.x, 256 threads), the wave reduction and the red[0..3] order are the same whichever launch calls it
__device__ __forceinline__ void ode_scaled_sq_body(const float2* __restrict__ p, const float2* __restrict__ q, const float2* __restrict__ r,
                                                   const float2* __restrict__ s, float atol, float rtol, double* __restrict__ out, long long n) {
  double acc = 0.0;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    float2 d = p[i];
    if (q) { const float2 qv = q[i]; d.x -= qv.x; d.y -= qv.y; }
    const float2 rv = r[i], sv = s[i];
    const float m = fmaxf(sqrtf(rv.x * rv.x + rv.y * rv.y), sqrtf(sv.x * sv.x + sv.y * sv.y));
    const float sc = atol + rtol * m;
    acc += (double)((d.x * d.x + d.y * d.y) / (sc * sc));
  }
  acc = fd_wave_sum(acc);
  __shared__ double red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) *out = red[0] + red[1] + red[2] + red[3];
}
// partial[block]: one sum over the whole [n] state
__global__ __launch_bounds__(256) void ode_scaled_sq_kernel(const float2* __restrict__ p, const float2* __restrict__ q, const float2* __restrict__ r,
                                                            const float2* __restrict__ s, float atol, float rtol, double* __restrict__ partial, long long n) {
  ode_scaled_sq_body(p, q, r, s, atol, rtol, partial + blockIdx.x, n);
}
// partial[b][block]: grid (blocks, B); block (j, b) is block j of the one-clip launch on clip b's n elements
__global__ __launch_bounds__(256) void ode_scaled_sq_clips_kernel(const float2* __restrict__ p, const float2* __restrict__ q, const float2* __restrict__ r,
                                                                  const float2* __restrict__ s, float atol, float rtol, double* __restrict__ partial,
                                                                  long long n) {
  const long long off = (long long)blockIdx.y * n;
  ode_scaled_sq_body(p + off, q ? q + off : nullptr, r + off, s + off, atol, rtol, partial + (size_t)blockIdx.y * gridDim.x + blockIdx.x, n);
}
// masked commit of an attempted step: for every clip b (= blockIdx.y) with accept[b] != 0, x <- x_new and k0 <- k6 (the FSAL stage); a clip
// that landed on checkpoint ckpt[b] > 0 also writes its plane to traj[ckpt[b]][b] (traj may be null).  Other clips are not touched.
__global__ void ode_commit_clips_kernel(const int* __restrict__ accept, const int* __restrict__ ckpt, const float2* __restrict__ x_new,
                                        const float2* __restrict__ k6, float2* __restrict__ x, float2* __restrict__ k0, float2* __restrict__ traj,
                                        int B, long long n) {
  const int b = blockIdx.y;
  if (!accept[b]) return;
  const long long off = (long long)b * n;
  const int c = ckpt[b];
  float2* tr = (traj && c > 0) ? traj + ((long long)c * B + b) * n : nullptr;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const float2 v = x_new[off + i];
    x[off + i] = v;
    k0[off + i] = k6[off + i];
    if (tr) tr[i] = v;
  }
}

}  // namespace

int fd_init_state(const float* Y, const fd_noise_src& noise, const double* sigma_dev, int sigma_n, float sigma_fac, float* x0, int B,
                  int F, int T, hipStream_t st) {
  const long long n = (long long)B * F * T;
  if (noise.seeds)
    hipLaunchKernelGGL(init_state_kernel<true>, dim3(grid_for(n, 256, 8192)), dim3(256), 0, st, (const float2*)Y, (const float2*)nullptr, noise.seeds,
                       noise.frame0, noise.draw, sigma_dev, sigma_n, sigma_fac, (float2*)x0, F, T, n);
  else
    hipLaunchKernelGGL(init_state_kernel<false>, dim3(grid_for(n, 256, 8192)), dim3(256), 0, st, (const float2*)Y, (const float2*)noise.ptr,
                       (const unsigned long long*)nullptr, (const int*)nullptr, 0, sigma_dev, sigma_n, sigma_fac, (float2*)x0, F, T, n);
  FD_LAUNCH_CHECK();
  return FD_OK;
}

int fd_caxpy(const float* a, const fd_noise_src& q, float cq, float* dst, int B, int F, int T, hipStream_t st) {
  const long long n = (long long)B * F * T;
  if (q.seeds && q.frame0)
    hipLaunchKernelGGL((caxpy_kernel<true, true>), dim3(grid_for(n, 256, 8192)), dim3(256), 0, st, (const float2*)a, (const float2*)nullptr, q.seeds, q.frame0,
                       q.draw, cq, (float2*)dst, F, T, n);
  else if (q.seeds)
    hipLaunchKernelGGL((caxpy_kernel<true, false>), dim3(grid_for(n, 256, 8192)), dim3(256), 0, st, (const float2*)a, (const float2*)nullptr, q.seeds,
                       (const int*)nullptr, q.draw, cq, (float2*)dst, F, T, n);
  else
    hipLaunchKernelGGL((caxpy_kernel<false, false>), dim3(grid_for(n, 256, 8192)), dim3(256), 0, st, (const float2*)a, (const float2*)q.ptr,
                       (const unsigned long long*)nullptr, (const int*)nullptr, 0, cq, (float2*)dst, F, T, n);
  FD_LAUNCH_CHECK();
  return FD_OK;
}

static int noise_fill_impl(const char* who, void* out, const unsigned long long* seeds, const int* frame0, int B, int F, int T_pad, int draw0, int n_draws,
                           int mode, void* stream) {
  FD_REQUIRE(out && seeds, "%s: null pointer", who);
  FD_REQUIRE(B > 0 && F > 0 && T_pad > 0 && draw0 >= 0 && n_draws > 0, "%s: bad shape (B=%d F=%d T_pad=%d draw0=%d n_draws=%d)", who, B, F, T_pad, draw0, n_draws);
  FD_REQUIRE(mode == FD_NOISE_GAUSSIAN || mode == FD_NOISE_BITS, "%s: unknown mode %d", who, mode);
  FD_REQUIRE((uintptr_t)out % 16 == 0, "%s: out must be 16-byte aligned", who);
  const long long npairs = (long long)n_draws * B * F * ((T_pad + 1) / 2);
  const dim3 grid(grid_for(npairs, 256, 1 << 16));
  if (mode == FD_NOISE_BITS)
    hipLaunchKernelGGL(noise_fill_kernel<true>, grid, dim3(256), 0, fd_stream(stream), (float2*)out, seeds, frame0, B, F, T_pad, draw0, npairs);
  else
    hipLaunchKernelGGL(noise_fill_kernel<false>, grid, dim3(256), 0, fd_stream(stream), (float2*)out, seeds, frame0, B, F, T_pad, draw0, npairs);
  FD_LAUNCH_CHECK();
  return FD_OK;
}

extern "C" int fd_noise_fill(void* out, const unsigned long long* seeds, int B, int F, int T_pad, int draw0, int n_draws, int mode, void* stream) {
  return noise_fill_impl("fd_noise_fill", out, seeds, nullptr, B, F, T_pad, draw0, n_draws, mode, stream);
}

// fd_noise_fill at absolute frames: column t of row b is frame frame0[b] + t (frame0: DEVICE int32 [B], 0 <= frame0[b], frame0[b] + T_pad
// < 2^31 -- the caller's contract, the values live on the device; NULL = zeros = fd_noise_fill)
extern "C" int fd_noise_fill_at(void* out, const unsigned long long* seeds, const int* frame0, int B, int F, int T_pad, int draw0, int n_draws, int mode,
                                void* stream) {
  return noise_fill_impl("fd_noise_fill_at", out, seeds, frame0, B, F, T_pad, draw0, n_draws, mode, stream);
}

// ---- long-form stitching: a recording's output [n] from the outputs of its overlapping rows (fd_enhance_chunks) ------------------------
// Row r holds the recording's samples [starts[r], starts[r] + row_stride) (its tail may be unused); bounds[r - 1] = the boundary between the
// rows r - 1 and r (ascending).  Sample i belongs to the row whose [bounds[r - 1], bounds[r]) contains it; within xfade / 2 of a boundary
// between the rows a (earlier) and b it is a + w (b - a) with w = weights[i - (boundary - xfade / 2)], each operation rounded on its own
// (NumPy float32 gives the same bits).  One output element per thread; an index outside a row is clamped into it (wrong tables give wrong
// samples, never an out-of-bounds access).
__global__ __launch_bounds__(256) void stitch_kernel(const float* __restrict__ rows, long long row_stride, const int* __restrict__ starts,
                                                     const int* __restrict__ bounds, int n_rows, const float* __restrict__ weights, int xfade,
                                                     float* __restrict__ out, long long n) {
#pragma clang fp contract(off)   // three roundings: without this, a + w * d is one fma (also through __fmul_rn / __fadd_rn, which inline to operators)
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= n) return;
  int lo = 0, hi = n_rows - 1;          // r = number of boundaries <= i
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((long long)bounds[mid - 1] <= i) lo = mid; else hi = mid - 1;
  }
  const int r = lo, half = xfade >> 1;
  auto at = [&](int row, long long idx) {
    long long k = idx - starts[row];
    k = k < 0 ? 0 : (k >= row_stride ? row_stride - 1 : k);
    return rows[(long long)row * row_stride + k];
  };
  float o;
  int a = -1;                            // the earlier row of the cross-fade that covers i, if any
  if (r > 0 && i < (long long)bounds[r - 1] + half) a = r - 1;
  else if (r + 1 < n_rows && i >= (long long)bounds[r] - half) a = r;
  if (a >= 0) {
    long long k = i - ((long long)bounds[a] - half);
    k = k < 0 ? 0 : (k >= xfade ? xfade - 1 : k);
    const float va = at(a, i), vb = at(a + 1, i);
    const float d = vb - va;
    const float p = weights[k] * d;
    o = va + p;
  } else {
    o = at(r, i);
  }
  out[i] = o;
}

extern "C" int fd_stitch_chunks(const float* rows, long long row_stride, const int* starts, const int* bounds, int n_rows, const float* weights, int xfade,
                                float* out, long long n, void* stream) {
  FD_REQUIRE(rows && starts && out && n_rows >= 1 && row_stride >= 1 && n >= 1, "fd_stitch_chunks: bad arguments");
  FD_REQUIRE(n <= 0x7fffffffll, "fd_stitch_chunks: at most 2^31 - 1 samples per recording (got %lld)", n);
  FD_REQUIRE(n_rows == 1 || (bounds && xfade >= 0 && xfade % 2 == 0 && (xfade == 0 || weights)), "fd_stitch_chunks: several rows need bounds, an even xfade and its weights");
  hipLaunchKernelGGL(stitch_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, fd_stream(stream), rows, row_stride, starts, bounds, n_rows, weights,
                     n_rows == 1 ? 0 : xfade, out, n);
  FD_LAUNCH_CHECK();
  return FD_OK;
}

// the terms of a linear combination that count -- k[j] present and c[j] != 0, at most 7 -- packed to the front of `a`; returns their number
static int compact_lincomb(const float* const* k, const float* c, int nk, fd_lincomb_args* a) {
  int m = 0;
  for (int j = 0; j < nk && j < 7; ++j)
    if (k[j] && c[j] != 0.f) { a->k[m] = (const float2*)k[j]; a->c[m] = c[j]; ++m; }
  for (int j = m; j < 7; ++j) { a->k[j] = nullptr; a->c[j] = 0.f; }
  return m;
}

int fd_ode_lincomb(const float* x, float cx, float dt, const float* const* k, const float* c, int nk, float* dst, long long n, hipStream_t st) {
  fd_lincomb_args a;
  const int m = compact_lincomb(k, c, nk, &a);
  hipLaunchKernelGGL(ode_lincomb_kernel, dim3(grid_for(n, 256, 8192)), dim3(256), 0, st, (const float2*)x, cx, dt, a, m, (float2*)dst, n);
  FD_LAUNCH_CHECK();
  return FD_OK;
}

int fd_ode_scaled_sq(const float* p, const float* q, const float* r, const float* s, float atol, float rtol, double* partial, int nblocks,
                     long long n, hipStream_t st) {
  hipLaunchKernelGGL(ode_scaled_sq_kernel, dim3(nblocks), dim3(256), 0, st, (const float2*)p, (const float2*)q, (const float2*)r, (const float2*)s,
                     atol, rtol, partial, n);
  FD_LAUNCH_CHECK();
  return FD_OK;
}

int fd_ode_lincomb_clips(const float* x, float cx, const float* dt_dev, const float* const* k, const float* c, int nk, float* dst, int B, long long n,
                         hipStream_t st) {
  fd_lincomb_args a;
  const int m = compact_lincomb(k, c, nk, &a);
  hipLaunchKernelGGL(ode_lincomb_clips_kernel, dim3(grid_for(n, 256, 8192), B), dim3(256), 0, st, (const float2*)x, cx, dt_dev, a, m, (float2*)dst, n);
  FD_LAUNCH_CHECK();
  return FD_OK;
}

int fd_ode_scaled_sq_clips(const float* p, const float* q, const float* r, const float* s, float atol, float rtol, double* partial, int nblocks, int B,
                           long long n, hipStream_t st) {
  hipLaunchKernelGGL(ode_scaled_sq_clips_kernel, dim3(nblocks, B), dim3(256), 0, st, (const float2*)p, (const float2*)q, (const float2*)r,
                     (const float2*)s, atol, rtol, partial, n);
  FD_LAUNCH_CHECK();
  return FD_OK;
}

int fd_ode_commit_clips(const int* accept, const int* ckpt, const float* x_new, const float* k6, float* x, float* k0, float* traj, int B, long long n,
                        hipStream_t st) {
  hipLaunchKernelGGL(ode_commit_clips_kernel, dim3(grid_for(n, 256, 8192), B), dim3(256), 0, st, accept, ckpt, (const float2*)x_new, (const float2*)k6,
                     (float2*)x, (float2*)k0, (float2*)traj, B, n);
  FD_LAUNCH_CHECK();
  return FD_OK;
}
