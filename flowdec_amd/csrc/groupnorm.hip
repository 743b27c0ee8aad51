// groupnorm.hip -- GroupNorm as the network runs it on NHWC activations (nn.GroupNorm, layerspp.py:229,241): deterministic per-(b, c)
// partial sums, the per-(b, c) affine that the consuming kernels fuse (the group may straddle a virtual concat, ncsnpp.py:337), and
// act(GroupNorm(x)) as a stand-alone pass for operator-level parity.
#include "common.h"

namespace {

// =====================================================================================================
// GroupNorm statistics: per-(b, c) sum and sum of squares (nn.GroupNorm, layerspp.py:229,241)
// =====================================================================================================
// grid (blocks_per_image, B), 256 threads = (C/8 channel vectors) x (2048/C pixel lanes).  Every block writes its
// own partial (sum, sum of squares) per channel: part[b][block][c][2] (float) -- deterministic, no atomics.  The
// MFMA conv epilogue emits the same format for its output (one partial per 16x16 tile).
template <typename T>
__global__ __launch_bounds__(256) void channel_sums_kernel(const T* __restrict__ x, float* __restrict__ part, int HW,
                                                           int C, int px_per_block) {
  const int cv = C >> 3;            // channel vectors (power of two, <= 32)
  const int lanes = 256 / cv;       // pixel lanes
  const int t = threadIdx.x;
  const int c8 = (t % cv) * 8, pl = t / cv;
  const int b = blockIdx.y;
  const int p0 = blockIdx.x * px_per_block;
  const int p1 = min(p0 + px_per_block, HW);
  float s[8], ss[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) s[i] = ss[i] = 0.f;
  const T* base = x + (size_t)b * HW * C + c8;
  for (int p = p0 + pl; p < p1; p += lanes) {
    float v[8];
    fd_load_vec<T, 8>(base + (size_t)p * C, v);
#pragma unroll
    for (int i = 0; i < 8; ++i) { s[i] += v[i]; ss[i] = fmaf(v[i], v[i], ss[i]); }
  }
  __shared__ float red[256][17];
#pragma unroll
  for (int i = 0; i < 8; ++i) { red[t][i] = s[i]; red[t][8 + i] = ss[i]; }
  __syncthreads();
  for (int o = t; o < 2 * C; o += 256) {
    const int c = o >> 1, which = o & 1;
    const int tv = c >> 3, e = (c & 7) + 8 * which;
    float acc = 0.f;
    for (int l = 0; l < lanes; ++l) acc += red[l * cv + tv][e];
    part[(((size_t)b * gridDim.x + blockIdx.x) * C + c) * 2 + which] = acc;
  }
}

// One block per (group, b): reduce the partials of the group's channels over all tiles in double, then write the
// per-channel affine (a = rstd*gamma, d = beta - mean*rstd*gamma).  The group may straddle the two tensors of a
// virtual concat [C0 | C1] (e.g. GroupNorm(32, 320) over cat(h[256], hs[64]), ncsnpp.py:337).
__global__ __launch_bounds__(256) void gn_finalize_kernel(const float* __restrict__ p0, int tiles0, int stride0, int C0,
                                                          const float* __restrict__ p1, int tiles1, int stride1, int C1,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          float* __restrict__ affine, int groups, double inv_n, float eps) {
  const int C = C0 + C1, cpg = C / groups;
  const int g = blockIdx.x, b = blockIdx.y;
  const int c_lo = g * cpg;
  double s = 0.0, ss = 0.0;
  // channels of this group that live in tensor 0 / tensor 1
  const int a0 = c_lo < C0 ? c_lo : C0, a1 = (c_lo + cpg) < C0 ? (c_lo + cpg) : C0;          // [a0, a1) in tensor 0
  const int b0 = (c_lo > C0 ? c_lo : C0) - C0, b1 = ((c_lo + cpg) > C0 ? (c_lo + cpg) : C0) - C0;  // [b0, b1) in tensor 1
  const int n0 = a1 - a0, n1 = b1 - b0;
#pragma unroll 8   // independent loads in flight: the loop is latency-, not bandwidth-bound
  for (int i = threadIdx.x; i < n0 * tiles0; i += 256) {
    const int tl = i / n0, c = a0 + i % n0;
    const float2 v = *reinterpret_cast<const float2*>(p0 + (((size_t)b * tiles0 + tl) * stride0 + c) * 2);
    s += v.x; ss += v.y;
  }
#pragma unroll 8
  for (int i = threadIdx.x; i < n1 * tiles1; i += 256) {
    const int tl = i / n1, c = b0 + i % n1;
    const float2 v = *reinterpret_cast<const float2*>(p1 + (((size_t)b * tiles1 + tl) * stride1 + c) * 2);
    s += v.x; ss += v.y;
  }
  s = fd_wave_sum(s); ss = fd_wave_sum(ss);
  __shared__ double rs[4], rss[4];
  __shared__ float sh_mean_rstd[2];
  if ((threadIdx.x & 63) == 0) { rs[threadIdx.x >> 6] = s; rss[threadIdx.x >> 6] = ss; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double S = rs[0] + rs[1] + rs[2] + rs[3], SS = rss[0] + rss[1] + rss[2] + rss[3];
    const double mean = S * inv_n;
    double var = SS * inv_n - mean * mean;
    var = var < 0.0 ? 0.0 : var;
    const double rstd = 1.0 / sqrt(var + (double)eps);
    sh_mean_rstd[0] = (float)rstd;
    sh_mean_rstd[1] = (float)(mean * rstd);
  }
  __syncthreads();
  if (threadIdx.x < cpg) {
    const int c = c_lo + threadIdx.x;
    const float a = sh_mean_rstd[0] * gamma[c];
    affine[((size_t)b * C + c) * 2] = a;
    affine[((size_t)b * C + c) * 2 + 1] = beta[c] - sh_mean_rstd[1] * gamma[c];
  }
}

// silu(a*x + d), per-(b,c) affine: act(GroupNorm(x)) as a stand-alone pass (operator-level parity; fused on the hot path)
template <typename T>
__global__ __launch_bounds__(256) void gn_silu_apply_kernel(const T* __restrict__ x, const float* __restrict__ affine, T* __restrict__ out,
                                                            long long hw, int C, long long nvec) {
  const int cv = C >> 3;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < nvec; i += (long long)gridDim.x * 256) {
    const int c8 = (int)(i % cv) * 8;
    const long long b = i / cv / hw;
    float v[8];
    fd_load_vec<T, 8>(x + i * 8, v);
    const float* ad = affine + ((size_t)b * C + c8) * 2;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = fd_silu(fmaf(v[j], ad[2 * j], ad[2 * j + 1]));
    fd_store_vec<T, 8>(out + i * 8, v);
  }
}

}  // namespace

extern "C" int fd_channel_sums_tiles(int H, int W) { return fd_cdiv((long long)H * W, 2048); }

extern "C" int fd_channel_sums(const void* x, float* part, int B, int H, int W, int C, int dtype, void* stream) {
  FD_REQUIRE(x && part, "fd_channel_sums: null pointer");
  FD_REQUIRE(C >= 8 && C <= 256 && (C & (C - 1)) == 0, "fd_channel_sums: C must be a power of two in [8,256] (got %d)", C);
  FD_REQUIRE(dtype == FD_F32 || dtype == FD_BF16, "fd_channel_sums: bad dtype");
  hipStream_t st = fd_stream(stream);
  const int HW = H * W;
  const int ppb = 2048;  // pixels per block
  dim3 grid(fd_cdiv(HW, ppb), B);
  if (dtype == FD_BF16)
    hipLaunchKernelGGL(channel_sums_kernel<bf16>, grid, dim3(256), 0, st, (const bf16*)x, part, HW, C, ppb);
  else
    hipLaunchKernelGGL(channel_sums_kernel<float>, grid, dim3(256), 0, st, (const float*)x, part, HW, C, ppb);
  FD_LAUNCH_CHECK();
  return FD_OK;
}

extern "C" int fd_gn_silu_apply(const void* x, const float* affine, void* out, int B, long long hw, int C, int dtype, void* stream) {
  FD_REQUIRE(x && affine && out, "fd_gn_silu_apply: null pointer");
  FD_REQUIRE(B > 0 && hw > 0 && C > 0 && C % 8 == 0, "fd_gn_silu_apply: C must be a multiple of 8");
  FD_REQUIRE(dtype == FD_F32 || dtype == FD_BF16, "fd_gn_silu_apply: bad dtype");
  const long long nvec = (long long)B * hw * (C / 8);
  const dim3 grid(grid_for(nvec, 256, 1 << 16));
  if (dtype == FD_BF16) hipLaunchKernelGGL(gn_silu_apply_kernel<bf16>, grid, dim3(256), 0, fd_stream(stream), (const bf16*)x, affine, (bf16*)out, hw, C, nvec);
  else hipLaunchKernelGGL(gn_silu_apply_kernel<float>, grid, dim3(256), 0, fd_stream(stream), (const float*)x, affine, (float*)out, hw, C, nvec);
  FD_LAUNCH_CHECK();
  return FD_OK;
}

extern "C" int fd_gn_finalize(const float* part0, int tiles0, int stride0, int C0, const float* part1, int tiles1, int stride1,
                              int C1, const float* gamma, const float* beta, float* affine, int B, int groups, long long hw,
                              float eps, void* stream) {
  FD_REQUIRE(part0 && gamma && beta && affine, "fd_gn_finalize: null pointer");
  FD_REQUIRE((C1 == 0) == (part1 == nullptr), "fd_gn_finalize: part1 / C1 mismatch");
  FD_REQUIRE(tiles0 > 0 && stride0 >= C0 && (C1 == 0 || (tiles1 > 0 && stride1 >= C1)), "fd_gn_finalize: bad partial geometry");
  const int C = C0 + C1;
  FD_REQUIRE(groups > 0 && C % groups == 0 && C / groups <= 256, "fd_gn_finalize: C=%d not divisible by groups=%d", C, groups);
  const double inv_n = 1.0 / ((double)hw * (C / groups));
  hipLaunchKernelGGL(gn_finalize_kernel, dim3(groups, B), dim3(256), 0, fd_stream(stream), part0, tiles0, stride0, C0, part1, tiles1,
                     stride1, C1, gamma, beta, affine, groups, inv_n, eps);
  FD_LAUNCH_CHECK();
  return FD_OK;
}
