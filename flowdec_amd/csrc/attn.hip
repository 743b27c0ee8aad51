// attn.hip -- the bottleneck self-attention block of the SGMSE-style NCSN++ backbone (AttnBlockpp, layerspp.py:72-101 with
// skip_rescale; NIN = layers.py:566-575):
//   h = GroupNorm_0(x)  (no SiLU);  q, k, v = h W_i + b_i;  w = softmax_j(q_i . k_j * C^-0.5) over all H*W positions;
//   out = (x + (w v) W_3 + b_3) / sqrt(2)
// Exact float32 arithmetic in every precision mode (v_mfma_f32_16x16x4_f32 = a k-ordered f32 fma chain): only the storage type of
// x / out follows the mode.  Two launches:
//   attn_qkv_kernel   one workgroup per (16 positions, q|k|v, image): the normalised rows in LDS, [16 x C] . [C x C] + b -> f32 workspace
//   attn_core_kernel  one workgroup per (16 queries, image): K / V streamed through LDS in tiles of 64 keys (16 per wave, every wave keeps
//                     its own running max / sum / output), the four waves merged in a fixed order, then the output projection, the
//                     residual, the store and the GroupNorm partial sums of the stored tensor ([B][tiles][C][2], tiles = 16 rows each)
// No atomics, fixed reduction orders, every workgroup reads only its own image: a clip gives the same bits alone or in any batch.
#include <math.h>

#include "common.h"
#include "internal.h"

namespace {

constexpr int QT = 16;   // positions per workgroup (queries of the core kernel, rows of the projection)
constexpr int KT = 64;   // keys per LDS tile: 16 per wave

// LDS image of a [rows][C] f32 tile: row-major, the column XOR-swizzled by the row so that 16 rows x 4 consecutive columns (the A / B
// operand of one 16x16x4 step) and 4 rows x 16 consecutive columns hit distinct banks.  Keeps 4-aligned column groups contiguous.
template <int C>
__device__ __forceinline__ int swz(int row, int c) { return row * C + (c ^ (((row & 15) * 4) & (C - 4))); }

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// q|k|v [3][B][N][C] (f32) = GroupNorm_0(x) . w_qkv[:, which*C : (which+1)*C] + b_qkv.   affine = [B][C][2] (a, d): h = a x + d.
template <typename T, int C>
__global__ __launch_bounds__(256) void attn_qkv_kernel(const T* __restrict__ x, const float* __restrict__ affine, const float* __restrict__ w_qkv,
                                                       const float* __restrict__ b_qkv, float* __restrict__ qkv, int N) {
  constexpr int NCT = C / 16, TPW = (NCT + 3) / 4;   // 16-column tiles, per wave
  __shared__ float hs[QT * C];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int p0 = blockIdx.x * QT, which = blockIdx.y, b = blockIdx.z;
  const int B = gridDim.z;
  for (int i = t; i < QT * C / 4; i += 256) {
    const int r = i / (C / 4), c = (i % (C / 4)) * 4;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (p0 + r < N) {
      fd_load_vec<T, 4>(x + ((size_t)b * N + p0 + r) * C + c, v);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float2 ad = *reinterpret_cast<const float2*>(affine + ((size_t)b * C + c + e) * 2);
        v[e] = fmaf(ad.x, v[e], ad.y);
      }
    }
    *reinterpret_cast<f32x4*>(&hs[swz<C>(r, c)]) = f32x4{v[0], v[1], v[2], v[3]};
  }
  __syncthreads();
  const int li = lane & 15, lk = lane >> 4;
  f32x4 acc[TPW];
#pragma unroll
  for (int u = 0; u < TPW; ++u) {
    const int j = wv + 4 * u;
    const float bv = j < NCT ? b_qkv[which * C + 16 * j + li] : 0.f;
    acc[u] = f32x4{bv, bv, bv, bv};
  }
  if (wv < NCT) {
    for (int s = 0; s < C / 4; ++s) {
      const float a = hs[swz<C>(li, 4 * s + lk)];
      const float* wrow = w_qkv + (size_t)(4 * s + lk) * (3 * C) + which * C + li;
#pragma unroll
      for (int u = 0; u < TPW; ++u) {
        const int j = wv + 4 * u;
        if (j < NCT) acc[u] = mfma4(a, wrow[16 * j], acc[u]);
      }
    }
  }
  float* dst = qkv + ((size_t)which * B + b) * (size_t)N * C;
#pragma unroll
  for (int u = 0; u < TPW; ++u) {
    const int j = wv + 4 * u;
    if (j >= NCT) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int p = p0 + 4 * lk + r;
      if (p < N) dst[(size_t)p * C + 16 * j + li] = acc[u][r];
    }
  }
}

// Stage rows [k0, k0 + KT) of src ([N][C] f32) into the swizzled LDS tile; rows past N are zero.
template <int C>
__device__ __forceinline__ void stage_tile(float* buf, const float* __restrict__ src, int k0, int N, int t) {
  for (int i = t; i < KT * C / 4; i += 256) {
    const int r = i / (C / 4), c = (i % (C / 4)) * 4;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (k0 + r < N) v = *reinterpret_cast<const f32x4*>(src + (size_t)(k0 + r) * C + c);
    *reinterpret_cast<f32x4*>(&buf[swz<C>(r, c)]) = v;
  }
}

template <typename T, int C>
__global__ __launch_bounds__(256) void attn_core_kernel(const float* __restrict__ qkv, const T* __restrict__ x, const float* __restrict__ w_out,
                                                        const float* __restrict__ b_out, T* __restrict__ out, float* __restrict__ part, int N,
                                                        float scale) {
  constexpr int NCT = C / 16, TPW = (NCT + 3) / 4;
  __shared__ float buf[KT * C];   // K tile, then V tile; after the key loop: the four waves' partial outputs, then the merged output
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int q0 = blockIdx.x * QT, b = blockIdx.y, B = gridDim.y;
  const int li = lane & 15, lk = lane >> 4;
  const size_t plane = (size_t)B * N * C;
  const float* Q = qkv + (size_t)b * N * C;
  const float* K = Q + plane;
  const float* V = K + plane;
  // S^T = K . Q^T: the B operand of step s is Q[q = li][c = 4s + lk] -- held in registers for the whole key loop
  float qreg[C / 4];
  {
    const int q = q0 + li;
#pragma unroll
    for (int s = 0; s < C / 4; ++s) qreg[s] = q < N ? Q[(size_t)q * C + 4 * s + lk] : 0.f;
  }
  // O^T (C x 16 queries): lane holds O^T[c = 16 j + 4 lk + r][q = li]; the running max / sum of query li (same in the 4 lane groups)
  f32x4 o[NCT];
#pragma unroll
  for (int j = 0; j < NCT; ++j) o[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;
  for (int k0 = 0; k0 < N; k0 += KT) {
    const int kb = k0 + 16 * wv;   // this wave's first key
    __syncthreads();
    stage_tile<C>(buf, K, k0, N, t);
    __syncthreads();
    f32x4 p = {0.f, 0.f, 0.f, 0.f};
    if (kb < N) {   // wave-uniform
      f32x4 st = {0.f, 0.f, 0.f, 0.f};
#pragma unroll   // (fully: qreg must stay in registers)
      for (int s = 0; s < C / 4; ++s) st = mfma4(buf[swz<C>(16 * wv + li, 4 * s + lk)], qreg[s], st);
      // lane holds S^T[key = kb + 4 lk + r][q = li]: the 16 keys of query li live in 4 registers x 4 lane groups
      float mx = -INFINITY;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        st[r] = kb + 4 * lk + r < N ? st[r] * scale : -INFINITY;
        mx = fmaxf(mx, st[r]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float mn = fmaxf(m, mx);   // finite: key kb < N is valid
      const float alpha = expf(m - mn);
      float ps = 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) { p[r] = expf(st[r] - mn); ps += p[r]; }
      ps += __shfl_xor(ps, 16, 64);
      ps += __shfl_xor(ps, 32, 64);
      l = fmaf(l, alpha, ps);
      m = mn;
#pragma unroll
      for (int j = 0; j < NCT; ++j) o[j] *= alpha;
    }
    __syncthreads();
    stage_tile<C>(buf, V, k0, N, t);
    __syncthreads();
    if (kb < N) {
      // O^T += V^T . P^T over this wave's 16 keys, step r = keys {kb + 4 g + r}: P^T's B operand is register r of the score tile as is
#pragma unroll
      for (int j = 0; j < NCT; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) o[j] = mfma4(buf[swz<C>(16 * wv + 4 * lk + r, 16 * j + li)], p[r], o[j]);
    }
  }
  // ---- merge the four waves (fixed order): M = max m_w, L = sum_w l_w e_w, O = sum_w O_w e_w / L with e_w = exp(m_w - M) ----
  __syncthreads();
  if (lk == 0) { buf[wv * 32 + 2 * li] = m; buf[wv * 32 + 2 * li + 1] = l; }
  __syncthreads();
  float e_self;
  {
    float mw[4], lw[4], M = -INFINITY;
#pragma unroll
    for (int w = 0; w < 4; ++w) { mw[w] = buf[w * 32 + 2 * li]; lw[w] = buf[w * 32 + 2 * li + 1]; M = fmaxf(M, mw[w]); }
    float L = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) L += mw[w] == -INFINITY ? 0.f : lw[w] * expf(mw[w] - M);
    e_self = m == -INFINITY ? 0.f : expf(m - M) / L;
  }
  __syncthreads();
  float* ow = buf + wv * (QT * C);
#pragma unroll
  for (int j = 0; j < NCT; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) ow[swz<C>(li, 16 * j + 4 * lk + r)] = o[j][r] * e_self;
  __syncthreads();
  for (int i = t; i < QT * C; i += 256) {   // in place into wave 0's slot: every element is read and written by one thread
    const int q = i / C, c = i % C, a = swz<C>(q, c);
    buf[a] = ((buf[a] + buf[QT * C + a]) + buf[2 * QT * C + a]) + buf[3 * QT * C + a];
  }
  __syncthreads();
  // ---- out = (x + O . w_out + b_out) / sqrt(2); lane holds row q0 + 4 lk + r, column 16 j + li ----
  f32x4 acc[TPW];
#pragma unroll
  for (int u = 0; u < TPW; ++u) {
    const int j = wv + 4 * u;
    const float bv = j < NCT ? b_out[16 * j + li] : 0.f;
    acc[u] = f32x4{bv, bv, bv, bv};
  }
  if (wv < NCT) {
    for (int s = 0; s < C / 4; ++s) {
      const float a = buf[swz<C>(li, 4 * s + lk)];
      const float* wrow = w_out + (size_t)(4 * s + lk) * C + li;
#pragma unroll
      for (int u = 0; u < TPW; ++u) {
        const int j = wv + 4 * u;
        if (j < NCT) acc[u] = mfma4(a, wrow[16 * j], acc[u]);
      }
    }
  }
  const float rs2 = 0.70710678118654752440f;
#pragma unroll
  for (int u = 0; u < TPW; ++u) {
    const int j = wv + 4 * u;
    if (j >= NCT) continue;
    const int c = 16 * j + li;
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int q = q0 + 4 * lk + r;
      if (q < N) {
        const size_t at = ((size_t)b * N + q) * C + c;
        const float v = (Elem<T>::ld(x + at) + acc[u][r]) * rs2;
        const T vs = (T)v;
        out[at] = vs;
        const float vq = (float)vs;   // statistics of the stored (rounded) tensor
        s1 += vq; s2 = fmaf(vq, vq, s2);
      }
    }
    s1 += __shfl_xor(s1, 16, 64); s2 += __shfl_xor(s2, 16, 64);
    s1 += __shfl_xor(s1, 32, 64); s2 += __shfl_xor(s2, 32, 64);
    if (part && lk == 0) *reinterpret_cast<float2*>(part + (((size_t)b * gridDim.x + blockIdx.x) * C + c) * 2) = float2{s1, s2};
  }
}

template <typename T, int C>
int launch_c(const void* x, const float* affine, const fd_attn_desc& d, float* qkv, void* out, float* stats, int B, int N, hipStream_t st) {
  hipLaunchKernelGGL((attn_qkv_kernel<T, C>), dim3(fd_cdiv(N, QT), 3, B), dim3(256), 0, st, (const T*)x, affine, d.w_qkv, d.b_qkv, qkv, N);
  FD_LAUNCH_CHECK();
  const float scale = (float)(1.0 / sqrt((double)C));
  hipLaunchKernelGGL((attn_core_kernel<T, C>), dim3(fd_cdiv(N, QT), B), dim3(256), 0, st, (const float*)qkv, (const T*)x, d.w_out, d.b_out, (T*)out,
                     stats, N, scale);
  FD_LAUNCH_CHECK();
  return FD_OK;
}

template <typename T>
int launch_t(const void* x, const float* affine, const fd_attn_desc& d, float* qkv, void* out, float* stats, int B, int N, hipStream_t st) {
  switch (d.C) {
    case 16: return launch_c<T, 16>(x, affine, d, qkv, out, stats, B, N, st);
    case 32: return launch_c<T, 32>(x, affine, d, qkv, out, stats, B, N, st);
    case 64: return launch_c<T, 64>(x, affine, d, qkv, out, stats, B, N, st);
    case 128: return launch_c<T, 128>(x, affine, d, qkv, out, stats, B, N, st);
    case 256: return launch_c<T, 256>(x, affine, d, qkv, out, stats, B, N, st);
  }
  return fd_set_error(FD_EINVAL, "attention block: C must be a power of two in [16, 256] (got %d)", d.C);
}

int check_attn(const fd_attn_desc* d, int B, int H, int W, int dtype) {
  FD_REQUIRE(d, "fd_attn_block: null descriptor");
  FD_REQUIRE(d->C >= 16 && d->C <= 256 && (d->C & (d->C - 1)) == 0, "fd_attn_block: C must be a power of two in [16, 256] (got %d)", d->C);
  FD_REQUIRE(B > 0 && H > 0 && W > 0, "fd_attn_block: bad shape");
  FD_REQUIRE(dtype == FD_BF16 || dtype == FD_F32, "fd_attn_block: bad dtype");
  return FD_OK;
}

}  // namespace

size_t fd_attn_qkv_bytes(int B, int N, int C) { return fd_align(sizeof(float) * 3 * (size_t)B * N * C); }
int fd_attn_stats_tiles(int H, int W) { return fd_cdiv((long long)H * W, QT); }

int fd_attn_launch(const void* x, const float* affine, const fd_attn_desc& d, float* qkv, void* out, float* stats, int B, int N, int dtype,
                   hipStream_t st) {
  return dtype == FD_BF16 ? launch_t<bf16>(x, affine, d, qkv, out, stats, B, N, st) : launch_t<float>(x, affine, d, qkv, out, stats, B, N, st);
}

// stand-alone call: [GroupNorm partials of x][affine][q|k|v] in the workspace
extern "C" size_t fd_attn_block_workspace_bytes(const fd_attn_desc* d, int B, int H, int W, int dtype) {
  if (check_attn(d, B, H, W, dtype) != FD_OK) return 0;
  const size_t part = fd_align(sizeof(float) * 2 * (size_t)B * fd_channel_sums_tiles(H, W) * d->C);
  const size_t aff = fd_align(sizeof(float) * 2 * (size_t)B * d->C);
  return part + aff + fd_attn_qkv_bytes(B, H * W, d->C);
}

extern "C" int fd_attn_block(const fd_attn_desc* d, const void* x, void* out, float* stats, int B, int H, int W, int dtype, void* ws, size_t ws_bytes,
                             void* stream) {
  FD_TRY(check_attn(d, B, H, W, dtype));
  FD_REQUIRE(x && out && ws, "fd_attn_block: null pointer");
  FD_REQUIRE(d->gn_gamma && d->gn_beta && d->w_qkv && d->b_qkv && d->w_out && d->b_out, "fd_attn_block: incomplete descriptor");
  const size_t need = fd_attn_block_workspace_bytes(d, B, H, W, dtype);
  if (ws_bytes < need) return fd_set_error(FD_ENOMEM, "fd_attn_block: workspace %zu < required %zu bytes", ws_bytes, need);
  const int C = d->C, tiles = fd_channel_sums_tiles(H, W);
  float* part = (float*)ws;
  float* aff = (float*)((char*)ws + fd_align(sizeof(float) * 2 * (size_t)B * tiles * C));
  float* qkv = (float*)((char*)aff + fd_align(sizeof(float) * 2 * (size_t)B * C));
  FD_TRY(fd_channel_sums(x, part, B, H, W, C, dtype, stream));
  FD_TRY(fd_gn_finalize(part, tiles, C, C, nullptr, 0, 0, 0, d->gn_gamma, d->gn_beta, aff, B, C / 4 < 32 ? C / 4 : 32, (long long)H * W, 1e-6f, stream));
  return fd_attn_launch(x, aff, *d, qkv, out, stats, B, H * W, dtype, fd_stream(stream));
}
