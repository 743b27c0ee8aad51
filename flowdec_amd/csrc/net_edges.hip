// net_edges.hip -- what the NCSN++ vector field does around its U-Net: the time conditioning (Gaussian Fourier features + 2 Linear,
// ncsnpp.py:263-274, layerspp.py:42-51; the per-ResnetBlock Dense_0 bias, layerspp.py:272-273), the kernels on the 4-channel tensors at
// the edges of the network (input packing ncsnpp.py:401-404, the input convolution ncsnpp.py:291, the 'sum' combine layerspp.py:54-69),
// and the output layer (1x1 or 3x3, 4 -> 2; ncsnpp.py:100,398,407-411) fused with the solvers' state updates (the ODE steps; the
// predictor / corrector of the ScoreDec sampler, sampling/predictors.py:48-71, correctors.py:52-66).  The five edge ops are launched
// through fd_edge_* (internal.h), one function per op.
#include "common.h"
#include "internal.h"
#include "noise.h"

namespace {

// =====================================================================================================
// Time embedding (ncsnpp.py:263-274, layerspp.py:42-51) -- one block per t row.
// =====================================================================================================
// acc = init + sum_k w[k] * x[k], k ascending (one fma per term: the order the parity tests pin), n % 4 == 0 and w 16-byte aligned (the
// public entry points refuse anything else: fd_check_time_embedding / fd_check_temb_bias, ops_api.hip).  The weight row is read
// as 16-byte vectors with 16 of them in flight: these matrix-vector products are one dependent chain per thread and sit on the
// critical path of every network evaluation.
__device__ __forceinline__ float fd_row_dot(const float* __restrict__ w, const float* x, int n, float init) {
  float acc = init;
  for (int k0 = 0; k0 < n; k0 += 64) {
    f32x4 wv[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) wv[j] = (k0 + 4 * j < n) ? *reinterpret_cast<const f32x4*>(w + k0 + 4 * j) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (k0 + 4 * j < n) {
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = fmaf(wv[j][e], x[k0 + 4 * j + e], acc);
      }
  }
  return acc;
}

__global__ __launch_bounds__(256) void time_embedding_kernel(const float* __restrict__ t, float t_imm, const float* __restrict__ W,
                                                             int nf, const float* __restrict__ w1, const float* __restrict__ b1,
                                                             const float* __restrict__ w2, const float* __restrict__ b2,
                                                             float* __restrict__ temb) {
  extern __shared__ float sm[];
  float* emb = sm;            // [2nf]
  float* hid = sm + 2 * nf;   // [4nf]
  const int r = blockIdx.x;
  const float tv = t ? t[r] : t_imm;
  for (int j = threadIdx.x; j < nf; j += blockDim.x) {
    const float xp = ((tv * W[j]) * 2.0f) * 3.14159274101257324f;  // x[:,None]*W[None,:]*2*np.pi in float32
    emb[j] = sinf(xp);
    emb[nf + j] = cosf(xp);
  }
  __syncthreads();
  const int E = 2 * nf, D = 4 * nf;
  for (int o = threadIdx.x; o < D; o += blockDim.x) {
    hid[o] = fd_silu(fd_row_dot(w1 + (size_t)o * E, emb, E, b1[o]));
  }
  __syncthreads();
  for (int o = threadIdx.x; o < D; o += blockDim.x) {
    temb[(size_t)r * D + o] = fd_row_dot(w2 + (size_t)o * D, hid, D, b2[o]);
  }
}

// out[r][o] = cb[o] + db[o] + sum_k dw[o][k] * silu(temb[r][k]); one job per ResnetBlock (layerspp.py:272-273)
__global__ __launch_bounds__(256) void temb_bias_kernel(const fd_temb_job* __restrict__ jobs, const float* __restrict__ temb,
                                                        int temb_dim) {
  extern __shared__ float st[];  // silu(temb[r])
  const fd_temb_job job = jobs[blockIdx.x];
  const int r = blockIdx.y;
  for (int k = threadIdx.x; k < temb_dim; k += blockDim.x) st[k] = fd_silu(temb[(size_t)r * temb_dim + k]);
  __syncthreads();
  for (int o = threadIdx.x; o < job.Cout; o += blockDim.x) {
    job.out[(size_t)r * job.Cout + o] = fd_row_dot(job.dense_w + (size_t)o * temb_dim, st, temb_dim, job.dense_b[o]) + job.conv_b[o];
  }
}

__global__ __launch_bounds__(256) void temb_bias_single_kernel(fd_temb_job job, const float* __restrict__ temb, int temb_dim) {
  extern __shared__ float st[];
  const int r = blockIdx.x;
  for (int k = threadIdx.x; k < temb_dim; k += blockDim.x) st[k] = fd_silu(temb[(size_t)r * temb_dim + k]);
  __syncthreads();
  for (int o = threadIdx.x; o < job.Cout; o += blockDim.x) {
    job.out[(size_t)r * job.Cout + o] = fd_row_dot(job.dense_w + (size_t)o * temb_dim, st, temb_dim, job.dense_b[o]) + (job.conv_b ? job.conv_b[o] : 0.f);
  }
}

// =====================================================================================================
// Edge-of-network kernels on the 4-channel tensors
// =====================================================================================================
// cat(x.re, x.im, y.re, y.im) (ncsnpp.py:401-404) -> NHWC [B][F][T][8]; channels 4..7 are zero padding so that the
// tensor (and its FIR-downsampled pyramid) can feed the MFMA conv, whose input channel counts are multiples of 8
template <typename T>
__global__ void pack_input_kernel(const float2* __restrict__ x, const float2* __restrict__ y, T* __restrict__ out, long long n) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const float2 a = x[i], b = y[i];
    const float v[8] = {a.x, a.y, b.x, b.y, 0.f, 0.f, 0.f, 0.f};
    fd_store_vec<T, 8>(out + 8 * i, v);
  }
}

// The input convolution all_modules.3 (conv3x3, 4 -> nf; ncsnpp.py:291, layers.py:128-134) with the GroupNorm partial sums of its output.
// On the matrix cores this layer is all prologue and epilogue (K = 4 padded channels x 9 taps: 237 us at 8 x 768 x 256 for a launch that
// writes 201 MB); here it is f32 vector FMAs next to the stores: one block = a 16 x 16 pixel tile, one thread = 8 couts x NG = Cout / 8
// consecutive pixels of a tile row, taps ascending, input channels ascending, one fma each (deterministic; statistics of the f32 values,
// fixed reduction order).  Input = the packed NHWC tensor of pack_input_kernel (4 real channels of 8), zero padding.
typedef float f32x2e __attribute__((ext_vector_type(2)));
typedef float f32x4e __attribute__((ext_vector_type(4)));
template <typename T, int NG>
__global__ __launch_bounds__(256) void conv_in_kernel(const T* __restrict__ in8, const float* __restrict__ w, const float* __restrict__ bias,
                                                      T* __restrict__ out, float* __restrict__ part, int H, int W) {
  constexpr int C = 8 * NG;
  constexpr int WBLK = 9;                         // f32x4 per (tap, cout group): 4 channels x 2 cout halves + 1 pad (bank spread)
  __shared__ f32x4e halo[18][18];
  __shared__ f32x4e wl[9 * NG * WBLK];
  __shared__ float red[4][C][2];
  const int t = threadIdx.x, tile = blockIdx.x, b = blockIdx.y;
  const int tiles_w = W >> 4;
  const int h0 = (tile / tiles_w) << 4, w0 = (tile % tiles_w) << 4;
  for (int i = t; i < 18 * 18; i += 256) {
    const int hr = i / 18, hc = i - hr * 18;
    const int gh = h0 - 1 + hr, gw = w0 - 1 + hc;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (gh >= 0 && gh < H && gw >= 0 && gw < W) fd_load_vec<T, 4>(in8 + (((size_t)b * H + gh) * W + gw) * 8, v);
    halo[hr][hc] = f32x4e{v[0], v[1], v[2], v[3]};
  }
  for (int e = t; e < C * 36; e += 256) {         // w: [Cout][4][3][3]
    const int co = e / 36, r = e - co * 36, ci = r / 9, tap = r - ci * 9;
    reinterpret_cast<float*>(wl)[(((tap * NG + (co >> 3)) * WBLK + ci * 2 + ((co & 7) >> 2)) << 2) + (co & 3)] = w[e];
  }
  __syncthreads();
  const int cg = t % NG, slot = t / NG;
  const int p0 = slot * NG, r = p0 >> 4, c0 = p0 & 15;
  f32x2e acc[NG][4];
#pragma unroll
  for (int p = 0; p < NG; ++p)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[p][j] = f32x2e{bias[cg * 8 + 2 * j], bias[cg * 8 + 2 * j + 1]};
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const int dy = tap / 3, dx = tap % 3;
    f32x4e wv[4][2];
#pragma unroll
    for (int ci = 0; ci < 4; ++ci)
#pragma unroll
      for (int h = 0; h < 2; ++h) wv[ci][h] = wl[(tap * NG + cg) * WBLK + ci * 2 + h];
#pragma unroll
    for (int p = 0; p < NG; ++p) {
      const f32x4e x = halo[r + dy][c0 + p + dx];
#pragma unroll
      for (int ci = 0; ci < 4; ++ci) {
        const f32x2e xx = {x[ci], x[ci]};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const f32x2e w2 = {wv[ci][j >> 1][2 * (j & 1)], wv[ci][j >> 1][2 * (j & 1) + 1]};
          acc[p][j] = __builtin_elementwise_fma(xx, w2, acc[p][j]);
        }
      }
    }
  }
  float s1[8], s2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s1[j] = s2[j] = 0.f;
#pragma unroll
  for (int p = 0; p < NG; ++p) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[2 * j] = acc[p][j][0]; v[2 * j + 1] = acc[p][j][1]; }
    fd_store_vec<T, 8>(out + (((size_t)b * H + h0 + r) * W + w0 + c0 + p) * C + cg * 8, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) { s1[j] += v[j]; s2[j] = fmaf(v[j], v[j], s2[j]); }
  }
  // lanes of a wave that share a cout group differ in the slot bits: fold them, then the four waves through LDS
#pragma unroll
  for (int msk = NG; msk < 64; msk <<= 1)
#pragma unroll
    for (int j = 0; j < 8; ++j) { s1[j] += __shfl_xor(s1[j], msk, 64); s2[j] += __shfl_xor(s2[j], msk, 64); }
  if ((t & 63) < NG) {
#pragma unroll
    for (int j = 0; j < 8; ++j) { red[t >> 6][cg * 8 + j][0] = s1[j]; red[t >> 6][cg * 8 + j][1] = s2[j]; }
  }
  __syncthreads();
  if (t < C * 2) {
    const int c = t >> 1, which = t & 1;
    part[(((size_t)b * gridDim.x + tile) * C + c) * 2 + which] = (red[0][c][which] + red[1][c][which]) + (red[2][c][which] + red[3][c][which]);
  }
}

// Combine 'sum' (layerspp.py:54-69): out = conv1x1(p4) + bias + h, fused with the per-tile GroupNorm partial sums of `out`
// (same [b][tile][C][2] format as channel_sums_kernel; the next ResnetBlock's GroupNorm_0 consumes them).  One block =
// COMBINE_PX pixels of one image; one thread = 8 couts of every (256 / (Cout / 8))-th pixel.
constexpr int COMBINE_PX = 256;
template <typename T>
__global__ __launch_bounds__(256) void combine_kernel(const T* __restrict__ p4, const float* __restrict__ w, const float* __restrict__ bias,
                                                      const T* __restrict__ h, T* __restrict__ out, float* __restrict__ part, int HW, int Cout) {
  const int cv = Cout >> 3, lanes = 256 / cv;
  const int t = threadIdx.x, cg = t % cv, pl = t / cv;
  const int b = blockIdx.y;
  const int p0 = blockIdx.x * COMBINE_PX, p1 = min(p0 + COMBINE_PX, HW);
  float wr[8][4], bs[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    bs[i] = bias[cg * 8 + i];
#pragma unroll
    for (int ci = 0; ci < 4; ++ci) wr[i][ci] = w[(size_t)(cg * 8 + i) * 4 + ci];
  }
  float s[8], ss[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) s[i] = ss[i] = 0.f;
  // eight pixels per trip with all loads issued first (the statistics are accumulated in the same pixel order as a plain loop)
  constexpr int UP = 8;
  for (int pb = p0 + pl; pb < p1; pb += UP * lanes) {
    float v[UP][4], hv[UP][8];
#pragma unroll
    for (int u = 0; u < UP; ++u) {
      const int p = pb + u * lanes;
      const size_t pix = (size_t)b * HW + (p < p1 ? p : p0);
      fd_load_vec<T, 4>(p4 + pix * 8, v[u]);   // the 4-channel pyramid is stored with 8-channel stride (see pack_input_kernel)
      fd_load_vec<T, 8>(h + pix * Cout + cg * 8, hv[u]);
    }
#pragma unroll
    for (int u = 0; u < UP; ++u) {
      const int p = pb + u * lanes;
      if (p < p1) {
        const size_t pix = (size_t)b * HW + p;
        float o[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          float acc = bs[i];
#pragma unroll
          for (int ci = 0; ci < 4; ++ci) acc = fmaf(wr[i][ci], v[u][ci], acc);
          o[i] = acc + hv[u][i];
          const float q = (float)(T)o[i];     // statistics of the stored (rounded) tensor, as channel_sums_kernel would see it
          s[i] += q; ss[i] = fmaf(q, q, ss[i]);
        }
        fd_store_vec<T, 8>(out + pix * Cout + cg * 8, o);
      }
    }
  }
  __shared__ float red[256][17];
#pragma unroll
  for (int i = 0; i < 8; ++i) { red[t][i] = s[i]; red[t][8 + i] = ss[i]; }
  __syncthreads();
  for (int o = t; o < 2 * Cout; o += 256) {
    const int c = o >> 1, which = o & 1;
    const int tv = c >> 3, e = (c & 7) + 8 * which;
    float acc = 0.f;
    for (int l = 0; l < lanes; ++l) acc += red[l * cv + tv][e];
    part[(((size_t)b * gridDim.x + blockIdx.x) * Cout + c) * 2 + which] = acc;
  }
}

// The 3x3 output layer (4 -> 2, zero padding 'same', no bias; the SGMSE-style backbone's output_layer_kwargs) at pixel i of the
// [B][H][W] image: f32, taps ascending, input channels ascending per tap.
template <typename T>
__device__ __forceinline__ float2 output3x3(const T* __restrict__ pyr, const float* __restrict__ wo, long long i, int H, int W) {
  const int w = (int)(i % W), h = (int)((i / W) % H);
  float vx = 0.f, vy = 0.f;
#pragma unroll
  for (int dy = 0; dy < 3; ++dy) {
    if (h + dy - 1 < 0 || h + dy - 1 >= H) continue;
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      if (w + dx - 1 < 0 || w + dx - 1 >= W) continue;
      float p[4];
      fd_load_vec<T, 4>(pyr + 4 * (i + (long long)(dy - 1) * W + (dx - 1)), p);
#pragma unroll
      for (int ci = 0; ci < 4; ++ci) {
        vx = fmaf(wo[ci * 9 + dy * 3 + dx], p[ci], vx);
        vy = fmaf(wo[36 + ci * 9 + dy * 3 + dx], p[ci], vy);
      }
    }
  }
  return float2{vx, vy};
}

// The eight weights of the 1x1 output layer ([2][4]): a kernel reads them once per thread, before its element loop.
struct out_w1x1 {
  float w0, w1, w2, w3, w4, w5, w6, w7;
  __device__ __forceinline__ explicit out_w1x1(const float* __restrict__ wo)
      : w0(wo[0]), w1(wo[1]), w2(wo[2]), w3(wo[3]), w4(wo[4]), w5(wo[5]), w6(wo[6]), w7(wo[7]) {}
};

// output_layer (1x1, 4 -> 2, no bias; ncsnpp.py:100,398 -- or 3x3, KS = 3) + view_as_complex (:407-411) at element i of the [B][H][W]
// image.  The one body of the three fused updates below: what they compute from it differs, the layer's bits do not.
template <typename T, int KS>
__device__ __forceinline__ float2 output_layer(const T* __restrict__ pyr, const float* __restrict__ wo, const out_w1x1& k, long long i, int H, int W) {
  if constexpr (KS == 3) {
    return output3x3<T>(pyr, wo, i, H, W);
  } else {
    float p[4];
    fd_load_vec<T, 4>(pyr + 4 * i, p);
    float2 v;
    v.x = fmaf(k.w3, p[3], fmaf(k.w2, p[2], fmaf(k.w1, p[1], k.w0 * p[0])));
    v.y = fmaf(k.w7, p[3], fmaf(k.w6, p[2], fmaf(k.w5, p[1], k.w4 * p[0])));
    return v;
  }
}

// cb * base[i] + cn * v, then + cy * Y[i] unless cy == 0 (Y is not read then): the part of the score-sampler update that the scalar and
// the per-clip kernel share
__device__ __forceinline__ float2 score_combine(float2 v, const float2* __restrict__ base, float cb, const float2* __restrict__ Y, float cy, float cn,
                                                long long i) {
  const float2 b = base[i];
  float2 o = {fmaf(cn, v.x, cb * b.x), fmaf(cn, v.y, cb * b.y)};
  if (cy != 0.f) { const float2 yv = Y[i]; o.x = fmaf(cy, yv.x, o.x); o.y = fmaf(cy, yv.y, o.y); }
  return o;
}

// The output layer fused with the solver's state update:  dst = base + coef * (v + k_old);  optionally k_save = v.
template <typename T, int KS>
__global__ void output_update_kernel(const T* __restrict__ pyr, const float* __restrict__ wo, const float2* __restrict__ base,
                                     const float2* __restrict__ kold, float coef, float2* __restrict__ dst,
                                     float2* __restrict__ ksave, long long n, int H, int W) {
  const out_w1x1 k1(wo);
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const float2 v = output_layer<T, KS>(pyr, wo, k1, i, H, W);
    if (ksave) ksave[i] = v;
    float2 s = v;
    if (kold) { const float2 k = kold[i]; s.x += k.x; s.y += k.y; }
    float2 o = {coef * s.x, coef * s.y};
    if (base) { const float2 bb = base[i]; o.x += bb.x; o.y += bb.y; }
    dst[i] = o;
  }
}

// Predictor / corrector update of the ScoreDec sampler (sampling/predictors.py:48-71, correctors.py:52-66) fused with the
// output layer:  dst = cb * base + cy * Y + cn * v + cz * z   (v = output_layer(pyr) as complex; every coefficient is a
// real scalar that the host derives from the OUVE closed forms, sdes.py:168-192).  SEEDED: z comes from the clips' seeds (draw index
// `draw`) instead of a buffer, at the absolute frames frame0[b] + t (frame0: int32 [B], may be null = zeros; noise.h), and is not
// generated at all when cz == 0: then neither seeds nor frame0 is read.  AT = false: frame0 is not looked at (the instantiation of the entry
// points that have none: the code it was before frame0 existed).
template <typename T, int KS, bool SEEDED, bool AT>
__global__ void score_update_kernel(const T* __restrict__ pyr, const float* __restrict__ wo, const float2* __restrict__ base, float cb,
                                    const float2* __restrict__ Y, float cy, float cn, const float2* __restrict__ z,
                                    const unsigned long long* __restrict__ seeds, const int* __restrict__ frame0, int draw, float cz,
                                    float2* __restrict__ dst, long long n, int H, int W) {
  const out_w1x1 k1(wo);
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const float2 v = output_layer<T, KS>(pyr, wo, k1, i, H, W);
    float2 o = score_combine(v, base, cb, Y, cy, cn, i);
    if (cz != 0.f) { const float2 zv = noise_elem<SEEDED>(z, seeds, draw, i, H, W, AT ? frame0 : nullptr); o.x = fmaf(cz, zv.x, o.x); o.y = fmaf(cz, zv.y, o.y); }
    dst[i] = o;
  }
}

// score_update_kernel with one time per clip and without the noise term (the right-hand side of the ScoreDec ODE sampler under per-clip
// step control):  dst[b] = cb_b * base[b] + cy_b * Y[b] + cn_b * v[b],  (cb_b, cy_b, cn_b) = ctab[b][0..2].  The clip is blockIdx.y, so the
// three coefficients are one wave-uniform load per block and no element divides by the clip size; a block walks its clip's H * W elements
// with the scalar kernel's one element per thread (consecutive lanes, consecutive 8 / 16-byte vectors).  Per element the arithmetic is
// score_update_kernel's -- output_layer and score_combine, the same skip at cy == 0 --, so clip b equals that kernel on the clip alone, bit for bit.
template <typename T, int KS>
__global__ void score_update_clips_kernel(const T* __restrict__ pyr, const float* __restrict__ wo, const float2* __restrict__ base,
                                          const float2* __restrict__ Y, const float* __restrict__ ctab, float2* __restrict__ dst, long long nclip,
                                          int H, int W) {
  const out_w1x1 k1(wo);
  const float cb = ctab[3 * blockIdx.y], cy = ctab[3 * blockIdx.y + 1], cn = ctab[3 * blockIdx.y + 2];
  const long long first = (long long)blockIdx.y * nclip;
  for (long long j = blockIdx.x * (long long)blockDim.x + threadIdx.x; j < nclip; j += (long long)gridDim.x * blockDim.x) {
    const long long i = first + j;
    dst[i] = score_combine(output_layer<T, KS>(pyr, wo, k1, i, H, W), base, cb, Y, cy, cn, i);
  }
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------
// C ABI + internal launchers
// ---------------------------------------------------------------------------------------------------------
int fd_time_embedding_impl(const float* t, float t_imm, int nt, const float* gfp_w, int nf, const float* w1, const float* b1,
                           const float* w2, const float* b2, float* temb, hipStream_t st) {
  hipLaunchKernelGGL(time_embedding_kernel, dim3(nt), dim3(256), sizeof(float) * 6 * nf, st, t, t_imm, gfp_w, nf, w1, b1, w2, b2, temb);
  FD_LAUNCH_CHECK();
  return FD_OK;
}

extern "C" int fd_time_embedding(const float* t, int nt, const float* gfp_w, int nf, const float* w1, const float* b1,
                                 const float* w2, const float* b2, float* temb, void* stream) {
  FD_REQUIRE(t, "fd_time_embedding: null pointer (t)");
  FD_TRY(fd_check_time_embedding("fd_time_embedding", nt, gfp_w, nf, w1, b1, w2, b2, temb));
  return fd_time_embedding_impl(t, 0.f, nt, gfp_w, nf, w1, b1, w2, b2, temb, fd_stream(stream));
}

int fd_temb_bias_batched(const fd_temb_job* jobs_dev, int njobs, const float* temb, int nt, int temb_dim, hipStream_t st) {
  hipLaunchKernelGGL(temb_bias_kernel, dim3(njobs, nt), dim3(256), sizeof(float) * temb_dim, st, jobs_dev, temb, temb_dim);
  FD_LAUNCH_CHECK();
  return FD_OK;
}

extern "C" int fd_temb_bias(const float* temb, int nt, int temb_dim, const float* dense_w, const float* dense_b,
                            const float* conv_bias, int Cout, float* out, void* stream) {
  FD_TRY(fd_check_temb_bias("fd_temb_bias", temb, nt, temb_dim));
  FD_TRY(fd_check_temb_job("fd_temb_bias", -1, dense_w, dense_b, out, Cout));
  fd_temb_job j{dense_w, dense_b, conv_bias, out, Cout};
  hipLaunchKernelGGL(temb_bias_single_kernel, dim3(nt), dim3(256), sizeof(float) * temb_dim, fd_stream(stream), j, temb, temb_dim);
  FD_LAUNCH_CHECK();
  return FD_OK;
}

// ---- the edge ops: fd_edge_<op>(a, dtype, st) holds the op's precondition and its launch (launch_<op><T> where the kernel has more template parameters) ----
int fd_combine_tiles(int H, int W) { return fd_cdiv((long long)H * W, COMBINE_PX); }

int fd_edge_pack_input(const fd_edge_args& a, int dtype, hipStream_t st) {
  const long long n = (long long)a.B * a.H * a.W;
  const dim3 grid(grid_for(n, 256, 8192));
  if (dtype == FD_BF16) hipLaunchKernelGGL(pack_input_kernel<bf16>, grid, dim3(256), 0, st, (const float2*)a.x, (const float2*)a.y, (bf16*)a.out, n);
  else hipLaunchKernelGGL(pack_input_kernel<float>, grid, dim3(256), 0, st, (const float2*)a.x, (const float2*)a.y, (float*)a.out, n);
  FD_LAUNCH_CHECK();
  return FD_OK;
}

int fd_edge_combine(const fd_edge_args& a, int dtype, hipStream_t st) {
  FD_REQUIRE(a.stats && a.Cout >= 8 && a.Cout <= 256 && (a.Cout & (a.Cout - 1)) == 0, "edge op: combine needs a stats buffer and a power-of-two Cout in [8, 256]");
  const dim3 grid(fd_combine_tiles(a.H, a.W), a.B);
  if (dtype == FD_BF16) hipLaunchKernelGGL(combine_kernel<bf16>, grid, dim3(256), 0, st, (const bf16*)a.x, a.w, a.bias, (const bf16*)a.y, (bf16*)a.out, a.stats, a.H * a.W, a.Cout);
  else hipLaunchKernelGGL(combine_kernel<float>, grid, dim3(256), 0, st, (const float*)a.x, a.w, a.bias, (const float*)a.y, (float*)a.out, a.stats, a.H * a.W, a.Cout);
  FD_LAUNCH_CHECK();
  return FD_OK;
}

template <typename T>
static int launch_output_update(const fd_edge_args& a, hipStream_t st) {
  const long long n = (long long)a.B * a.H * a.W;
  if (a.ks == 3)
    hipLaunchKernelGGL((output_update_kernel<T, 3>), dim3(grid_for(n, 256, 8192)), dim3(256), 0, st, (const T*)a.x, a.w, (const float2*)a.base, (const float2*)a.kold, a.coef, (float2*)a.out, (float2*)a.ksave, n, a.H, a.W);
  else
    hipLaunchKernelGGL((output_update_kernel<T, 1>), dim3(grid_for(n, 256, 8192)), dim3(256), 0, st, (const T*)a.x, a.w, (const float2*)a.base, (const float2*)a.kold, a.coef, (float2*)a.out, (float2*)a.ksave, n, a.H, a.W);
  FD_LAUNCH_CHECK();
  return FD_OK;
}
int fd_edge_output_update(const fd_edge_args& a, int dtype, hipStream_t st) {
  return dtype == FD_BF16 ? launch_output_update<bf16>(a, st) : launch_output_update<float>(a, st);
}

template <typename T>
static int launch_score_update(const fd_edge_args& a, hipStream_t st) {
  const long long n = (long long)a.B * a.H * a.W;
  if (a.ctab) {   // one time per clip: the clip is the grid's y
    const long long nclip = (long long)a.H * a.W;
    const dim3 grid(grid_for(nclip, 256, 8192), a.B);
    if (a.ks == 3)
      hipLaunchKernelGGL((score_update_clips_kernel<T, 3>), grid, dim3(256), 0, st, (const T*)a.x, a.w, (const float2*)a.base, (const float2*)a.y, a.ctab, (float2*)a.out, nclip, a.H, a.W);
    else
      hipLaunchKernelGGL((score_update_clips_kernel<T, 1>), grid, dim3(256), 0, st, (const T*)a.x, a.w, (const float2*)a.base, (const float2*)a.y, a.ctab, (float2*)a.out, nclip, a.H, a.W);
  } else {
#define FD_SCORE_UPDATE(KS_, SEEDED_, AT_)                                                                                                       \
  hipLaunchKernelGGL((score_update_kernel<T, KS_, SEEDED_, AT_>), dim3(grid_for(n, 256, 8192)), dim3(256), 0, st, (const T*)a.x, a.w, (const float2*)a.base, \
                     a.cb, (const float2*)a.y, a.cy, a.coef, (const float2*)a.z.ptr, a.z.seeds, a.z.frame0, a.z.draw, a.cz, (float2*)a.out, n, a.H, a.W)
    if (a.z.seeds && a.z.frame0) { if (a.ks == 3) FD_SCORE_UPDATE(3, true, true); else FD_SCORE_UPDATE(1, true, true); }
    else if (a.z.seeds) { if (a.ks == 3) FD_SCORE_UPDATE(3, true, false); else FD_SCORE_UPDATE(1, true, false); }
    else { if (a.ks == 3) FD_SCORE_UPDATE(3, false, false); else FD_SCORE_UPDATE(1, false, false); }
#undef FD_SCORE_UPDATE
  }
  FD_LAUNCH_CHECK();
  return FD_OK;
}
int fd_edge_score_update(const fd_edge_args& a, int dtype, hipStream_t st) {
  return dtype == FD_BF16 ? launch_score_update<bf16>(a, st) : launch_score_update<float>(a, st);
}

template <typename T>
static int launch_conv_in(const fd_edge_args& a, hipStream_t st) {
  const dim3 grid((a.H >> 4) * (a.W >> 4), a.B);
#define FD_CONV_IN(NG_) hipLaunchKernelGGL((conv_in_kernel<T, NG_>), grid, dim3(256), 0, st, (const T*)a.x, a.w, a.bias, (T*)a.out, a.stats, a.H, a.W)
  switch (a.Cout) {
    case 8: FD_CONV_IN(1); break;
    case 16: FD_CONV_IN(2); break;
    case 32: FD_CONV_IN(4); break;
    case 64: FD_CONV_IN(8); break;
    case 128: FD_CONV_IN(16); break;
    default: return fd_set_error(FD_EINVAL, "edge_launch: conv_in needs Cout in {8, 16, 32, 64, 128}");
  }
#undef FD_CONV_IN
  FD_LAUNCH_CHECK();
  return FD_OK;
}
int fd_edge_conv_in(const fd_edge_args& a, int dtype, hipStream_t st) {
  FD_REQUIRE(a.x && a.w && a.bias && a.out && a.stats && a.H % 16 == 0 && a.W % 16 == 0, "edge op: conv_in needs whole 16 x 16 tiles, weights, bias and a stats buffer");
  return dtype == FD_BF16 ? launch_conv_in<bf16>(a, st) : launch_conv_in<float>(a, st);
}

extern "C" int fd_conv_in(const void* in8, const float* w, const float* bias, void* out, float* stats, int B, int H, int W, int Cout, int dtype,
                          void* stream) {
  FD_REQUIRE(dtype == FD_BF16 || dtype == FD_F32, "fd_conv_in: dtype must be FD_BF16 or FD_F32");
  FD_REQUIRE(B > 0 && H > 0 && W > 0, "fd_conv_in: bad shape");
  fd_edge_args a;
  a.x = in8; a.w = w; a.bias = bias; a.out = out; a.stats = stats; a.B = B; a.H = H; a.W = W; a.Cout = Cout;
  return fd_edge_conv_in(a, dtype, fd_stream(stream));
}
