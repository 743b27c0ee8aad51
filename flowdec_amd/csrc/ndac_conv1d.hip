// ndac_conv1d.hip -- the codec's direct 1-D convolutions: the EXACT path, f32 on the vector ALUs in a defined operation order per output
// (input channels ascending, taps ascending, one fma each; every convolution kernel below produces the same bits), which is what makes the
// encoder's code indices reproducible.  Layout [B][C][T] float32 (the reference's Conv1d layout).  Kernels:
//   conv1d_kernel       LDS-tiled dilated / strided 1-D convolution, 128 outputs x 32 channels per workgroup; optional Snake of the INPUT
//                       while the tile is staged (operator-level ABI), bias / residual add (ResidualUnit: x + block(x)) / tanh and the
//                       NEXT layer's Snake (second output) in the epilogue
//   conv1d_s1_kernel    the stride-1 layers (K = 7 dilation 1 / 3 / 9, K = 1, K = 3): register windows of 4 consecutive outputs
//   conv1d_ci1_kernel / conv1d_co1_kernel   the one-channel ends of the codec (audio -> d channels, d channels -> audio)
//   convtr1d_kernel     transposed convolution as a gather: output n takes taps k = (n + p) mod s, + s, ... of inputs (n + p - k) / s
// Ragged calls: every kernel reads input positions at and behind T as the zero padding; under a frame table (fd_ndac_lens) that bound is the
// CLIP's own length at the layer, so a clip in a batch of longer rows sees exactly the padding it sees alone -- the same bits -- and
// nothing behind it is read as data.  No table (every dense call): the bound is T.
#include <math.h>

#include "ndac_internal.h"

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));
constexpr int TT = 128;   // output positions per workgroup
constexpr int CT = 32;    // output channels per workgroup
constexpr int CIC = 8;    // input channels per LDS chunk
constexpr int CTP = CT + 4;   // padded weight row of the transposed convolution

__device__ __forceinline__ float snake_f(float x, float alpha) {
  // x + (alpha + 1e-9)^-1 sin^2(alpha x)   (dac/nn/layers.py `snake`); IEEE division, sinf at full precision
  const float s = sinf(alpha * x);
  return x + (1.0f / (alpha + 1e-9f)) * (s * s);
}

struct Conv1dArgs {
  const float* x; const float* w; const float* bias; const float* alpha; const float* res; float* out;
  float* out_act; const float* alpha_out;   // optional second output: snake(result, alpha_out[co]) -- the NEXT layer's activated input,
                                            // computed once by the producer instead of once per consuming workgroup (24x at 768 channels)
  int B, Ci, T, Co, K, To, stride, pad, dil, tanh_out;
  int wt;   // weight layout: 0 = [Co][Ci][K] (nn.Conv1d, the operator-level ABI), 1 = [Ci][K][Co] (the codec's own copy: coalesced staging)
  fd_ndac_lens lens;   // ragged decode: clip b is lens.frames[b] * lens.mul + lens.add positions long (T stays the row pitch); null = T
};

// The clip's own input length: positions at and behind it read as the zero padding, whatever the row holds there.
template <typename Args>
__device__ __forceinline__ int clip_len(const Args& a, int b) { return a.lens.frames ? a.lens.frames[b] * a.lens.mul + a.lens.add : a.T; }

// weights are read as [Co][Ci][K] (PyTorch layout) and staged as [ci][k][co] so that a thread's 4 output channels are one b128 read
__global__ __launch_bounds__(256) void conv1d_kernel(Conv1dArgs a) {
  extern __shared__ float sm[];
  const int span = (TT - 1) * a.stride + (a.K - 1) * a.dil + 1;
  float* xs = sm;                         // [CIC][span]
  float* ws = sm + CIC * span;            // [CIC][K][CT]
  const int b = blockIdx.z, co0 = blockIdx.y * CT, t0 = blockIdx.x * TT;
  const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;   // thread: outputs t0 + tx + 32 j (j < 4) x channels co0 + 4 ty .. + 3
  f32x2 acc[4][2];   // [output j][channel pair]: v_pk_fma_f32, two channels per instruction (the same IEEE fma per element)
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j][0] = acc[j][1] = f32x2{0.f, 0.f};
  const long long in0 = (long long)t0 * a.stride - a.pad;   // input position of xs[.][0]
  const int Tb = clip_len(a, b);
  for (int c0 = 0; c0 < a.Ci; c0 += CIC) {
    __syncthreads();
    for (int i = tid; i < CIC * span; i += 256) {
      const int ci = i / span, p = i - ci * span;
      const long long tin = in0 + p;
      float v = 0.f;
      if (c0 + ci < a.Ci && tin >= 0 && tin < Tb) {
        v = a.x[((size_t)b * a.Ci + c0 + ci) * a.T + tin];
        if (a.alpha) v = snake_f(v, a.alpha[c0 + ci]);      // zero padding applies to the ACTIVATED signal (Snake, then Conv1d(padding=..))
      }
      xs[i] = v;
    }
    for (int i = tid; i < CIC * a.K * CT; i += 256) {
      const int co = i % CT, r = i / CT, k = r % a.K, ci = r / a.K;
      ws[i] = (c0 + ci < a.Ci && co0 + co < a.Co) ? a.w[a.wt ? ((size_t)(c0 + ci) * a.K + k) * a.Co + co0 + co : ((size_t)(co0 + co) * a.Ci + c0 + ci) * a.K + k] : 0.f;
    }
    __syncthreads();
#pragma unroll 1
    for (int ci = 0; ci < CIC; ++ci) {
      const float* xr = xs + ci * span + tx * a.stride;
      const float* wr = ws + ci * a.K * CT + ty * 4;
      for (int k = 0; k < a.K; ++k) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(wr + k * CT);
        const f32x2 w01 = {wv[0], wv[1]}, w23 = {wv[2], wv[3]};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float xv = xr[32 * j * a.stride + k * a.dil];
          const f32x2 x2 = {xv, xv};
          acc[j][0] = __builtin_elementwise_fma(x2, w01, acc[j][0]);
          acc[j][1] = __builtin_elementwise_fma(x2, w23, acc[j][1]);
        }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int co = co0 + ty * 4 + c;
    if (co >= a.Co) continue;
    const float bv = a.bias ? a.bias[co] : 0.f;
    const float ao = a.out_act ? a.alpha_out[co] : 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int t = t0 + tx + 32 * j;
      if (t >= a.To) continue;
      const size_t o = ((size_t)b * a.Co + co) * a.To + t;
      float v = acc[j][c >> 1][c & 1] + bv;
      if (a.res) v += a.res[o];
      if (a.tanh_out) v = tanhf(v);
      if (a.out) a.out[o] = v;
      if (a.out_act) a.out_act[o] = snake_f(v, ao);
    }
  }
}

// Stride-1 convolutions with a compile-time tap count and dilation (every ResidualUnit conv: K = 7 with dilation 1 / 3, K = 1; the
// K = 3 latent conv): a thread owns two groups of 4 CONSECUTIVE outputs (t0 + 4 tx + {0..3} and 128 further) x 4 channels.  Per input
// channel the 4 + (K - 1) DIL inputs a group needs are read ONCE as aligned ds_read_b128 (lane stride 16 B: conflict-free) into a
// register window and all K taps run out of registers -- 13 wide LDS reads per 224 packed-FMA pairs (K = 7, DIL = 1) where the generic
// kernel above issues one ds_read_b32 per 4 FMAs and is bound by the LDS pipe.  256 outputs x 32 channels per workgroup.
// (8 channels per thread -- 64 per workgroup, twice the FMAs per weight read -- measured SLOWER: encode 26.7 -> 31.1 ms at 146-166
// registers, three waves per SIMD instead of five.)
constexpr int TT1 = 256;
template <int K, int DIL>
__global__ __launch_bounds__(256) void conv1d_s1_kernel(Conv1dArgs a) {
  extern __shared__ float sm[];
  constexpr int HALO = (K - 1) * DIL;
  constexpr int SPAN = (TT1 + HALO + 3) / 4 * 4;     // floats per staged input row (multiple of 4: aligned b128 rows)
  constexpr int NW = (4 + HALO + 3) / 4;             // b128 reads per group window
  float* xs = sm;                                    // [CIC][SPAN]
  float* ws = sm + CIC * SPAN;                       // [CIC][K][CT]
  const int b = blockIdx.z, co0 = blockIdx.y * CT, t0 = blockIdx.x * TT1;
  const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
  f32x2 acc[2][4][2];   // [group][output][channel pair]
#pragma unroll
  for (int g = 0; g < 2; ++g)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[g][i][0] = acc[g][i][1] = f32x2{0.f, 0.f};
  const long long in0 = (long long)t0 - a.pad;
  const int Tb = clip_len(a, b);
  for (int c0 = 0; c0 < a.Ci; c0 += CIC) {
    __syncthreads();
    for (int i = tid; i < CIC * SPAN; i += 256) {
      const int ci = i / SPAN, p = i - ci * SPAN;
      const long long tin = in0 + p;
      float v = 0.f;
      if (c0 + ci < a.Ci && tin >= 0 && tin < Tb) {
        v = a.x[((size_t)b * a.Ci + c0 + ci) * a.T + tin];
        if (a.alpha) v = snake_f(v, a.alpha[c0 + ci]);
      }
      xs[i] = v;
    }
    for (int i = tid; i < CIC * K * CT; i += 256) {
      const int co = i % CT, r = i / CT, k = r % K, ci = r / K;
      ws[i] = (c0 + ci < a.Ci && co0 + co < a.Co) ? a.w[a.wt ? ((size_t)(c0 + ci) * K + k) * a.Co + co0 + co : ((size_t)(co0 + co) * a.Ci + c0 + ci) * K + k] : 0.f;
    }
    __syncthreads();
#pragma unroll 1
    for (int ci = 0; ci < CIC; ++ci) {
      const float* wr = ws + ci * K * CT + ty * 4;
      f32x2 w01[K], w23[K];
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(wr + k * CT);
        w01[k] = f32x2{wv[0], wv[1]}; w23[k] = f32x2{wv[2], wv[3]};
      }
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const float* xr = xs + ci * SPAN + 4 * tx + 128 * g;
        float xw[4 * NW];
#pragma unroll
        for (int m = 0; m < NW; ++m) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(xr + 4 * m);
          xw[4 * m] = v[0]; xw[4 * m + 1] = v[1]; xw[4 * m + 2] = v[2]; xw[4 * m + 3] = v[3];
        }
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const f32x2 x2 = {xw[i + k * DIL], xw[i + k * DIL]};
            acc[g][i][0] = __builtin_elementwise_fma(x2, w01[k], acc[g][i][0]);
            acc[g][i][1] = __builtin_elementwise_fma(x2, w23[k], acc[g][i][1]);
          }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int co = co0 + ty * 4 + c;
    if (co >= a.Co) continue;
    const float bv = a.bias ? a.bias[co] : 0.f;
    const float ao = a.out_act ? a.alpha_out[co] : 0.f;
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int t = t0 + 4 * tx + 128 * g + i;
        if (t >= a.To) continue;
        const size_t o = ((size_t)b * a.Co + co) * a.To + t;
        float v = acc[g][i][c >> 1][c & 1] + bv;
        if (a.res) v += a.res[o];
        if (a.tanh_out) v = tanhf(v);
        if (a.out) a.out[o] = v;
        if (a.out_act) a.out_act[o] = snake_f(v, ao);
      }
  }
}

// The two ends of the codec, where the 32-channel tiles above are 97 % padding: ONE input channel (the encoder's first layer:
// audio -> d channels) and ONE output channel (the decoder's last layer: d channels -> audio, tanh).  Same fma sequence per output
// as conv1d_kernel (input channels ascending, taps ascending, then + bias): identical bits.
__global__ __launch_bounds__(256) void conv1d_ci1_kernel(Conv1dArgs a) {   // Ci == 1, stride 1, K <= 8, no input activation
  const int b = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
  if (t >= a.To) return;
  const int Tb = clip_len(a, b);
  float xv[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const long long tin = (long long)t - a.pad + (long long)k * a.dil;
    xv[k] = k < a.K && tin >= 0 && tin < Tb ? a.x[(size_t)b * a.T + tin] : 0.f;
  }
  for (int co = 0; co < a.Co; ++co) {
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (k < a.K) acc = __builtin_fmaf(xv[k], a.w[a.wt ? k * a.Co + co : co * a.K + k], acc);
    const size_t o = ((size_t)b * a.Co + co) * a.To + t;
    float v = acc + (a.bias ? a.bias[co] : 0.f);
    if (a.res) v += a.res[o];
    if (a.tanh_out) v = tanhf(v);
    if (a.out) a.out[o] = v;
    if (a.out_act) a.out_act[o] = snake_f(v, a.alpha_out[co]);
  }
}

constexpr int C1C = 16;   // input channels per LDS chunk of the one-output-channel kernel
__global__ __launch_bounds__(256) void conv1d_co1_kernel(Conv1dArgs a) {   // Co == 1, stride 1
  extern __shared__ float sm[];
  const int span = 256 + (a.K - 1) * a.dil;
  const int b = blockIdx.y, t0 = blockIdx.x * 256, tid = threadIdx.x;
  const long long in0 = (long long)t0 - a.pad;
  const int Tb = clip_len(a, b);
  float acc = 0.f;
  for (int c0 = 0; c0 < a.Ci; c0 += C1C) {
    __syncthreads();
    for (int i = tid; i < C1C * span; i += 256) {
      const int ci = i / span, p = i - ci * span;
      const long long tin = in0 + p;
      float v = 0.f;
      if (c0 + ci < a.Ci && tin >= 0 && tin < Tb) {
        v = a.x[((size_t)b * a.Ci + c0 + ci) * a.T + tin];
        if (a.alpha) v = snake_f(v, a.alpha[c0 + ci]);
      }
      sm[i] = v;
    }
    __syncthreads();
    const int cn = a.Ci - c0 < C1C ? a.Ci - c0 : C1C;
    for (int ci = 0; ci < cn; ++ci) {
      const float* xr = sm + ci * span + tid;
      const float* wr = a.w + (size_t)(c0 + ci) * a.K;   // [Co = 1][Ci][K] and [Ci][K][Co = 1] are the same array
      for (int k = 0; k < a.K; ++k) acc = __builtin_fmaf(xr[k * a.dil], wr[k], acc);
    }
  }
  const int t = t0 + tid;
  if (t >= a.To) return;
  const size_t o = (size_t)b * a.To + t;
  float v = acc + (a.bias ? a.bias[0] : 0.f);
  if (a.res) v += a.res[o];
  if (a.tanh_out) v = tanhf(v);
  if (a.out) a.out[o] = v;
  if (a.out_act) a.out_act[o] = snake_f(v, a.alpha_out[0]);
}

struct ConvTr1dArgs {
  const float* x; const float* w; const float* bias; const float* alpha; float* out;
  float* out_act; const float* alpha_out;
  int B, Ci, T, Co, K, To, stride, pad;
  int wt;   // 0 = [Ci][Co][K] (nn.ConvTranspose1d), 1 = [Ci][K][Co]
  fd_ndac_lens lens;
};

// out[b][co][n] = bias[co] + sum_ci sum_{k = (n + p) mod s, += s, < K} act(x)[b][ci][(n + p - k) / s] * w[ci][co][k]   (w: [Ci][Co][K])
__global__ __launch_bounds__(256) void convtr1d_kernel(ConvTr1dArgs a) {
  extern __shared__ float sm[];
  const int ntap = (a.K + a.stride - 1) / a.stride;
  const int tspan = TT / a.stride + ntap + 1;
  float* xs = sm;                         // [CIC][tspan]
  float* ws = sm + CIC * tspan;           // [CIC][K][CTP]: rows padded by 16 B -- the tap index k varies per LANE here (k = (n + p) mod s),
                                          // and rows 128 B apart would put the lanes of a b128 group on 2 of its 16 slots
  const int b = blockIdx.z, co0 = blockIdx.y * CT, n0 = blockIdx.x * TT;
  const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
  const int tbase = (n0 + a.pad) / a.stride - (ntap - 1);   // input position of xs[.][0] (may be negative)
  const int Tb = clip_len(a, b);
  float acc[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[j][c] = 0.f;
  int kk0[4], tt0[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int n = n0 + tx + 32 * j;
    kk0[j] = (n + a.pad) % a.stride;
    tt0[j] = (n + a.pad) / a.stride - tbase;   // xs index of the tap k = kk0; tap k + m s reads index tt0 - m
  }
  for (int c0 = 0; c0 < a.Ci; c0 += CIC) {
    __syncthreads();
    for (int i = tid; i < CIC * tspan; i += 256) {
      const int ci = i / tspan, p = i - ci * tspan, tin = tbase + p;
      float v = 0.f;
      if (c0 + ci < a.Ci && tin >= 0 && tin < Tb) {
        v = a.x[((size_t)b * a.Ci + c0 + ci) * a.T + tin];
        if (a.alpha) v = snake_f(v, a.alpha[c0 + ci]);
      }
      xs[i] = v;
    }
    for (int i = tid; i < CIC * a.K * CT; i += 256) {
      const int co = i % CT, r = i / CT, k = r % a.K, ci = r / a.K;
      ws[r * CTP + co] = (c0 + ci < a.Ci && co0 + co < a.Co) ? a.w[a.wt ? ((size_t)(c0 + ci) * a.K + k) * a.Co + co0 + co : ((size_t)(c0 + ci) * a.Co + co0 + co) * a.K + k] : 0.f;
    }
    __syncthreads();
#pragma unroll 1
    for (int ci = 0; ci < CIC; ++ci) {
      const float* xr = xs + ci * tspan;
      const float* wr = ws + ci * a.K * CTP + ty * 4;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        for (int m = 0, k = kk0[j]; k < a.K; ++m, k += a.stride) {
          const float xv = xr[tt0[j] - m];
          const f32x4 wv = *reinterpret_cast<const f32x4*>(wr + k * CTP);
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[j][c] = fmaf(xv, wv[c], acc[j][c]);
        }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int co = co0 + ty * 4 + c;
    if (co >= a.Co) continue;
    const float bv = a.bias ? a.bias[co] : 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = n0 + tx + 32 * j;
      if (n < a.To) {
        const size_t o = ((size_t)b * a.Co + co) * a.To + n;
        const float v = acc[j][c] + bv;
        if (a.out) a.out[o] = v;
        if (a.out_act) a.out_act[o] = snake_f(v, a.alpha_out[co]);
      }
    }
  }
}

size_t conv1d_lds(int K, int stride, int dil) { return sizeof(float) * (size_t)(CIC * ((TT - 1) * stride + (K - 1) * dil + 1) + CIC * K * CT); }
size_t convtr_lds(int K, int stride) { return sizeof(float) * (size_t)(CIC * (TT / stride + (K + stride - 1) / stride + 1) + CIC * K * CTP); }

}  // namespace

int fd_launch_conv1d(const float* x, const float* w, const float* bias, const float* alpha, const float* res, float* out, int B, int Ci, int T, int Co,
                     int K, int stride, int pad, int dil, int tanh_out, hipStream_t st, int wt, float* out_act, const float* alpha_out, fd_ndac_lens lens) {
  FD_REQUIRE(B > 0 && Ci > 0 && T > 0 && Co > 0 && K > 0 && stride > 0 && dil > 0 && pad >= 0, "fd_conv1d: bad shape");
  const long long To = ((long long)T + 2 * pad - (long long)dil * (K - 1) - 1) / stride + 1;
  FD_REQUIRE(To > 0 && To < (1ll << 31), "fd_conv1d: empty output");
  const size_t lds = conv1d_lds(K, stride, dil);
  FD_REQUIRE(lds <= 64 * 1024, "fd_conv1d: kernel %d / stride %d / dilation %d needs %zu bytes of LDS (limit 64 KiB)", K, stride, dil, lds);
  Conv1dArgs a{x, w, bias, alpha, res, out, out_act, alpha_out, B, Ci, T, Co, K, (int)To, stride, pad, dil, tanh_out, wt, lens};
  // the accumulation order per output is the same in both kernels (input channels ascending, taps ascending, one fma each): identical bits
  if (stride == 1 && Ci == 1 && K <= 8 && !alpha) {
    hipLaunchKernelGGL(conv1d_ci1_kernel, dim3(fd_cdiv(To, 256), B), dim3(256), 0, st, a);
    FD_LAUNCH_CHECK();
    return FD_OK;
  }
  if (stride == 1 && Co == 1 && sizeof(float) * C1C * (256 + (size_t)(K - 1) * dil) <= 64 * 1024) {
    hipLaunchKernelGGL(conv1d_co1_kernel, dim3(fd_cdiv(To, 256), B), dim3(256), sizeof(float) * C1C * (256 + (size_t)(K - 1) * dil), st, a);
    FD_LAUNCH_CHECK();
    return FD_OK;
  }
#define FD_CONV1D_S1(K_, D_)                                                                                                                      \
  if (stride == 1 && K == K_ && dil == D_ && Co >= 4) {                                                                                           \
    constexpr size_t lds1 = sizeof(float) * (size_t)(CIC * ((TT1 + (K_ - 1) * D_ + 3) / 4 * 4) + CIC * K_ * CT);                                    \
    hipLaunchKernelGGL((conv1d_s1_kernel<K_, D_>), dim3(fd_cdiv(To, TT1), fd_cdiv(Co, CT), B), dim3(256), lds1, st, a);                            \
    FD_LAUNCH_CHECK();                                                                                                                            \
    return FD_OK;                                                                                                                                 \
  }
  FD_CONV1D_S1(7, 1) FD_CONV1D_S1(7, 3) FD_CONV1D_S1(7, 9) FD_CONV1D_S1(1, 1) FD_CONV1D_S1(3, 1)
#undef FD_CONV1D_S1
  hipLaunchKernelGGL(conv1d_kernel, dim3(fd_cdiv(To, TT), fd_cdiv(Co, CT), B), dim3(256), lds, st, a);
  FD_LAUNCH_CHECK();
  return FD_OK;
}

int fd_launch_convtr1d(const float* x, const float* w, const float* bias, const float* alpha, float* out, int B, int Ci, int T, int Co, int K, int stride,
                       int pad, hipStream_t st, int wt, float* out_act, const float* alpha_out, fd_ndac_lens lens) {
  FD_REQUIRE(B > 0 && Ci > 0 && T > 0 && Co > 0 && K > 0 && stride > 0 && pad >= 0, "fd_conv_transpose1d: bad shape");
  const long long To = ((long long)T - 1) * stride - 2 * pad + K;
  FD_REQUIRE(To > 0 && To < (1ll << 31), "fd_conv_transpose1d: empty output");
  const size_t lds = convtr_lds(K, stride);
  FD_REQUIRE(lds <= 64 * 1024, "fd_conv_transpose1d: kernel %d needs %zu bytes of LDS (limit 64 KiB)", K, lds);
  ConvTr1dArgs a{x, w, bias, alpha, out, out_act, alpha_out, B, Ci, T, Co, K, (int)To, stride, pad, wt, lens};
  hipLaunchKernelGGL(convtr1d_kernel, dim3(fd_cdiv(To, TT), fd_cdiv(Co, CT), B), dim3(256), lds, st, a);
  FD_LAUNCH_CHECK();
  return FD_OK;
}

extern "C" int fd_conv1d(const float* x, const float* w, const float* bias, const float* alpha_in, const float* residual, float* out, int B, int Ci, int T,
                         int Co, int K, int stride, int padding, int dilation, int tanh_out, void* stream) {
  FD_REQUIRE(x && w && out, "fd_conv1d: null pointer");
  return fd_launch_conv1d(x, w, bias, alpha_in, residual, out, B, Ci, T, Co, K, stride, padding, dilation, tanh_out, fd_stream(stream));
}

extern "C" int fd_conv_transpose1d(const float* x, const float* w, const float* bias, const float* alpha_in, float* out, int B, int Ci, int T, int Co, int K,
                                   int stride, int padding, void* stream) {
  FD_REQUIRE(x && w && out, "fd_conv_transpose1d: null pointer");
  return fd_launch_convtr1d(x, w, bias, alpha_in, out, B, Ci, T, Co, K, stride, padding, fd_stream(stream));
}
