// fir.hip -- the resampling of the NCSN++ vector field on NHWC activations: the FIR [1,3,3,1] x2 up / down kernels in polyphase form with
// the fused GroupNorm affine + SiLU second output (upsample_2d / downsample_2d, up_or_down_sampling.py:220-282 via op/upfirdn2d.py), the
// rule that picks one of them for a call (fir_select) and the switch that launches it (launch_fir), and the generic boundary ops
// upfirdn2d (op/upfirdn2d.py:183-224, upfirdn2d_kernel.cu:60-218) and fused_bias_act (fused_bias_act_kernel.cu:30-61).
#include <type_traits>

#include "common.h"

namespace {

// =====================================================================================================
// FIR [1,3,3,1] x2 resampling, polyphase form (up_or_down_sampling.py:220-282 via op/upfirdn2d.py)
//   down: out[n]   = (x[2n-1] + 3 x[2n] + 3 x[2n+1] + x[2n+2]) / 8     per axis, zeros outside
//   up  : out[2i]  = (x[i-1] + 3 x[i]) / 4 ; out[2i+1] = (3 x[i] + x[i+1]) / 4
// One thread = one VEC-channel vector of a strip of N consecutive rows at one column (output rows for down, input rows for
// up).  The filter is applied separably with a register sliding window DOWN the strip: every input row contributes one
// horizontally combined value per thread (3 / 4 neighbouring columns, activated once: silu(a*x+d), zero padding AFTER
// the activation), and the vertical taps run over the last 3 (up) / 4 (down) combined rows.  Per output this is 3x (up) /
// 2x (down) fewer loads and SiLU evaluations than the direct form, and at any moment neighbouring threads read
// neighbouring pixels of the same image row (contiguous HBM traffic).  With `affine`, the second output is the resample
// of the activated input.  N = 1 degenerates to the direct form (used without activation, where loads are all there is).
// =====================================================================================================
// The load is unconditional (the caller clamps the coordinates into the image, so the value is finite) and the zero
// padding is applied by a 0/1 factor: loads inside divergent branches would be waited for one at a time.
template <typename T, int VEC, bool ACT>
__device__ __forceinline__ void fir_load_px(const T* __restrict__ x, size_t base, bool ok, const float (&a)[VEC], const float (&d)[VEC],
                                            float (&r)[VEC], float (&ac)[VEC]) {
  fd_load_vec<T, VEC>(x + base, r);
  const float m = ok ? 1.f : 0.f;   // a multiply, not a select: hipcc turns the select into a divergent branch around the SiLU
#pragma unroll
  for (int i = 0; i < VEC; ++i) {
    ac[i] = ACT ? m * fd_silu(fmaf(r[i], a[i], d[i])) : 0.f;
    r[i] *= m;
  }
}
__device__ __forceinline__ int fir_clamp(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// A pixel's VEC channels as loaded (not yet converted): the marching kernels request the NEXT row before they store the current one.
// Loads and stores return in order on this ISA (one vmcnt counter): a wait for loads issued AFTER a row's stores is a wait for the
// stores' acknowledgement as well -- measured on fir_up: 194 us of loads + arithmetic and 237 us of stores ran back to back (431 us).
template <typename T, int VEC> struct fir_raw;
template <> struct fir_raw<bf16, 8> { bf16x8 v; __device__ void load(const bf16* p) { v = *reinterpret_cast<const bf16x8*>(p); }
  __device__ void get(float (&f)[8]) const {
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = (float)v[i]; } };
template <> struct fir_raw<bf16, 4> { bf16x4 v; __device__ void load(const bf16* p) { v = *reinterpret_cast<const bf16x4*>(p); }
  __device__ void get(float (&f)[4]) const {
#pragma unroll
    for (int i = 0; i < 4; ++i) f[i] = (float)v[i]; } };
template <> struct fir_raw<float, 4> { f32x4 v; __device__ void load(const float* p) { v = *reinterpret_cast<const f32x4*>(p); }
  __device__ void get(float (&f)[4]) const {
#pragma unroll
    for (int i = 0; i < 4; ++i) f[i] = v[i]; } };
// activation + zero padding of an already loaded pixel (the arithmetic of fir_load_px)
template <int VEC, bool ACT>
__device__ __forceinline__ void fir_act_px(bool ok, const float (&a)[VEC], const float (&d)[VEC], float (&r)[VEC], float (&ac)[VEC]) {
  const float m = ok ? 1.f : 0.f;
#pragma unroll
  for (int i = 0; i < VEC; ++i) {
    ac[i] = ACT ? m * fd_silu(fmaf(r[i], a[i], d[i])) : 0.f;
    r[i] *= m;
  }
}

// down: one thread = one VEC-channel vector of a BY x BX block of output pixels: the (2BY+2) x (2BX+2) input patch is
// loaded and activated once (2x2: 9 instead of 16 SiLU evaluations per output; 1x1 is the direct form).
template <typename T, int VEC, bool ACT, int BY, int BX>
__global__ __launch_bounds__(256) void fir_down_kernel(const T* __restrict__ x, const float* __restrict__ affine,
                                                       T* __restrict__ out_raw, T* __restrict__ out_act, int B, int H,
                                                       int W, int C) {
  constexpr int PSY = 2 * BY + 2, PSX = 2 * BX + 2;   // input patch
  const int cvn = C / VEC;
  const int OH = H >> 1, OW = W >> 1, nbx = (OW + BX - 1) / BX, nby = (OH + BY - 1) / BY;
  const long long total = (long long)B * nby * nbx * cvn;
  const long long idx = blockIdx.x * 256ll + threadIdx.x;
  if (idx >= total) return;
  const int cv = (int)(idx % cvn);
  long long q = idx / cvn;
  const int ox0 = (int)(q % nbx) * BX; q /= nbx;
  const int oy0 = (int)(q % nby) * BY;
  const int b = (int)(q / nby);
  const int c = cv * VEC;
  float a[VEC], d[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) { a[i] = 0.f; d[i] = 0.f; }
  if (ACT) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) { a[i] = affine[((size_t)b * C + c + i) * 2]; d[i] = affine[((size_t)b * C + c + i) * 2 + 1]; }
  }
  const float wt[4] = {0.125f, 0.375f, 0.375f, 0.125f};
  float accr[BY][BX][VEC], acca[BY][BX][VEC];
#pragma unroll
  for (int py = 0; py < BY; ++py)
#pragma unroll
    for (int px = 0; px < BX; ++px)
#pragma unroll
      for (int i = 0; i < VEC; ++i) { accr[py][px][i] = 0.f; acca[py][px][i] = 0.f; }
  const size_t img = (size_t)b * H * W;
#pragma unroll
  for (int ry = 0; ry < PSY; ++ry) {               // input row iy = 2 * oy0 - 1 + ry
    const int iy = 2 * oy0 - 1 + ry;
    const bool yok = iy >= 0 && iy < H;
    float hr[BX][VEC], ha[BX][VEC];               // horizontal sums of this row for the BX output columns
#pragma unroll
    for (int px = 0; px < BX; ++px)
#pragma unroll
      for (int i = 0; i < VEC; ++i) { hr[px][i] = 0.f; ha[px][i] = 0.f; }
#pragma unroll
    for (int rx = 0; rx < PSX; ++rx) {
      const int ix = 2 * ox0 - 1 + rx;
      float r[VEC], ac[VEC];
      fir_load_px<T, VEC, ACT>(x, (img + (size_t)fir_clamp(iy, H) * W + fir_clamp(ix, W)) * C + c, yok && ix >= 0 && ix < W, a, d, r, ac);
#pragma unroll
      for (int px = 0; px < BX; ++px) {
        const int kx = rx - 2 * px;               // tap index of this column for output column px
        if (kx >= 0 && kx < 4) {
#pragma unroll
          for (int i = 0; i < VEC; ++i) { hr[px][i] = fmaf(wt[kx], r[i], hr[px][i]); if (ACT) ha[px][i] = fmaf(wt[kx], ac[i], ha[px][i]); }
        }
      }
    }
#pragma unroll
    for (int py = 0; py < BY; ++py) {
      const int ky = ry - 2 * py;
      if (ky >= 0 && ky < 4) {
#pragma unroll
        for (int px = 0; px < BX; ++px)
#pragma unroll
          for (int i = 0; i < VEC; ++i) {
            accr[py][px][i] = fmaf(wt[ky], hr[px][i], accr[py][px][i]);
            if (ACT) acca[py][px][i] = fmaf(wt[ky], ha[px][i], acca[py][px][i]);
          }
      }
    }
    __builtin_amdgcn_sched_barrier(0);            // one patch row of loads in flight at a time (bounds the register use)
  }
#pragma unroll
  for (int py = 0; py < BY; ++py)
#pragma unroll
    for (int px = 0; px < BX; ++px) {
      const int oy = oy0 + py, ox = ox0 + px;
      if (oy < OH && ox < OW) {
        const size_t o = (((size_t)b * OH + oy) * OW + ox) * C + c;
        if (out_raw) fd_store_vec<T, VEC>(out_raw + o, accr[py][px]);
        if (ACT && out_act) fd_store_vec<T, VEC>(out_act + o, acca[py][px]);
      }
    }
}

// down, big grids: one thread = 4 channels of a BX-wide column block, MARCHING down a strip of NR output rows: every input row is
// loaded and activated once per thread and enters the two output rows it belongs to ((2BX+2)/(2BX) x (2NR+2)/(2NR) = 1.33 SiLU
// evaluations per input instead of 1.875 with 4x2 blocks).  Per output the fma sequence is the one of fir_down_kernel (horizontal taps
// ascending from 0, then vertical taps ascending from 0): identical bits.  The FIR arithmetic is written on channel pairs (v_pk_fma_f32).
typedef float fir_f2 __attribute__((ext_vector_type(2)));
// FAST (every strip and column block full, both outputs): the stores are unconditional and the row-pair step exists three times --
// without stores (row pair 0), with stores (row pair 1, peeled) and as the loop body -- so that every path into a wait for the next
// input row carries the same memory operations: hipcc's s_waitcnt vmcnt(n) then counts the stores still in flight instead of waiting
// for them (see fir_raw).
template <typename T, int BX, int NR, bool FAST = false>
__global__ __launch_bounds__(256) void fir_down_march_kernel(const T* __restrict__ x, const float* __restrict__ affine, T* __restrict__ out_raw,
                                                             T* __restrict__ out_act, int B, int H, int W, int C) {
  constexpr int VEC = 4, PSX = 2 * BX + 2;
  const int cvn = C / VEC;
  const int OH = H >> 1, OW = W >> 1, nbx = (OW + BX - 1) / BX, nst = (OH + NR - 1) / NR;
  const long long total = (long long)B * nst * nbx * cvn;
  const long long idx = blockIdx.x * 256ll + threadIdx.x;
  if (idx >= total) return;
  const int cv = (int)(idx % cvn);
  long long q = idx / cvn;
  const int ox0 = (int)(q % nbx) * BX; q /= nbx;
  const int oy0 = (int)(q % nst) * NR;
  const int b = (int)(q / nst);
  const int c = cv * VEC;
  float a[VEC], d[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) { a[i] = affine[((size_t)b * C + c + i) * 2]; d[i] = affine[((size_t)b * C + c + i) * 2 + 1]; }
  const fir_f2 wt2[4] = {{0.125f, 0.125f}, {0.375f, 0.375f}, {0.375f, 0.375f}, {0.125f, 0.125f}};
  // [output row: prev = rp - 1 | cur = rp][column][raw lo, raw hi, act lo, act hi channel pairs]
  fir_f2 acc[2][BX][4];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int px = 0; px < BX; ++px)
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[s][px][k] = fir_f2{0.f, 0.f};
  const size_t img = (size_t)b * H * W;
  int xi[PSX]; bool xok[PSX];
#pragma unroll
  for (int rx = 0; rx < PSX; ++rx) { const int ix = 2 * ox0 - 1 + rx; xok[rx] = ix >= 0 && ix < W; xi[rx] = fir_clamp(ix, W); }
  const int nrows = FAST ? NR : (OH - oy0 < NR ? OH - oy0 : NR);
  fir_raw<T, VEC> nxt[PSX];
  auto request_row = [&](int iy) {              // (clamped: the zero padding is a factor later)
    const size_t row = (img + (size_t)fir_clamp(iy, H) * W) * C + c;
#pragma unroll
    for (int rx = 0; rx < PSX; ++rx) nxt[rx].load(x + row + (size_t)xi[rx] * C);
  };
  // row pair rp = input rows 2 (oy0 + rp) - 1 and 2 (oy0 + rp): taps (2, 3) of output row rp - 1, (0, 1) of rp; then output row rp - 1 is
  // complete (stored when `store`), and rp becomes the previous row
  auto step = [&](int rp, auto store) __attribute__((always_inline)) {
#pragma unroll
    for (int par = 0; par < 2; ++par) {
      const int iy = 2 * (oy0 + rp) - 1 + par;
      const bool yok = iy >= 0 && iy < H;
      float r[PSX][VEC];
#pragma unroll
      for (int rx = 0; rx < PSX; ++rx) nxt[rx].get(r[rx]);
      request_row(iy + 1);                      // the next row, before this row pair's stores; one row past the strip at the end
      __builtin_amdgcn_sched_barrier(0);
      fir_f2 h[BX][4];
#pragma unroll
      for (int px = 0; px < BX; ++px)
#pragma unroll
        for (int k = 0; k < 4; ++k) h[px][k] = fir_f2{0.f, 0.f};
#pragma unroll
      for (int rx = 0; rx < PSX; ++rx) {
        const float m = yok && xok[rx] ? 1.f : 0.f;
        float ac[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) { ac[i] = m * fd_silu(fmaf(r[rx][i], a[i], d[i])); r[rx][i] *= m; }
        const fir_f2 v[4] = {{r[rx][0], r[rx][1]}, {r[rx][2], r[rx][3]}, {ac[0], ac[1]}, {ac[2], ac[3]}};
#pragma unroll
        for (int px = 0; px < BX; ++px) {
          const int kx = rx - 2 * px;
          if (kx >= 0 && kx < 4) {
#pragma unroll
            for (int k = 0; k < 4; ++k) h[px][k] = __builtin_elementwise_fma(wt2[kx], v[k], h[px][k]);
          }
        }
      }
#pragma unroll
      for (int px = 0; px < BX; ++px)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          acc[1][px][k] = __builtin_elementwise_fma(wt2[par], h[px][k], acc[1][px][k]);
          acc[0][px][k] = __builtin_elementwise_fma(wt2[2 + par], h[px][k], acc[0][px][k]);
        }
    }
    if (decltype(store)::value) {
      const int oy = oy0 + rp - 1;
#pragma unroll
      for (int px = 0; px < BX; ++px) {
        const int ox = ox0 + px;
        if (FAST || ox < OW) {
          const size_t o = (((size_t)b * OH + oy) * OW + ox) * C + c;
          const float vr[VEC] = {acc[0][px][0][0], acc[0][px][0][1], acc[0][px][1][0], acc[0][px][1][1]};
          const float va[VEC] = {acc[0][px][2][0], acc[0][px][2][1], acc[0][px][3][0], acc[0][px][3][1]};
          if (FAST || out_raw) fd_store_vec<T, VEC>(out_raw + o, vr);
          if (FAST || out_act) fd_store_vec<T, VEC>(out_act + o, va);
        }
      }
    }
#pragma unroll
    for (int px = 0; px < BX; ++px)
#pragma unroll
      for (int k = 0; k < 4; ++k) { acc[0][px][k] = acc[1][px][k]; acc[1][px][k] = fir_f2{0.f, 0.f}; }
  };
  request_row(2 * oy0 - 1);
  step(0, std::false_type{});
  if (FAST) {
    step(1, std::true_type{});
#pragma unroll 1
    for (int rp = 2; rp <= NR; ++rp) step(rp, std::true_type{});
  } else {
#pragma unroll 1
    for (int rp = 1; rp <= nrows; ++rp) step(rp, std::true_type{});
  }
}

// up: one thread = VEC channels of BX input columns, N input rows: 2 BX output columns x 2N output rows; BX + 2 columns are loaded and
// activated per row ((BX + 2) / BX x (N + 2) / N activations per input: 3.75 at 1 x 8, 2.5 at 2 x 8).  The arithmetic is written on
// channel pairs (v_pk_mul_f32 / v_pk_fma_f32: the same IEEE operations per element as the scalar form); every output is the same
// operation sequence for every (N, BX).
// FAST: every strip is full (H % N == 0, W % BX == 0) and both outputs exist: the stores are UNCONDITIONAL -- no control flow between a
// row's loads and the next row's use, so hipcc's s_waitcnt vmcnt(n) counts the stores in flight exactly instead of joining a path
// without them (which made every wait for a row also a wait for the previous row's stores).
template <typename T, int VEC, bool ACT, int N, int BX, bool FAST = false>
__global__ __launch_bounds__(256) void fir_up_kernel(const T* __restrict__ x, const float* __restrict__ affine,
                                                     T* __restrict__ out_raw, T* __restrict__ out_act, int B, int H,
                                                     int W, int C) {
  constexpr int NP = VEC / 2;
  const int cvn = C / VEC, ns = (H + N - 1) / N, nbx = (W + BX - 1) / BX;
  const long long total = (long long)B * ns * nbx * cvn;
  const long long idx = blockIdx.x * 256ll + threadIdx.x;
  if (idx >= total) return;
  const int cv = (int)(idx % cvn);
  long long q = idx / cvn;
  const int ix0 = (int)(q % nbx) * BX; q /= nbx;
  const int y0 = (int)(q % ns) * N;
  const int b = (int)(q / ns);
  const int c = cv * VEC;
  float a[VEC], d[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) { a[i] = 0.f; d[i] = 0.f; }
  if (ACT) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) { a[i] = affine[((size_t)b * C + c + i) * 2]; d[i] = affine[((size_t)b * C + c + i) * 2 + 1]; }
  }
  const int OW = 2 * W, OH = 2 * H;
  const fir_f2 w75 = {0.75f, 0.75f}, w25 = {0.25f, 0.25f};
  // horizontally combined rows for the output columns 2ix (px = 0: (x[ix-1] + 3 x[ix]) / 4) and 2ix+1 (px = 1), slot = row % 3
  fir_f2 hr[3][2 * BX][NP], ha[3][2 * BX][NP];
  const size_t img = (size_t)b * H * W;
  fir_raw<T, VEC> nxt[BX + 2];
  auto request_row = [&](int j) {                // input row y0 - 1 + j (clamped: the zero padding is a factor later)
    const size_t row = (img + (size_t)fir_clamp(y0 - 1 + j, H) * W) * C + c;
#pragma unroll
    for (int dx = 0; dx < BX + 2; ++dx) nxt[dx].load(x + row + (size_t)fir_clamp(ix0 + dx - 1, W) * C);
  };
  request_row(0);
#pragma unroll
  for (int j = 0; j < N + 2; ++j) {              // input row yy = y0 - 1 + j
    const int yy = y0 - 1 + j;
    const bool yok = yy >= 0 && yy < H;
    float r[BX + 2][VEC], ac[BX + 2][VEC];
#pragma unroll
    for (int dx = 0; dx < BX + 2; ++dx) nxt[dx].get(r[dx]);
    if (j + 1 < N + 2) request_row(j + 1);       // before this row's stores (see fir_raw)
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int dx = 0; dx < BX + 2; ++dx) {
      const int xx = ix0 + dx - 1;
      fir_act_px<VEC, ACT>(yok && xx >= 0 && xx < W, a, d, r[dx], ac[dx]);
    }
#pragma unroll
    for (int bx = 0; bx < BX; ++bx)
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        const fir_f2 r0 = {r[bx][2 * i], r[bx][2 * i + 1]}, r1 = {r[bx + 1][2 * i], r[bx + 1][2 * i + 1]}, r2 = {r[bx + 2][2 * i], r[bx + 2][2 * i + 1]};
        hr[j % 3][2 * bx][i] = __builtin_elementwise_fma(w75, r1, w25 * r0);
        hr[j % 3][2 * bx + 1][i] = __builtin_elementwise_fma(w75, r1, w25 * r2);
        if (ACT) {
          const fir_f2 a0 = {ac[bx][2 * i], ac[bx][2 * i + 1]}, a1 = {ac[bx + 1][2 * i], ac[bx + 1][2 * i + 1]}, a2 = {ac[bx + 2][2 * i], ac[bx + 2][2 * i + 1]};
          ha[j % 3][2 * bx][i] = __builtin_elementwise_fma(w75, a1, w25 * a0);
          ha[j % 3][2 * bx + 1][i] = __builtin_elementwise_fma(w75, a1, w25 * a2);
        }
      }
    if (j >= 2) {                                // rows j-2, j-1, j complete the two output rows of input row iy = yy - 1
      const int iy = yy - 1;
      if (FAST || iy < H) {
        const int up = (j - 2) % 3, m = (j - 1) % 3, dn = j % 3;
#pragma unroll
        for (int py = 0; py < 2; ++py) {
          const int other = py == 0 ? up : dn;   // py = 0: (row[iy-1] + 3 row[iy]) / 4; py = 1: (3 row[iy] + row[iy+1]) / 4
          const size_t o = (((size_t)b * OH + 2 * iy + py) * OW + 2 * ix0) * C + c;
#pragma unroll
          for (int px = 0; px < 2 * BX; ++px) {
            if (!FAST && BX > 1 && ix0 + px / 2 >= W) continue;
            float o0[VEC], p0[VEC];
#pragma unroll
            for (int i = 0; i < NP; ++i) {
              const fir_f2 t0 = __builtin_elementwise_fma(w75, hr[m][px][i], w25 * hr[other][px][i]);
              o0[2 * i] = t0[0]; o0[2 * i + 1] = t0[1];
              if (ACT) {
                const fir_f2 u0 = __builtin_elementwise_fma(w75, ha[m][px][i], w25 * ha[other][px][i]);
                p0[2 * i] = u0[0]; p0[2 * i + 1] = u0[1];
              }
            }
            if (FAST || out_raw) fd_store_vec<T, VEC>(out_raw + o + (size_t)px * C, o0);
            if (ACT && (FAST || out_act)) fd_store_vec<T, VEC>(out_act + o + (size_t)px * C, p0);
          }
        }
      }
    }
  }
}

// =====================================================================================================
// Generic upfirdn2d (op/upfirdn2d.py:183-224 semantics; CUDA twin upfirdn2d_kernel.cu:60-218)
// =====================================================================================================
template <typename T>
__global__ __launch_bounds__(256) void upfirdn2d_kernel(const T* __restrict__ in, const float* __restrict__ kernel,
                                                        T* __restrict__ out, int major, int in_h, int in_w, int minor,
                                                        int kh, int kw, int up_x, int up_y, int down_x, int down_y,
                                                        int pad_x0, int pad_y0, int out_h, int out_w) {
  const long long total = (long long)major * out_h * out_w * minor;
  for (long long idx = blockIdx.x * 256ll + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const int mi = (int)(idx % minor);
    long long r = idx / minor;
    const int ox = (int)(r % out_w); r /= out_w;
    const int oy = (int)(r % out_h);
    const int mj = (int)(r / out_h);
    float acc = 0.f;
    // out[oy,ox] = sum_{i,j} kernel[kh-1-i][kw-1-j] * U[oy*down_y + i - pad_y0][ox*down_x + j - pad_x0],
    // U = zero-inserted input (U[u][v] = in[u/up_y][v/up_x] when both divisible and in range)
    for (int i = 0; i < kh; ++i) {
      const int u = oy * down_y + i - pad_y0;
      if (u < 0 || u % up_y != 0) continue;
      const int iy = u / up_y;
      if (iy >= in_h) continue;
      for (int j = 0; j < kw; ++j) {
        const int v = ox * down_x + j - pad_x0;
        if (v < 0 || v % up_x != 0) continue;
        const int ix = v / up_x;
        if (ix >= in_w) continue;
        acc = fmaf(kernel[(kh - 1 - i) * kw + (kw - 1 - j)], Elem<T>::ld(in + (((size_t)mj * in_h + iy) * in_w + ix) * minor + mi), acc);
      }
    }
    Elem<T>::st(out + idx, acc);
  }
}

// fused_bias_act_kernel.cu:30-61, grad == 0
__global__ void fused_bias_act_kernel(const float* __restrict__ x, const float* __restrict__ bias, float* __restrict__ out,
                                      long long n, int step_b, int size_b, int act, float alpha, float scale) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    float v = x[i];
    if (bias) v += bias[(i / step_b) % size_b];
    if (act == 3) v = v > 0.f ? v : v * alpha;
    out[i] = v * scale;
  }
}

}  // namespace

// ---- FIR x2 resampling: one rule that picks the kernel (fir_select), one switch that launches what it picked (launch_fir) ----
// family: FD_FIR_UP = fir_up_kernel (rows = input rows per thread N, cols = BX), FD_FIR_DOWN = fir_down_kernel (rows x cols = the BY x BX
// output block), FD_FIR_DOWN_MARCH = fir_down_march_kernel (rows = NR output rows of a strip, cols = 4); vec = channels per thread;
// act = the ACT instantiation (an affine is present); fast = the unconditional-store form; grid = workgroups of 256 threads.
struct fir_variant { int family, rows, cols, vec, act, fast; long long grid; };

// The choice for one fd_fir_resample call, from the shape and from WHICH of affine / out_raw / out_act are present (FD_EINVAL where the
// call is refused).  Rows / output block per thread of the fused (activated) variants: big blocks re-use activated inputs (fewer SiLU
// evaluations per output), small ones make more, shorter threads -- a small image is latency-bound (one clip at 384 x 64: 13-25 us with
// the big blocks).  Every output is the same fma sequence in every variant, so the choice may depend on the batch size.
static int fir_select(int B, int H, int W, int C, int direction, int dtype, bool has_affine, bool has_raw, bool has_act, fir_variant* out) {
  FD_REQUIRE(has_raw || has_act, "fd_fir_resample: null pointer");
  FD_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0, "fd_fir_resample: bad shape (B=%d H=%d W=%d C=%d)", B, H, W, C);
  FD_REQUIRE(direction == 1 || direction == -1, "fd_fir_resample: direction must be +1 (up) or -1 (down)");
  FD_REQUIRE(C % 4 == 0, "fd_fir_resample: C must be a multiple of 4");
  FD_REQUIRE(direction > 0 || (H % 2 == 0 && W % 2 == 0), "fd_fir_resample: down needs even H, W");
  FD_REQUIRE(!has_act || has_affine, "fd_fir_resample: out_act needs affine");
  FD_REQUIRE(dtype == FD_BF16 || dtype == FD_F32, "fd_fir_resample: bad dtype %d", dtype);
  const bool half = dtype == FD_BF16;
  // bf16: 8-channel (16-byte) vectors where C allows, except the fused down direction (strips / 4x2 blocks of 4-channel vectors: round 2,
  // profiles/r02_fir_down_variants.txt -- the 4x2 block fits the register budget only with 4 channels: 430 us vs 512 us for 8-channel
  // vectors x 4x1 at 8 x 768 x 256 x 256)
  const int vec = half && !(direction < 0 && has_affine) && C % 8 == 0 ? 8 : 4;
  const int R = direction > 0 ? H : H / 2, Q = direction > 0 ? W : W / 2;   // the rows / columns the threads tile: input (up), output (down)
  auto grid = [&](int rows, int cols) { return ((long long)B * fd_cdiv(R, rows) * fd_cdiv(Q, cols) * (C / vec) + 255) / 256; };
  auto pick = [&](int family, int rows, int cols, bool fast) {
    *out = fir_variant{family, rows, cols, vec, has_affine ? 1 : 0, fast ? 1 : 0, grid(rows, cols)};
    return FD_OK;
  };
  constexpr long long ENOUGH = 512;   // workgroups that keep 256 CUs busy
  if (direction > 0) {
    if (!has_affine) return pick(FD_FIR_UP, 1, 1, false);
    // measured at 8 x 384 x 128 x 256 -> 768 x 256 (1.8 GB moved): 8 rows x 1 column, 8-channel vectors 414 us; 16 rows 446; 4 rows 432;
    // 4-channel vectors 409 / 458 / 463; two columns per thread (2.5 instead of 3.75 activations per input) 403 (4 ch x 8 rows): the up
    // direction does not react to the activation count or the vector width (4.4 TB/s, 4.0 of them stores) -- BX stays 1.  What it reacts
    // to is the store accounting (FAST): 357-361 us; FAST variants of the other shapes: 4 rows 404, 16 rows 392, 4-channel vectors 380-448
    if (grid(8, 1) >= ENOUGH) return pick(FD_FIR_UP, 8, 1, H % 8 == 0 && has_raw && has_act);
    if (grid(2, 1) >= ENOUGH) return pick(FD_FIR_UP, 2, 1, false);
    return pick(FD_FIR_UP, 1, 1, false);
  }
  // measured on MI355X at 8 x 768 x 256 x 256 (bf16, dual output): 1x1 756 us, 2x2 675, 2x1 614, 8x1 565, 4x2 543, 4x1 467
  if (!has_affine) return pick(FD_FIR_DOWN, 1, 1, false);
  // round 3: marching strips of NR output rows x 4 columns (1.33 instead of 1.875 activations per input, packed FIR arithmetic)
  // measured at B = 8 x 256 channels (scripts/fir_bench.py): 768 x 256: 4x2 blocks 444 us, strips of 4 / 8 / 16 rows 315 / 302 / 292 us;
  // 384 x 128: 130 us, 102 / 97 / 120 us (16-row strips leave 1.5 workgroups per CU) -> the tallest strip with >= 3 workgroups per CU
  constexpr long long FILL = 768;
  if (has_act)
    for (int nr = 16; nr >= 4; nr >>= 1)
      if (grid(nr, 4) >= FILL) return pick(FD_FIR_DOWN_MARCH, nr, 4, has_raw && R % nr == 0 && Q % 4 == 0);
  if (half && grid(4, 2) >= ENOUGH) return pick(FD_FIR_DOWN, 4, 2, false);
  if (half && grid(2, 1) >= ENOUGH) return pick(FD_FIR_DOWN, 2, 1, false);
  if (!half && grid(4, 1) >= ENOUGH) return pick(FD_FIR_DOWN, 4, 1, false);
  return pick(FD_FIR_DOWN, 1, 1, false);
}

// Launches exactly the variant `v` that fir_select returned (T / VEC = its storage type and vector width).  The kernels fir_select cannot
// pick for this <T, VEC> are not instantiated: a variant without a case below is an internal error, never another kernel.
template <typename T, int VEC>
static int launch_fir(const fir_variant& v, const void* x, const float* affine, void* out_raw, void* out_act, int B, int H, int W, int C,
                      hipStream_t st) {
  [[maybe_unused]] constexpr bool HALF = sizeof(T) == 2;
  const dim3 grid((unsigned)v.grid);
  const int key = ((v.family * 100 + v.rows) * 10 + v.cols) * 100 + v.act * 10 + v.fast;
#define FD_FIR_ARGS grid, dim3(256), 0, st, (const T*)x, affine, (T*)out_raw, (T*)out_act, B, H, W, C
#define FD_FIR_KEY(FAM_, ROWS_, COLS_, ACT_, FAST_) ((((FAM_) * 100 + (ROWS_)) * 10 + (COLS_)) * 100 + (ACT_) * 10 + (FAST_))
  bool done = true;
  switch (key) {
    case FD_FIR_KEY(FD_FIR_UP, 1, 1, 0, 0): hipLaunchKernelGGL((fir_up_kernel<T, VEC, false, 1, 1>), FD_FIR_ARGS); break;
    case FD_FIR_KEY(FD_FIR_UP, 8, 1, 1, 1): hipLaunchKernelGGL((fir_up_kernel<T, VEC, true, 8, 1, true>), FD_FIR_ARGS); break;
    case FD_FIR_KEY(FD_FIR_UP, 8, 1, 1, 0): hipLaunchKernelGGL((fir_up_kernel<T, VEC, true, 8, 1>), FD_FIR_ARGS); break;
    case FD_FIR_KEY(FD_FIR_UP, 2, 1, 1, 0): hipLaunchKernelGGL((fir_up_kernel<T, VEC, true, 2, 1>), FD_FIR_ARGS); break;
    case FD_FIR_KEY(FD_FIR_UP, 1, 1, 1, 0): hipLaunchKernelGGL((fir_up_kernel<T, VEC, true, 1, 1>), FD_FIR_ARGS); break;
    case FD_FIR_KEY(FD_FIR_DOWN, 1, 1, 0, 0): hipLaunchKernelGGL((fir_down_kernel<T, VEC, false, 1, 1>), FD_FIR_ARGS); break;
    default: done = false;
  }
  if constexpr (VEC == 4) {   // the fused down direction always runs on 4-channel vectors (fir_select)
    if (!done) {
      done = true;
      switch (key) {
        case FD_FIR_KEY(FD_FIR_DOWN_MARCH, 16, 4, 1, 1): hipLaunchKernelGGL((fir_down_march_kernel<T, 4, 16, true>), FD_FIR_ARGS); break;
        case FD_FIR_KEY(FD_FIR_DOWN_MARCH, 16, 4, 1, 0): hipLaunchKernelGGL((fir_down_march_kernel<T, 4, 16, false>), FD_FIR_ARGS); break;
        case FD_FIR_KEY(FD_FIR_DOWN_MARCH, 8, 4, 1, 1): hipLaunchKernelGGL((fir_down_march_kernel<T, 4, 8, true>), FD_FIR_ARGS); break;
        case FD_FIR_KEY(FD_FIR_DOWN_MARCH, 8, 4, 1, 0): hipLaunchKernelGGL((fir_down_march_kernel<T, 4, 8, false>), FD_FIR_ARGS); break;
        case FD_FIR_KEY(FD_FIR_DOWN_MARCH, 4, 4, 1, 1): hipLaunchKernelGGL((fir_down_march_kernel<T, 4, 4, true>), FD_FIR_ARGS); break;
        case FD_FIR_KEY(FD_FIR_DOWN_MARCH, 4, 4, 1, 0): hipLaunchKernelGGL((fir_down_march_kernel<T, 4, 4, false>), FD_FIR_ARGS); break;
        case FD_FIR_KEY(FD_FIR_DOWN, 1, 1, 1, 0): hipLaunchKernelGGL((fir_down_kernel<T, VEC, true, 1, 1>), FD_FIR_ARGS); break;
        default: done = false;
      }
    }
    if constexpr (HALF) {
      if (!done && key == FD_FIR_KEY(FD_FIR_DOWN, 4, 2, 1, 0)) { hipLaunchKernelGGL((fir_down_kernel<T, VEC, true, 4, 2>), FD_FIR_ARGS); done = true; }
      if (!done && key == FD_FIR_KEY(FD_FIR_DOWN, 2, 1, 1, 0)) { hipLaunchKernelGGL((fir_down_kernel<T, VEC, true, 2, 1>), FD_FIR_ARGS); done = true; }
    } else {
      if (!done && key == FD_FIR_KEY(FD_FIR_DOWN, 4, 1, 1, 0)) { hipLaunchKernelGGL((fir_down_kernel<T, VEC, true, 4, 1>), FD_FIR_ARGS); done = true; }
    }
  }
#undef FD_FIR_KEY
#undef FD_FIR_ARGS
  if (!done)
    return fd_set_error(FD_ESTATE, "internal: fd_fir_resample has no kernel for variant (family %d, %d x %d, vec %d, act %d, fast %d)", v.family,
                        v.rows, v.cols, v.vec, v.act, v.fast);
  FD_LAUNCH_CHECK();
  return FD_OK;
}

extern "C" int fd_fir_variant(int B, int H, int W, int C, int direction, int dtype, int has_affine, int want_raw, int want_act) {
  fir_variant v;
  const int rc = fir_select(B, H, W, C, direction, dtype, has_affine != 0, want_raw != 0, want_act != 0, &v);
  if (rc != FD_OK) return rc;
  return ((((v.family * 100 + v.rows) * 10 + v.cols) * 10 + v.vec) * 10 + v.act) * 10 + v.fast;
}

extern "C" int fd_fir_resample(const void* x, const float* affine, void* out_raw, void* out_act, int B, int H, int W,
                               int C, int direction, int dtype, void* stream) {
  FD_REQUIRE(x, "fd_fir_resample: null pointer");
  fir_variant v;
  const int rc = fir_select(B, H, W, C, direction, dtype, affine != nullptr, out_raw != nullptr, out_act != nullptr, &v);
  if (rc != FD_OK) return rc;
  hipStream_t st = fd_stream(stream);
  if (dtype == FD_F32) return launch_fir<float, 4>(v, x, affine, out_raw, out_act, B, H, W, C, st);
  if (v.vec == 8) return launch_fir<bf16, 8>(v, x, affine, out_raw, out_act, B, H, W, C, st);
  return launch_fir<bf16, 4>(v, x, affine, out_raw, out_act, B, H, W, C, st);
}

extern "C" int fd_upfirdn2d_out_size(int in_size, int up, int down, int pad0, int pad1, int ksize) {
  return (in_size * up + pad0 + pad1 - ksize + down) / down;  // upfirdn2d_kernel.cu:248-251
}

extern "C" int fd_upfirdn2d(const void* input, const float* kernel, void* out, int major, int in_h, int in_w, int minor,
                            int kernel_h, int kernel_w, int up_x, int up_y, int down_x, int down_y, int pad_x0, int pad_x1,
                            int pad_y0, int pad_y1, int dtype, void* stream) {
  FD_REQUIRE(input && kernel && out, "fd_upfirdn2d: null pointer");
  FD_REQUIRE(up_x >= 1 && up_y >= 1 && down_x >= 1 && down_y >= 1, "fd_upfirdn2d: up/down factors must be >= 1");
  FD_REQUIRE(major > 0 && in_h > 0 && in_w > 0 && minor > 0 && kernel_h > 0 && kernel_w > 0, "fd_upfirdn2d: bad shape");
  const int out_h = fd_upfirdn2d_out_size(in_h, up_y, down_y, pad_y0, pad_y1, kernel_h);
  const int out_w = fd_upfirdn2d_out_size(in_w, up_x, down_x, pad_x0, pad_x1, kernel_w);
  FD_REQUIRE(out_h > 0 && out_w > 0, "fd_upfirdn2d: empty output (%d x %d)", out_h, out_w);
  const long long n = (long long)major * out_h * out_w * minor;
  dim3 grid(grid_for(n, 256, 65536));
  if (dtype == FD_F32)
    hipLaunchKernelGGL(upfirdn2d_kernel<float>, grid, dim3(256), 0, fd_stream(stream), (const float*)input, kernel, (float*)out, major,
                       in_h, in_w, minor, kernel_h, kernel_w, up_x, up_y, down_x, down_y, pad_x0, pad_y0, out_h, out_w);
  else if (dtype == FD_BF16)
    hipLaunchKernelGGL(upfirdn2d_kernel<bf16>, grid, dim3(256), 0, fd_stream(stream), (const bf16*)input, kernel, (bf16*)out, major,
                       in_h, in_w, minor, kernel_h, kernel_w, up_x, up_y, down_x, down_y, pad_x0, pad_y0, out_h, out_w);
  else
    return fd_set_error(FD_EINVAL, "fd_upfirdn2d: bad dtype %d", dtype);
  FD_LAUNCH_CHECK();
  return FD_OK;
}

extern "C" int fd_fused_bias_act(const float* x, const float* bias, float* out, long long n, int step_b, int size_b,
                                 int act, float alpha, float scale, void* stream) {
  FD_REQUIRE(x && out && n >= 0, "fd_fused_bias_act: bad arguments");
  FD_REQUIRE(act == 1 || act == 3, "fd_fused_bias_act: act must be 1 (linear) or 3 (lrelu)");
  FD_REQUIRE(bias == nullptr || (step_b > 0 && size_b > 0), "fd_fused_bias_act: bad bias geometry");
  if (n == 0) return FD_OK;
  hipLaunchKernelGGL(fused_bias_act_kernel, dim3(grid_for(n, 256, 65536)), dim3(256), 0, fd_stream(stream), x, bias, out, n,
                     step_b, size_b, act, alpha, scale);
  FD_LAUNCH_CHECK();
  return FD_OK;
}
