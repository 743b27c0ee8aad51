// fracshift.hip -- a ragged batch of signals moved by a whole number of samples plus a fraction, with polarity (include/flowdec_hip.h
// "Alignment in time"; host yardstick and the definition: flowdec_amd/align.py frac_shift).  eval_cli --align-frac and the --align of
// estimate_cli / loss_cli cut every signal whose delay has a fractional part (or an inverted polarity) with it.
//
//   out[b][i] = f32( sign_b * sum_{k = -W + 1 .. W} f64(s_b[n0_b + i + base_b + k]) * taps_b[k + W - 1] ),   0 <= i < n1_b - n0_b
//
// k ascending, every product and every sum rounded to float64 on its own (no contraction: the pragma below), ONE rounding to float32.
// Samples outside [0, len_b) are zeros by definition: staged as zeros from the index alone, never loaded.  The taps are a row of the
// host's bank (align.frac_bank): the device evaluates no transcendental.  An output sample is one thread's own chain over values that
// depend on its clip only, so a clip's samples have the same bits alone, in a batch and at any batch position.
//
// Workgroup (tile, b) owns TILE output samples: it stages the TILE + 2 W - 1 input samples they read once in LDS as float32 and the 2 W
// taps as float64; a thread then owns the outputs t, t + 256, ... (consecutive lanes read consecutive LDS words, the tap is a broadcast).
// Every index is clamped: len into the row, the window into [0, Lo], the input index tested against [0, len) in 64 bits -- a wrong table
// gives wrong samples, never an access outside a row.  The row behind the window (i >= n1 - n0) is written as zeros.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int TILE = 1024;                // output samples per workgroup
constexpr int MAX_TAPS = 256;             // W: half the filter length
constexpr int MAX_ROW = 0x7fffffff - 1024;

__global__ __launch_bounds__(256) void frac_shift_kernel(const float* __restrict__ s, const int* __restrict__ lens, int Ls, const int* __restrict__ base,
                                                         const double* __restrict__ taps, int W, const int* __restrict__ sign, const int* __restrict__ n0,
                                                         const int* __restrict__ n1, float* __restrict__ out, int Lo) {
  __shared__ float span[TILE + 2 * MAX_TAPS];
  __shared__ double h[2 * MAX_TAPS];
  const int b = blockIdx.y, t = threadIdx.x;
  const int nt = 2 * W;
  int len = lens[b];
  len = len < 0 ? 0 : (len > Ls ? Ls : len);
  long long count = (long long)n1[b] - (long long)n0[b];
  count = count < 0 ? 0 : (count > Lo ? Lo : count);
  const long long o0 = (long long)blockIdx.x * TILE;                          // the tile's first output sample
  const long long m0 = (long long)n0[b] + o0 + base[b] - W + 1;               // the input sample of span[0]
  const float* __restrict__ row = s + (size_t)b * Ls;
  for (int i = t; i < TILE + nt - 1; i += 256) {
    const long long m = m0 + i;
    span[i] = (m >= 0 && m < len) ? row[m] : 0.f;
  }
  for (int i = t; i < nt; i += 256) h[i] = taps[(size_t)b * nt + i];
  __syncthreads();
  const double sg = sign[b] < 0 ? -1.0 : 1.0;
  float* __restrict__ orow = out + (size_t)b * Lo;
  for (int i = t; i < TILE; i += 256) {
    const long long o = o0 + i;
    if (o >= Lo) break;
    double acc = 0.0;
    for (int k = 0; k < nt; ++k) {
      const double p = (double)span[i + k] * h[k];
      acc = acc + p;
    }
    orow[o] = o < count ? (float)(sg * acc) : 0.f;
  }
}

}  // namespace

extern "C" int fd_frac_shift(const float* s, const int* lens, int B, int Ls, const int* base, const double* taps, int W, const int* sign, const int* n0,
                             const int* n1, float* out, int Lo, void* stream) {
  FD_REQUIRE(s && lens && base && taps && sign && n0 && n1 && out, "fd_frac_shift: null pointer");
  FD_REQUIRE(B > 0 && B <= 65535, "fd_frac_shift: bad batch B %d (1 <= B <= 65535)", B);
  FD_REQUIRE(Ls > 0 && Ls <= MAX_ROW && Lo > 0 && Lo <= MAX_ROW, "fd_frac_shift: bad row lengths Ls %d Lo %d (1 <= Ls, Lo <= %d)", Ls, Lo, MAX_ROW);
  FD_REQUIRE(W >= 1 && W <= MAX_TAPS, "fd_frac_shift: bad half width W %d (1 <= W <= %d: 2 W taps)", W, MAX_TAPS);
  hipLaunchKernelGGL(frac_shift_kernel, dim3((Lo + TILE - 1) / TILE, B), dim3(256), 0, fd_stream(stream), s, lens, Ls, base, taps, W, sign, n0, n1, out, Lo);
  FD_LAUNCH_CHECK();
  return FD_OK;
}
