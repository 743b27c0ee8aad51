// xcorr.hip -- bounded-lag cross-correlation of ragged batches and the lag of its peak (include/flowdec_hip.h "Evaluation metrics";
// host yardstick and the definition: flowdec_amd/align.py).  eval_cli --align finds a triple's delays with it before scoring.
//
//   c[b][l + M] = sum_n a_b[n] b_b[n + l],  l in [-M, M],  n over max(0, -l) <= n < min(la, lb - l);  an empty range is exactly 0.0
//
// Rows a [B][La], b [B][Lb] float32; clip b = the first lens_a[b] / lens_b[b] samples of its rows (clamped into the row by fd_clip_len).
// The samples are float32, so every product is exact in float64 and only the float64 additions round; a term whose factor is a staged
// zero adds exactly nothing.  Samples outside [0, len) are zeros BY DEFINITION: they are staged as zeros from the index alone and never
// loaded, neither from the row's tail nor from the next row.  (Inputs are finite: an infinity inside a clip times such a zero would be a
// NaN the definition does not have.)
//
// The sum runs on the matrix cores.  With A[i][k] = a[s + k - i] and B[k][j] = b[s + k + 16 j + l_blk], one v_mfma_f64_16x16x4_f64 adds
// to C[i][j] the products a[n] b[n + l] of the 4 samples n = s - i .. s - i + 3 for the 256 lags l = l_blk + 16 j + i; s advances by 4.
// Operand lanes: A[i][k] and B[k][j] in lane (i or j) + 16 k, one float64 each; C/D: col j = lane & 15, row i = (lane >> 4) + 4 reg.
//
// The contract is the one metrics.hip states: a clip's c and lag have the same BITS alone, in a batch, at any batch position and next to
// clips of any other lengths.  Every partition and every order of addition is a function of (lens_a[b], lens_b[b], max_lag) only:
//   * s is cut at the fixed absolute positions j * SLICE, so for a lag of offset i = (l + M) % 16 slice j holds the samples
//     [j SLICE - i, (j + 1) SLICE - i); clip b has ceil((la + 15) / SLICE) slices, whatever La is
//   * workgroup (slice j, lag tile, clip b) owns the LAG_TILE lags from -M + tile * LAG_TILE; each of its four waves owns 512 of them as
//     two accumulator blocks and feeds them the slice in ASCENDING s, four samples per instruction -- no reduction across lanes or
//     waves, no atomics -- and writes one float64 partial per lag
//   * the finalise kernel adds a clip's slice partials in index order, then the lag is picked from the finished float64 values
// The slice is staged through LDS as float32 in chunks of CHUNK samples of a (and the 16 before them) and the CHUNK + LAG_TILE samples of
// b they meet; a lane converts one a and two b values per pair of instructions.  Chunks that cannot meet the tile's lags inside the clip
// are skipped (a function of la, lb, M and the tile only; skipping or adding their zeros gives the same bits).
//
// The lag is pick_lag's rule: the largest c, NaN counting as -inf; among equal maxima the smallest |l|, and +l before -l.  That is a total
// order, so the two-level reduction (256 lags per workgroup, then the workgroups' winners) finds the same lag in any grouping.
//
// Kernel variant kept: the f64 matrix instruction.  The plain v_fma_f64 form of the same partition (8 lags per thread as ascending fma
// chains over a register window of b) gives the same bits on integer data and is 12 % slower (MEASUREMENTS.md "Alignment").
//
// fd_xcorr_lags_frac (eval_cli --align-frac / --align-polarity, the --align of estimate_cli and loss_cli) runs the same slice kernel, a
// finalise variant that picks on |c| when polarity is asked for, and one workgroup per clip that interpolates the peak on a grid of 1 / Q
// samples from the host's table of windowed sincs (align.py frac_bank, refine_lag): see xcorr_refine_kernel.
#include <limits.h>
#include <math.h>

#include "measure_common.h"

namespace {

constexpr int LAG_TILE = 2048;            // lags per workgroup: 4 waves x 2 blocks of 256
constexpr int CHUNK = 2048;               // steps s staged per pass (a multiple of 4)
constexpr int APAD = 16;                  // samples of a staged in front of a chunk (the lag offsets i = 0 .. 15 reach back by i)
constexpr int SLICE = 16 * CHUNK;         // steps per workgroup: the unit of the float64 partials
constexpr int PICK = 256;                 // lags per workgroup of the finalise kernel
constexpr int MAX_LAG_CAP = 1 << 20;
constexpr int MAX_ROW = 0x7fffffff - 1024;

typedef __attribute__((ext_vector_type(4))) double f64x4;

// a clip of la samples has the steps s = 0 .. la + 14 (offset 15 meets its last sample at s = la + 14)
__host__ __device__ __forceinline__ int slices_of(long long la) { return (int)((la + 15 + SLICE - 1) / SLICE); }

// part[b][j][l + M] = sum over n in [j SLICE - i, (j + 1) SLICE - i), i = (l + M) % 16, of a_b[n] b_b[n + l], ascending, 4 per instruction
__global__ __launch_bounds__(256) void xcorr_slice_kernel(const float* __restrict__ a, const float* __restrict__ bsig, const int* __restrict__ lens_a,
                                                          const int* __restrict__ lens_b, int La, int Lb, int M, int slices,
                                                          double* __restrict__ part) {
  __shared__ float sa[CHUNK + APAD];            // sa[i] = a[n0 - APAD + i]
  __shared__ float sb[CHUNK + LAG_TILE];        // sb[i] = b[n0 + l0 + i]
  const int j = blockIdx.x, tile = blockIdx.y, b = blockIdx.z, t = threadIdx.x;
  const long long la = fd_clip_len(lens_a, b, La), lb = fd_clip_len(lens_b, b, Lb);
  if (j >= slices_of(la)) return;                               // not one of this clip's slices (uniform)
  const long long slice_lo = (long long)j * SLICE;
  const long long W = 2LL * M + 1;
  const long long l0 = -(long long)M + (long long)tile * LAG_TILE;   // the tile's first lag
  // the n that can meet a lag of this tile inside both clips: [max(0, -(l0 + LAG_TILE - 1)), min(la, lb - l0))
  const long long n_first = l0 + LAG_TILE - 1 < 0 ? -(l0 + LAG_TILE - 1) : 0;
  const long long n_end = la < lb - l0 ? la : lb - l0;
  const float* __restrict__ arow = a + (size_t)b * La;
  const float* __restrict__ brow = bsig + (size_t)b * Lb;
  const int lane = t & 63, wave = t >> 6;
  const int lo = lane & 15, hi = lane >> 4;     // A: row i = lo, k = hi;  B: col j = lo, k = hi
  f64x4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
  for (int c = 0; c < SLICE / CHUNK; ++c) {
    const long long n0 = slice_lo + (long long)c * CHUNK;       // the chunk's steps are n0 .. n0 + CHUNK - 1, its samples n0 - 15 .. n0 + CHUNK - 1
    if (n0 - 15 >= n_end) break;
    if (n0 + CHUNK <= n_first) continue;
    __syncthreads();                                            // the previous chunk has been read
    for (int i = t; i < CHUNK + APAD; i += 256) {
      const long long n = n0 - APAD + i;
      sa[i] = (n >= 0 && n < la) ? arow[n] : 0.f;
    }
    for (int i = t; i < CHUNK + LAG_TILE; i += 256) {
      const long long m = n0 + l0 + i;
      sb[i] = (m >= 0 && m < lb) ? brow[m] : 0.f;
    }
    __syncthreads();
    const float* __restrict__ pa = sa + APAD + hi - lo;                   // + s: index in [1, CHUNK + APAD - 1]
    const float* __restrict__ pb = sb + hi + 16 * lo + 512 * wave;        // + s + 256: at most 3 + 240 + 1536 + CHUNK - 4 + 256 = CHUNK + LAG_TILE - 17
#pragma unroll 4
    for (int s = 0; s < CHUNK; s += 4) {
      const double av = (double)pa[s], b0 = (double)pb[s], b1 = (double)pb[s + 256];
      acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, b0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, b1, acc1, 0, 0, 0);
    }
  }
  double* __restrict__ out = part + ((size_t)b * slices + j) * (size_t)W;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long long idx = (long long)tile * LAG_TILE + 512 * wave + 16 * lo + hi + 4 * r;     // C/D: col = lane & 15, row = (lane >> 4) + 4 r
    if (idx < W) out[idx] = acc0[r];
    if (idx + 256 < W) out[idx + 256] = acc1[r];
  }
}

// pick_lag's order: is (v1, l1) before (v0, l0)?  (NaN has been replaced by -inf)
__device__ __forceinline__ bool better(double v1, int l1, double v0, int l0) {
  if (v1 != v0) return v1 > v0;
  const int m1 = l1 < 0 ? -l1 : l1, m0 = l0 < 0 ? -l0 : l0;
  if (m1 != m0) return m1 < m0;
  return l1 > l0;
}

__device__ __forceinline__ void block_best(double& v, int& l, double* __restrict__ sv, int* __restrict__ sl) {
  const int t = threadIdx.x;
  sv[t] = v; sl[t] = l;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o && better(sv[t + o], sl[t + o], sv[t], sl[t])) { sv[t] = sv[t + o]; sl[t] = sl[t + o]; }
    __syncthreads();
  }
  v = sv[0]; l = sl[0];
}

// the clip's slice partials in index order -> part[b][0][.] (and c); the best of this workgroup's PICK lags -> best_v / best_l [b][blk],
// picked on |c| when `polarity` is set (fd_xcorr_lags_frac); the finished c is the same either way
__global__ __launch_bounds__(256) void xcorr_finalise_kernel(double* __restrict__ part, const int* __restrict__ lens_a, int La, int M, int slices, int blocks,
                                                             int polarity, double* __restrict__ c, double* __restrict__ best_v, int* __restrict__ best_l) {
  __shared__ double sv[256];
  __shared__ int sl[256];
  const int b = blockIdx.y, t = threadIdx.x;
  const long long W = 2LL * M + 1;
  const long long idx = (long long)blockIdx.x * PICK + t;
  const int ns = slices_of(fd_clip_len(lens_a, b, La));
  double v = -HUGE_VAL;
  int l = INT_MAX;                          // loses every tie against a real lag
  if (idx < W) {
    double* __restrict__ p = part + (size_t)b * slices * (size_t)W + idx;
    double s = 0.0;
    for (int j = 0; j < ns; ++j) s += p[(size_t)j * W];
    p[0] = s;
    if (c) c[(size_t)b * W + idx] = s;
    const double m = polarity ? fabs(s) : s;
    v = m != m ? -HUGE_VAL : m;
    l = (int)(idx - M);
  }
  block_best(v, l, sv, sl);
  if (t == 0) { best_v[(size_t)b * blocks + blockIdx.x] = v; best_l[(size_t)b * blocks + blockIdx.x] = l; }
}

__global__ __launch_bounds__(256) void xcorr_pick_kernel(const double* __restrict__ best_v, const int* __restrict__ best_l, int blocks, int* __restrict__ lags) {
  __shared__ double sv[256];
  __shared__ int sl[256];
  const int b = blockIdx.x;
  double v = -HUGE_VAL;
  int l = INT_MAX;
  for (int i = threadIdx.x; i < blocks; i += 256) {
    const double vi = best_v[(size_t)b * blocks + i];
    const int li = best_l[(size_t)b * blocks + i];
    if (better(vi, li, v, l)) { v = vi; l = li; }
  }
  block_best(v, l, sv, sl);
  if (threadIdx.x == 0) lags[b] = l;
}

// ---- fd_xcorr_lags_frac: the peak on a grid of 1 / Q samples, with polarity (align.py refine_lag) -----------------------------------------
// One workgroup per clip: l0 from the workgroups' winners (xcorr_pick_kernel's reduction), the sign of c[l0], then the 2 Q - 1 candidates
// q of refine_lag from the finished c (part[b][0][.]) and the bank [Q][2 taps]: r(q) = sum_k (sign c[l0 + floor(q / Q) + k]) H[q mod Q][k],
// k ascending, every product and sum rounded on its own (no contraction), indices outside [-M, M] left out, NaN as -inf; the best by
// `better` (a total order on (r, q): any grouping finds the same q).  A candidate is one thread's own chain, so nothing depends on B.
__global__ __launch_bounds__(256) void xcorr_refine_kernel(const double* __restrict__ part, const double* __restrict__ best_v, const int* __restrict__ best_l,
                                                           int slices, int blocks, int M, const double* __restrict__ bank, int Q, int taps, int polarity,
                                                           long long* __restrict__ lag_q, int* __restrict__ sign) {
#pragma clang fp contract(off)
  __shared__ double sv[256];
  __shared__ int sl[256];
  const int b = blockIdx.x, t = threadIdx.x;
  double v = -HUGE_VAL;
  int l0 = INT_MAX;
  for (int i = t; i < blocks; i += 256) {
    const double vi = best_v[(size_t)b * blocks + i];
    const int li = best_l[(size_t)b * blocks + i];
    if (better(vi, li, v, l0)) { v = vi; l0 = li; }
  }
  block_best(v, l0, sv, sl);
  __syncthreads();                                              // sv[0] / sl[0] have been read by every thread
  l0 = l0 < -M ? -M : (l0 > M ? M : l0);                        // (always inside; clamped so that no table can lead outside the row)
  const long long W = 2LL * M + 1;
  const double* __restrict__ c = part + (size_t)b * slices * (size_t)W + M;      // c[l], l in [-M, M]
  const double sg = (polarity && c[l0] < 0.0) ? -1.0 : 1.0;
  const long long edge = (long long)M * Q;
  double rv = -HUGE_VAL;
  int rq = INT_MAX;                                             // loses every tie against a real candidate
  for (int i = t; i < 2 * Q - 1; i += 256) {
    const int q = i - (Q - 1);
    const long long lq = (long long)l0 * Q + q;
    if (lq > edge || lq < -edge) continue;                      // |l0 + q / Q| > M
    const int fl = q < 0 ? -1 : 0, j = q - fl * Q;              // floor(q / Q), q mod Q
    const double* __restrict__ h = bank + (size_t)j * (2 * taps);
    double r = 0.0;
    for (int k = 0; k < 2 * taps; ++k) {
      const long long l = (long long)l0 + fl + k - taps + 1;
      if (l >= -M && l <= M) {
        const double p = (sg * c[l]) * h[k];
        r = r + p;
      }
    }
    if (r != r) r = -HUGE_VAL;
    if (better(r, q, rv, rq)) { rv = r; rq = q; }
  }
  block_best(rv, rq, sv, sl);
  if (t == 0) {
    lag_q[b] = (long long)l0 * Q + (rq == INT_MAX ? 0 : rq);
    sign[b] = sg < 0.0 ? -1 : 1;
  }
}

struct xcorr_layout { size_t part, best_v, best_l, total; int slices, tiles, blocks; };

inline bool args_ok(int B, int La, int Lb, int max_lag) {
  return B > 0 && B <= 65535 && max_lag >= 1 && max_lag <= MAX_LAG_CAP && La > 0 && La <= MAX_ROW && Lb > 0 && Lb <= MAX_ROW;
}

xcorr_layout layout(int B, int La, int max_lag) {
  xcorr_layout s;
  const size_t W = 2 * (size_t)max_lag + 1;
  s.slices = slices_of(La);
  s.tiles = (int)((W + LAG_TILE - 1) / LAG_TILE);
  s.blocks = (int)((W + PICK - 1) / PICK);
  s.part = fd_align(sizeof(double) * (size_t)B * s.slices * W);
  s.best_v = fd_align(sizeof(double) * (size_t)B * s.blocks);
  s.best_l = fd_align(sizeof(int) * (size_t)B * s.blocks);
  s.total = s.part + s.best_v + s.best_l;
  return s;
}

struct xcorr_front { xcorr_layout s; hipStream_t st; double* part; double* best_v; int* best_l; };

// What fd_xcorr_lags and fd_xcorr_lags_frac (`who`) share: the checks of the batch (and of grid = {Q, W}, fractional only), the carve-up
// of the workspace (`ws_fn` sizes it), the slice sums and the finalise kernel.  The entry point adds its own last kernel.
// The Q / W checks sit here, behind the batch checks and ahead of the workspace check, and not in fd_xcorr_lags_frac ahead of the call:
// that is the order a caller with several bad arguments has always been answered in.
int front(const char* who, const char* ws_fn, const float* a, const float* b, const int* lens_a, const int* lens_b, int B, int La, int Lb, int max_lag,
          const int* grid, int polarity, double* c, void* ws, size_t ws_bytes, void* stream, xcorr_front* f) {
  FD_REQUIRE(B > 0 && B <= 65535, "%s: bad batch B %d (1 <= B <= 65535)", who, B);
  FD_REQUIRE(max_lag >= 1 && max_lag <= MAX_LAG_CAP, "%s: bad max_lag %d (1 <= max_lag <= %d)", who, max_lag, MAX_LAG_CAP);
  FD_REQUIRE(La > 0 && La <= MAX_ROW && Lb > 0 && Lb <= MAX_ROW, "%s: bad row lengths La %d Lb %d (1 <= La, Lb <= %d)", who, La, Lb, MAX_ROW);
  if (grid) {
    FD_REQUIRE(grid[0] >= 2 && grid[0] <= 1024, "%s: bad grid Q %d (2 <= Q <= 1024 steps per sample)", who, grid[0]);
    FD_REQUIRE(grid[1] >= 1 && grid[1] <= 256, "%s: bad half width W %d (1 <= W <= 256: 2 W taps)", who, grid[1]);
  }
  f->s = layout(B, La, max_lag);
  const size_t need = f->s.total + 256;
  if (ws_bytes < need) return fd_set_error(FD_ENOMEM, "%s: workspace %zu < required %zu bytes (%s)", who, ws_bytes, need, ws_fn);
  f->st = fd_stream(stream);
  char* base = aligned(ws);
  f->part = reinterpret_cast<double*>(base);
  f->best_v = reinterpret_cast<double*>(base + f->s.part);
  f->best_l = reinterpret_cast<int*>(base + f->s.part + f->s.best_v);
  hipLaunchKernelGGL(xcorr_slice_kernel, dim3(f->s.slices, f->s.tiles, B), dim3(256), 0, f->st, a, b, lens_a, lens_b, La, Lb, max_lag, f->s.slices, f->part);
  hipLaunchKernelGGL(xcorr_finalise_kernel, dim3(f->s.blocks, B), dim3(256), 0, f->st, f->part, lens_a, La, max_lag, f->s.slices, f->s.blocks, polarity, c,
                     f->best_v, f->best_l);
  return FD_OK;
}

}  // namespace

extern "C" size_t fd_xcorr_workspace_bytes(int B, int La, int Lb, int max_lag) {
  if (!args_ok(B, La, Lb, max_lag)) return 0;
  return layout(B, La, max_lag).total + 256;    // (the entry point aligns the base itself)
}

extern "C" int fd_xcorr_lags(const float* a, const float* b, const int* lens_a, const int* lens_b, int B, int La, int Lb, int max_lag, double* c,
                             int* lags, void* ws, size_t ws_bytes, void* stream) {
  FD_REQUIRE(a && b && lens_a && lens_b && lags && ws, "fd_xcorr_lags: null pointer");
  xcorr_front f;
  FD_TRY(front("fd_xcorr_lags", "fd_xcorr_workspace_bytes", a, b, lens_a, lens_b, B, La, Lb, max_lag, nullptr, 0, c, ws, ws_bytes, stream, &f));
  hipLaunchKernelGGL(xcorr_pick_kernel, dim3(B), dim3(256), 0, f.st, f.best_v, f.best_l, f.s.blocks, lags);
  FD_LAUNCH_CHECK();
  return FD_OK;
}

extern "C" size_t fd_xcorr_frac_workspace_bytes(int B, int La, int Lb, int max_lag) { return fd_xcorr_workspace_bytes(B, La, Lb, max_lag); }

extern "C" int fd_xcorr_lags_frac(const float* a, const float* b, const int* lens_a, const int* lens_b, int B, int La, int Lb, int max_lag,
                                  const double* bank, int Q, int W, int polarity, double* c, long long* lag_q, int* sign, void* ws, size_t ws_bytes,
                                  void* stream) {
  FD_REQUIRE(a && b && lens_a && lens_b && lag_q && sign && ws, "fd_xcorr_lags_frac: null pointer");
  FD_REQUIRE(bank, "fd_xcorr_lags_frac: null bank (DEVICE double [Q][2 W], align.frac_bank)");
  const int grid[2] = {Q, W};
  xcorr_front f;
  FD_TRY(front("fd_xcorr_lags_frac", "fd_xcorr_frac_workspace_bytes", a, b, lens_a, lens_b, B, La, Lb, max_lag, grid, polarity ? 1 : 0, c, ws, ws_bytes, stream,
               &f));
  hipLaunchKernelGGL(xcorr_refine_kernel, dim3(B), dim3(256), 0, f.st, f.part, f.best_v, f.best_l, f.s.slices, f.s.blocks, max_lag, bank, Q, W, polarity ? 1 : 0,
                     lag_q, sign);
  FD_LAUNCH_CHECK();
  return FD_OK;
}
