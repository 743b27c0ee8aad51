// loudness.hip -- integrated loudness after ITU-R BS.1770-4 / EBU R 128 of a ragged batch of mono signals at 48 kHz (include/flowdec_hip.h
// "Loudness"; host yardstick and the definition: flowdec_amd/loudness.py).  eval_cli --loudness / --match-loudness and loudness.LoudnessMeter
// run on it.  The K-weighting is a recursive filter (two biquads), the only one in this library: every sample depends on all earlier ones,
// so the order of operations below IS the definition, and the yardstick follows it operation for operation.
//
// The step (transposed direct form II, the two stages in cascade; every product, sum and difference rounded to float64 on its own: the
// pragma below; the products by the second stage's b0 = b2 = 1 are exact and left out):
//     y  = B0 x + s1        s1' = (B1 x - A1 y) + s2        s2' = B2 x - A2 y
//     z  = y + s3           s3' = (D1 y - C1 z) + s4        s4' = y - C2 z
// The signal is cut into sub-blocks of 4800 samples (100 ms) from its sample 0 and every sub-block into 64 chunks of 75 samples; only
// whole sub-blocks are read.  With Mc / Ms the zero-input transitions over 75 / 4800 samples (column i: the step run that many times on
// the unit state i with x = 0; tabulated on the host, fd_loudness_tables) and  e + M s  meaning  e_i + (((M_i0 s_0 + M_i1 s_1) + M_i2 s_2) +
// M_i3 s_3):
//   pass A   (one wave per sub-block j, one lane per chunk k)  e_jk = the state after the chunk's 75 steps from the zero state;
//            T_j = t_64 of  t_0 = 0, t_{k+1} = e_jk + Mc t_k                     (the sub-block's end state from the zero state)
//   carry    (one wave per clip)                               S_0 = the caller's state or 0,  S_{j+1} = T_j + Ms S_j
//   pass B   (one wave per sub-block, one lane per chunk)      s_j0 = S_j, s_{j,k+1} = e_jk + Mc s_jk;  the chunk runs its 75 steps again
//            from s_jk and adds z z in ascending sample order (from 0.0); E[j] = the 64 chunk sums added in ascending k.
// Nothing per sample is written to memory: 2 KB of chunk states per 19 KB sub-block.  A wave stages its 4800 samples in LDS with coalesced
// loads; lane k then reads words 75 k + i, and 75 is odd, so the 64 lanes fall into 64 different banks.  The carry is the only sequential
// part: 10 steps a second of signal.
//
// The gates (fd_loudness_gate; one wave per clip): block j = sub-blocks j..j+3, ms_j = (((E[j] + E[j+1]) + E[j+2]) + E[j+3]) / 19200.
// A sum over blocks is taken as 64 lane sums (lane l adds its blocks l, l + 64, ... in ascending order to 0.0) added in ascending l.
// sum1, n1 over ms_j > ABS_GATE;  thr = 0.1 (sum1 / n1);  sum2, n2 over ms_j > ABS_GATE and ms_j > thr;  ms_gated = sum2 / n2.
// Fewer than 4 sub-blocks: NaN, counts 0 0 0.  A block that is not finite: NaN, counts (blocks, 0, 0).  n1 = 0: 0.0 (-inf LUFS).
// float64 subnormals are kept by the hardware (a burst followed by digital silence runs the state through them): no special casing.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int SUB = 4800;                 // samples per sub-block (100 ms at 48 kHz)
constexpr int CH = 75;                    // samples per chunk (one lane)
constexpr int NCH = SUB / CH;             // 64 chunks per sub-block (one wave)
constexpr int MAX_ROW = 0x7fffffff - 1024;
static_assert(NCH == 64 && NCH * CH == SUB, "one wave per sub-block");

// BS.1770-4 Table 1 (shelf) and Table 2 (high-pass) at 48 kHz
constexpr double B0 = 1.53512485958697, B1 = -2.69169618940638, B2 = 1.19839281085285, A1 = -1.69065929318241, A2 = 0.73248077421585;
constexpr double D1 = -2.0, C1 = -1.99004745483398, C2 = 0.99007225036621;
constexpr double ABS_GATE = 1.1724653045822981e-07;   // 10^((-70 + 0.691) / 10), the float64 loudness.py computes (pinned there)
constexpr double BLOCK_SAMPLES = 19200.0;

struct Mat4 {
  double m[16];   // row-major
};

__host__ __device__ __forceinline__ double kstep(double x, double (&s)[4]) {
  const double p = B0 * x;
  const double y = p + s[0];
  const double q1 = B1 * x;
  const double q2 = A1 * y;
  const double r = q1 - q2;
  const double n1 = r + s[1];
  const double u1 = B2 * x;
  const double u2 = A2 * y;
  const double n2 = u1 - u2;
  const double z = y + s[2];
  const double v1 = D1 * y;
  const double v2 = C1 * z;
  const double w = v1 - v2;
  const double n3 = w + s[3];
  const double g = C2 * z;
  const double n4 = y - g;
  s[0] = n1; s[1] = n2; s[2] = n3; s[3] = n4;
  return z;
}

// s <- e + M s
__device__ __forceinline__ void advance(const Mat4& M, const double* e, double (&s)[4]) {
  double n[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    double a = M.m[4 * i] * s[0];
    double c = M.m[4 * i + 1] * s[1];
    a = a + c;
    c = M.m[4 * i + 2] * s[2];
    a = a + c;
    c = M.m[4 * i + 3] * s[3];
    a = a + c;
    n[i] = e[i] + a;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) s[i] = n[i];
}

void transition(int steps, Mat4* M) {
  for (int col = 0; col < 4; ++col) {
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    s[col] = 1.0;
    for (int i = 0; i < steps; ++i) kstep(0.0, s);
    for (int r = 0; r < 4; ++r) M->m[4 * r + col] = s[r];
  }
}

struct Tables {
  Mat4 chunk, sub;
  Tables() {
    transition(CH, &chunk);
    transition(SUB, &sub);
  }
};
const Tables& tables() {
  static const Tables t;
  return t;
}

__device__ __forceinline__ int clip_nsub(const int* lengths, int b, int L) {
  int len = lengths[b];
  len = len < 0 ? 0 : (len > L ? L : len);
  return len / SUB;
}

__device__ __forceinline__ void stage_tile(float* tile, const float* __restrict__ x, int b, int L, int j, int t) {
  const float* __restrict__ src = x + (size_t)b * L + (size_t)j * SUB;
  for (int i = t; i < SUB; i += NCH) tile[i] = src[i];
}

__global__ __launch_bounds__(NCH) void loud_pass_a(const float* __restrict__ x, const int* __restrict__ lengths, int L, int J, Mat4 Mc,
                                                   double* __restrict__ e_ws, double* __restrict__ T_ws) {
  __shared__ float tile[SUB];
  __shared__ double es[NCH][4];
  const int b = blockIdx.y, j = blockIdx.x, t = threadIdx.x;
  if (j >= clip_nsub(lengths, b, L)) return;
  stage_tile(tile, x, b, L, j, t);
  __syncthreads();
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = 0; i < CH; ++i) kstep((double)tile[t * CH + i], s);
  const size_t sb = (size_t)b * J + j;
  double* __restrict__ eo = e_ws + (sb * NCH + t) * 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    es[t][i] = s[i];
    eo[i] = s[i];
  }
  __syncthreads();
  if (t == 0) {
    double u[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < NCH; ++k) advance(Mc, es[k], u);
#pragma unroll
    for (int i = 0; i < 4; ++i) T_ws[sb * 4 + i] = u[i];
  }
}

__global__ __launch_bounds__(NCH) void loud_carry(const int* __restrict__ lengths, int L, int J, Mat4 Ms, const double* __restrict__ T_ws,
                                                  double* __restrict__ S_ws, double* state, int* __restrict__ nsub_out) {
  __shared__ double Ts[NCH][4];
  const int b = blockIdx.x, t = threadIdx.x;
  const int nsub = clip_nsub(lengths, b, L);
  double S[4] = {0.0, 0.0, 0.0, 0.0};
  if (state) {
#pragma unroll
    for (int i = 0; i < 4; ++i) S[i] = state[(size_t)b * 4 + i];
  }
  for (int j0 = 0; j0 < nsub; j0 += NCH) {
    const int jj = j0 + t;
    if (jj < nsub) {
#pragma unroll
      for (int i = 0; i < 4; ++i) Ts[t][i] = T_ws[((size_t)b * J + jj) * 4 + i];
    }
    __syncthreads();
    const int cnt = nsub - j0 < NCH ? nsub - j0 : NCH;
    double mine[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < cnt; ++k) {
      if (k == t) {
#pragma unroll
        for (int i = 0; i < 4; ++i) mine[i] = S[i];
      }
      advance(Ms, Ts[k], S);
    }
    if (jj < nsub) {
#pragma unroll
      for (int i = 0; i < 4; ++i) S_ws[((size_t)b * J + jj) * 4 + i] = mine[i];
    }
    __syncthreads();
  }
  if (t == 0) {
    nsub_out[b] = nsub;
    if (state) {
#pragma unroll
      for (int i = 0; i < 4; ++i) state[(size_t)b * 4 + i] = S[i];
    }
  }
}

__global__ __launch_bounds__(NCH) void loud_pass_b(const float* __restrict__ x, const int* __restrict__ lengths, int L, int J, Mat4 Mc,
                                                   const double* __restrict__ e_ws, const double* __restrict__ S_ws, double* __restrict__ E) {
  __shared__ float tile[SUB];
  __shared__ double es[NCH][4];
  __shared__ double ps[NCH];
  const int b = blockIdx.y, j = blockIdx.x, t = threadIdx.x;
  const size_t sb = (size_t)b * J + j;
  if (j >= clip_nsub(lengths, b, L)) {
    if (t == 0) E[sb] = 0.0;
    return;
  }
  stage_tile(tile, x, b, L, j, t);
  double s[4], mine[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    es[t][i] = e_ws[(sb * NCH + t) * 4 + i];
    s[i] = S_ws[sb * 4 + i];
  }
  __syncthreads();
  for (int k = 0; k < NCH; ++k) {
    if (k == t) {
#pragma unroll
      for (int i = 0; i < 4; ++i) mine[i] = s[i];
    }
    advance(Mc, es[k], s);
  }
  double acc = 0.0;
  for (int i = 0; i < CH; ++i) {
    const double z = kstep((double)tile[t * CH + i], mine);
    const double zz = z * z;
    acc = acc + zz;
  }
  ps[t] = acc;
  __syncthreads();
  if (t == 0) {
    double sum = ps[0];
    for (int k = 1; k < NCH; ++k) sum = sum + ps[k];
    E[sb] = sum;
  }
}

__device__ __forceinline__ double block_ms(const double* __restrict__ e, int j) {
  double a = e[j] + e[j + 1];
  a = a + e[j + 2];
  a = a + e[j + 3];
  return a / BLOCK_SAMPLES;
}

// the 64 lane sums added in ascending lane order, the counts and flags added up; every lane gets the totals
__device__ __forceinline__ void lanes_total(double* pa, int* pc, int* pb, int t, double acc, int cnt, int bad, double* sum, int* n, int* anybad) {
  __syncthreads();
  pa[t] = acc; pc[t] = cnt; pb[t] = bad;
  __syncthreads();
  double a = pa[0];
  int c = pc[0], f = pb[0];
  for (int l = 1; l < NCH; ++l) {
    a = a + pa[l];
    c += pc[l];
    f |= pb[l];
  }
  *sum = a; *n = c; *anybad = f;
}

__global__ __launch_bounds__(NCH) void loud_gate(const double* __restrict__ E, const int* __restrict__ nsub, int J, double* __restrict__ ms_out,
                                                 int* __restrict__ counts_out) {
  __shared__ double pa[NCH];
  __shared__ int pc[NCH], pb[NCH];
  const int b = blockIdx.x, t = threadIdx.x;
  int ns = nsub[b];
  ns = ns < 0 ? 0 : (ns > J ? J : ns);
  const int nblk = ns >= 4 ? ns - 3 : 0;
  const double* __restrict__ e = E + (size_t)b * J;
  const double nan = __builtin_nan("");
  double acc = 0.0, sum1, sum2;
  int cnt = 0, bad = 0, n1, n2, anybad;
  for (int j = t; j < nblk; j += NCH) {
    const double m = block_ms(e, j);
    if (!(m - m == 0.0)) bad = 1;             // NaN or Inf
    if (m > ABS_GATE) {
      acc = acc + m;
      ++cnt;
    }
  }
  lanes_total(pa, pc, pb, t, acc, cnt, bad, &sum1, &n1, &anybad);
  double ms = nan;
  int c1 = 0, c2 = 0;
  if (nblk > 0 && !anybad) {
    if (n1 == 0) {
      ms = 0.0;
    } else {
      const double mean1 = sum1 / (double)n1;
      const double thr = 0.1 * mean1;
      acc = 0.0;
      cnt = 0;
      for (int j = t; j < nblk; j += NCH) {
        const double m = block_ms(e, j);
        if (m > ABS_GATE && m > thr) {
          acc = acc + m;
          ++cnt;
        }
      }
      lanes_total(pa, pc, pb, t, acc, cnt, 0, &sum2, &n2, &anybad);
      ms = sum2 / (double)n2;
      c1 = n1;
      c2 = n2;
    }
  }
  if (t == 0) {
    ms_out[b] = ms;
    counts_out[3 * b] = nblk;
    counts_out[3 * b + 1] = c1;
    counts_out[3 * b + 2] = c2;
  }
}

struct Layout {
  size_t e, T, S, E, nsub, total;   // byte offsets into the workspace
};

bool layout(int B, int L, Layout* lo) {
  if (B <= 0 || B > 65535 || L <= 0 || L > MAX_ROW) return false;
  const size_t sb = (size_t)B * (size_t)(L / SUB);
  lo->e = 0;
  lo->T = lo->e + sb * NCH * 4 * sizeof(double);
  lo->S = lo->T + sb * 4 * sizeof(double);
  lo->E = lo->S + sb * 4 * sizeof(double);
  lo->nsub = lo->E + sb * sizeof(double);
  lo->total = lo->nsub + (((size_t)B * sizeof(int) + 255) / 256) * 256;
  return true;
}

int check_shape(const char* who, int B, int L) {
  FD_REQUIRE(B > 0 && B <= 65535, "%s: bad batch B %d (1 <= B <= 65535)", who, B);
  FD_REQUIRE(L > 0 && L <= MAX_ROW, "%s: bad row length L %d (1 <= L <= %d)", who, L, MAX_ROW);
  return FD_OK;
}

int check_ws(const char* who, const Layout& lo, const void* ws, size_t ws_bytes) {
  FD_REQUIRE(ws, "%s: null pointer (ws)", who);
  FD_REQUIRE(((uintptr_t)ws & 7) == 0, "%s: the workspace must be 8-byte aligned", who);
  if (ws_bytes < lo.total) return fd_set_error(FD_ENOMEM, "%s: workspace too small (%zu bytes, fd_loudness_workspace_bytes gives %zu)", who, ws_bytes, lo.total);
  return FD_OK;
}

int launch_energies(const float* x, const int* lengths, int B, int L, double* state, double* E, int* nsub, const Layout& lo, void* ws, hipStream_t st) {
  const int J = L / SUB;
  char* w = static_cast<char*>(ws);
  double* e_ws = reinterpret_cast<double*>(w + lo.e);
  double* T_ws = reinterpret_cast<double*>(w + lo.T);
  double* S_ws = reinterpret_cast<double*>(w + lo.S);
  const Tables& tb = tables();
  if (J > 0) {
    hipLaunchKernelGGL(loud_pass_a, dim3(J, B), dim3(NCH), 0, st, x, lengths, L, J, tb.chunk, e_ws, T_ws);
    FD_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(loud_carry, dim3(B), dim3(NCH), 0, st, lengths, L, J, tb.sub, T_ws, S_ws, state, nsub);
  FD_LAUNCH_CHECK();
  if (J > 0) {
    hipLaunchKernelGGL(loud_pass_b, dim3(J, B), dim3(NCH), 0, st, x, lengths, L, J, tb.chunk, e_ws, S_ws, E);
    FD_LAUNCH_CHECK();
  }
  return FD_OK;
}

}  // namespace

extern "C" int fd_loudness_tables(double* chunk16, double* sub16, double* abs_gate) {
  FD_REQUIRE(chunk16 && sub16 && abs_gate, "fd_loudness_tables: null pointer");
  const Tables& tb = tables();
  for (int i = 0; i < 16; ++i) {
    chunk16[i] = tb.chunk.m[i];
    sub16[i] = tb.sub.m[i];
  }
  *abs_gate = ABS_GATE;
  return FD_OK;
}

extern "C" size_t fd_loudness_workspace_bytes(int B, int L) {
  Layout lo;
  return layout(B, L, &lo) ? lo.total : 0;
}

extern "C" int fd_loudness_energies(const float* x, const int* lengths, int B, int L, double* state, double* E_out, int* nsub_out, void* ws, size_t ws_bytes,
                                    void* stream) {
  FD_REQUIRE(x && lengths && nsub_out, "fd_loudness_energies: null pointer");
  FD_TRY(check_shape("fd_loudness_energies", B, L));
  FD_REQUIRE(E_out || L < SUB, "fd_loudness_energies: null pointer (E_out; it may be NULL only when L < %d leaves it no column)", SUB);
  Layout lo;
  layout(B, L, &lo);
  FD_TRY(check_ws("fd_loudness_energies", lo, ws, ws_bytes));
  return launch_energies(x, lengths, B, L, state, E_out, nsub_out, lo, ws, fd_stream(stream));
}

extern "C" int fd_loudness_gate(const double* E, const int* nsub, int B, int Jmax, double* ms_out, int* counts_out, void* stream) {
  FD_REQUIRE(nsub && ms_out && counts_out, "fd_loudness_gate: null pointer");
  FD_REQUIRE(B > 0 && B <= 65535, "fd_loudness_gate: bad batch B %d (1 <= B <= 65535)", B);
  FD_REQUIRE(Jmax >= 0 && Jmax <= MAX_ROW / SUB, "fd_loudness_gate: bad sub-block count Jmax %d (0 <= Jmax <= %d)", Jmax, MAX_ROW / SUB);
  FD_REQUIRE(E || Jmax == 0, "fd_loudness_gate: null pointer (E; it may be NULL only when Jmax is 0)");
  hipLaunchKernelGGL(loud_gate, dim3(B), dim3(NCH), 0, fd_stream(stream), E, nsub, Jmax, ms_out, counts_out);
  FD_LAUNCH_CHECK();
  return FD_OK;
}

extern "C" int fd_loudness(const float* x, const int* lengths, int B, int L, double* ms_out, int* counts_out, void* ws, size_t ws_bytes, void* stream) {
  FD_REQUIRE(x && lengths && ms_out && counts_out, "fd_loudness: null pointer");
  FD_TRY(check_shape("fd_loudness", B, L));
  Layout lo;
  layout(B, L, &lo);
  FD_TRY(check_ws("fd_loudness", lo, ws, ws_bytes));
  char* w = static_cast<char*>(ws);
  double* E = reinterpret_cast<double*>(w + lo.E);
  int* nsub = reinterpret_cast<int*>(w + lo.nsub);
  FD_TRY(launch_energies(x, lengths, B, L, nullptr, E, nsub, lo, ws, fd_stream(stream)));
  hipLaunchKernelGGL(loud_gate, dim3(B), dim3(NCH), 0, fd_stream(stream), (const double*)E, (const int*)nsub, L / SUB, ms_out, counts_out);
  FD_LAUNCH_CHECK();
  return FD_OK;
}
