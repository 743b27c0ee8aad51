// ndac_pool.hip -- one native step for a pool of NDAC streaming sessions (include/flowdec_hip.h "Codec pools"; flowdec_amd/ndac_pool.py).
// A step is ONE device table (fd_ndac_pool_row, an entry per row of the call) and a fixed chain of launches whatever the number of rows:
//   decode  pool_decode_gather_kernel (code rings -> z_q [B][latent][T], from_codes fused in, per-row nq; the device frame table)
//           -> the decoder walk of fd_ndac_decode_ragged under that table -> pool_decode_emit_kernel (the final samples of every row -> out)
//   encode  pool_encode_gather_kernel (sample rings -> x [B][T * hop]; the frame table) -> the encoder walk and the quantiser of
//           fd_ndac_encode_ragged with the call's n_quantizers -> pool_encode_emit_kernel (the first nq_b code rows of the final frames)
// Every check runs on the HOST copy of the table before anything is launched; nothing is copied back and the stream is never waited for.
// The chain is linear, so with use_graph it is captured once per (direction, B, T, n_quantizers, precision, table, workspace) -- after one
// eager call with that key -- and replayed: the table's CONTENT (rings, windows, outputs) is read by the kernels at run time and is not
// part of the graph.  No atomics.  What the device table steers is clamped into the rows of the workspace: a device table that differs
// from the checked host copy gives wrong values, never an access outside the workspace.  (The ring and out pointers are the caller's.)
#include <map>
#include <set>
#include <tuple>

#include "align.h"
#include "ndac_internal.h"

namespace {

struct PoolCodebooks {   // what the decode gather takes of the codec
  const float* const* wout; const float* const* bout; const float* const* cb;   // DEVICE arrays [n_codebooks] of device pointers (rvq_from_codes_kernel's)
  int latent_dim, codebook_size, codebook_dim, n_codebooks;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// grid (x, B), grid-stride over the row's latent_dim * T elements.  z_q[b][c][t] = sum_{q < nq_b} term_q(code ring of row b at frame
// start_b + t), q ascending, f32 adds: the arithmetic of rvq_from_codes_kernel on the row alone.  Columns at and behind frames_b are 0
// (the walk never reads them).  Frame i of code row q lives at ring[q * ring_cap + i % ring_cap]: the window may wrap.
__global__ __launch_bounds__(256) void pool_decode_gather_kernel(const fd_ndac_pool_row* __restrict__ table, PoolCodebooks v, float* __restrict__ zq,
                                                                 int* __restrict__ frames_out, int T) {
#pragma clang fp contract(off)
  const int b = blockIdx.y;
  const fd_ndac_pool_row r = table[b];
  const int cap = r.ring_cap < 1 ? 1 : r.ring_cap;
  const int frames = clampi(r.frames, 1, T < cap ? T : cap), nq = clampi(r.nq, 1, v.n_codebooks);
  if (blockIdx.x == 0 && threadIdx.x == 0) frames_out[b] = frames;
  const int* __restrict__ ring = (const int*)r.ring;
  long long s0 = r.start % cap;
  if (s0 < 0) s0 += cap;
  const int n = v.latent_dim * T;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const int c = i / T, t = i - c * T;
    float z = 0.f;
    if (t < frames) {
      long long k = s0 + t;
      if (k >= cap) k -= cap;
      for (int q = 0; q < nq; ++q) z = z + fd_rvq_code_term(v.cb[q], v.wout[q], v.bout[q], ring[(size_t)q * cap + k], v.codebook_size, v.codebook_dim, c);
    }
    zq[((size_t)b * v.latent_dim + c) * T + t] = z;
  }
}

// grid (x, B): out_b[i] = audio[b][emit_lo_b * up + i], i < emit_count_b * up (up = decoded samples per frame)
__global__ __launch_bounds__(256) void pool_decode_emit_kernel(const fd_ndac_pool_row* __restrict__ table, const float* __restrict__ audio, int Lo, int up) {
  const int b = blockIdx.y;
  const fd_ndac_pool_row r = table[b];
  const long long lo = (long long)(r.emit_lo < 0 ? 0 : r.emit_lo) * up;
  long long n = (long long)(r.emit_count < 0 ? 0 : r.emit_count) * up;
  if (lo + n > Lo) n = Lo - lo;
  float* __restrict__ out = (float*)r.out;
  for (long long i = blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) out[i] = audio[(size_t)b * Lo + lo + i];
}

// grid (x, B): x[b][i] = sample ring of row b at start_b + i for i < frames_b * hop, 0 behind (never read as data); the frame table
__global__ __launch_bounds__(256) void pool_encode_gather_kernel(const fd_ndac_pool_row* __restrict__ table, float* __restrict__ x, int* __restrict__ frames_out,
                                                                 int T, int hop) {
  const int b = blockIdx.y;
  const fd_ndac_pool_row r = table[b];
  const int cap = r.ring_cap < 1 ? 1 : r.ring_cap;
  const int fmax = cap / hop < T ? cap / hop : T;
  const int frames = clampi(r.frames, 1, fmax < 1 ? 1 : fmax);
  if (blockIdx.x == 0 && threadIdx.x == 0) frames_out[b] = frames;
  const float* __restrict__ ring = (const float*)r.ring;
  long long s0 = r.start % cap;
  if (s0 < 0) s0 += cap;
  const int L = T * hop, len = frames * hop <= cap ? frames * hop : 0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < L; i += gridDim.x * 256) {
    float val = 0.f;
    if (i < len) {
      long long k = s0 + i;
      if (k >= cap) k -= cap;
      val = ring[k];
    }
    x[(size_t)b * L + i] = val;
  }
}

// grid (x, B): out_b [nq_b][emit_count_b] = codes[b][q][emit_lo_b + j]   (codes: [B][nq_call][T] of the quantiser)
__global__ __launch_bounds__(256) void pool_encode_emit_kernel(const fd_ndac_pool_row* __restrict__ table, const int* __restrict__ codes, int nq_call, int T) {
  const int b = blockIdx.y;
  const fd_ndac_pool_row r = table[b];
  const int lo = clampi(r.emit_lo, 0, T), nq = clampi(r.nq, 0, nq_call);
  const int cnt = clampi(r.emit_count, 0, T - lo);
  int* __restrict__ out = (int*)r.out;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < nq * cnt; i += gridDim.x * 256) {
    const int q = i / cnt, j = i - q * cnt;
    out[i] = codes[((size_t)b * nq_call + q) * T + lo + j];
  }
}

// ---- the captured step --------------------------------------------------------------------------------------------------------------
struct PoolKey {     // everything a captured step bakes into its kernel arguments
  int dir = 0, B = 0, T = 0, nq = 0, precision = 0;
  const void *table = nullptr, *ws = nullptr;
  auto tie() const { return std::tie(dir, B, T, nq, precision, table, ws); }
  bool operator<(const PoolKey& o) const { return tie() < o.tie(); }
};
struct PoolState {
  std::map<PoolKey, hipGraphExec_t> graphs;
  std::set<PoolKey> seen;     // keys that ran once eagerly: a step is captured at its second sighting (as fdm::run_maybe_graph does)
};

template <typename Fn>
int run_step(fd_ndac* m, const PoolKey& key, bool use_graph, hipStream_t st, Fn&& enqueue) {
  if (!use_graph) return enqueue();
  if (!m->pool_state) m->pool_state = new PoolState();
  PoolState& ps = *static_cast<PoolState*>(m->pool_state);
  auto it = ps.graphs.find(key);
  if (it == ps.graphs.end()) {
    if (!ps.seen.count(key)) {
      if (ps.seen.size() >= 256) ps.seen.clear();
      ps.seen.insert(key);
      return enqueue();
    }
    if (ps.graphs.size() >= 64) {   // the key holds raw buffer pointers: bound the cache for callers that keep making pools
      FD_HIP(hipStreamSynchronize(st));   // (rare path) nothing captured earlier may still be in flight when it is destroyed
      for (auto& g : ps.graphs) (void)hipGraphExecDestroy(g.second);
      ps.graphs.clear();
    }
    hipGraph_t graph = nullptr;
    FD_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    const int rc = enqueue();
    const hipError_t e = hipStreamEndCapture(st, &graph);
    if (rc != FD_OK) { if (graph) (void)hipGraphDestroy(graph); return rc; }
    if (e != hipSuccess) return fd_set_error(FD_ERUNTIME, "hipStreamEndCapture failed: %s", hipGetErrorString(e));
    hipGraphExec_t exec = nullptr;
    FD_HIP(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
    (void)hipGraphDestroy(graph);
    it = ps.graphs.emplace(key, exec).first;
  }
  FD_HIP(hipGraphLaunch(it->second, st));
  return FD_OK;
}

// ---- workspace ----------------------------------------------------------------------------------------------------------------------
struct PoolLayout {
  size_t frames, zq, io, codes, walk, walk_bytes, total;   // byte offsets: frame table | z_q | audio (decode) / x (encode) | codes | the walk's own
  int Lo;                                                  // decoded samples of T frames
};
PoolLayout layout(const fd_ndac* m, int B, int T) {
  const fd_ndac_config& c = m->plan.cfg;
  PoolLayout p{};
  p.Lo = fd_ndac_decoded_length(m, T);
  const long long Lmax = (long long)T * m->plan.hop > p.Lo ? (long long)T * m->plan.hop : p.Lo;
  p.frames = 0;
  p.zq = fd_align(sizeof(int) * (size_t)B);
  p.io = p.zq + fd_align(sizeof(float) * (size_t)B * c.latent_dim * T);
  p.codes = p.io + fd_align(sizeof(float) * (size_t)B * Lmax);
  p.walk = p.codes + fd_align(sizeof(int) * (size_t)B * c.n_codebooks * T);
  p.walk_bytes = fd_ndac_workspace_bytes(m, B, (int)Lmax);
  p.total = p.walk + p.walk_bytes;
  return p;
}

// The checks of both calls, on the host copy of the table.  unit: ring elements per frame (decode 1, encode hop).
int check_table(const char* who, const fd_ndac_pool_row* h, int B, int T, int unit, int nq_max) {
  for (int b = 0; b < B; ++b) {
    const fd_ndac_pool_row& r = h[b];
    FD_REQUIRE(r.ring && r.out, "%s: row %d has a null ring or out pointer", who, b);
    FD_REQUIRE(r.frames >= 1 && r.frames <= T, "%s: row %d: frames = %d is outside [1, %d]", who, b, r.frames, T);
    FD_REQUIRE(r.start >= 0 && r.ring_cap >= 1 && (long long)r.frames * unit <= r.ring_cap, "%s: row %d: a window of %d frames from %lld does not fit a ring of %d",
               who, b, r.frames, r.start, r.ring_cap);
    FD_REQUIRE(r.nq >= 1 && r.nq <= nq_max, "%s: row %d: nq = %d is outside [1, %d]", who, b, r.nq, nq_max);
    FD_REQUIRE(r.emit_lo >= 0 && r.emit_count >= 0 && (long long)r.emit_lo + r.emit_count <= r.frames,
               "%s: row %d: the final frames [%d, %d + %d) leave the window of %d frames", who, b, r.emit_lo, r.emit_lo, r.emit_count, r.frames);
  }
  return FD_OK;
}

int grid_x(long long n) { return grid_for(n, 256, 256); }

}  // namespace

void fd_ndac_pool_state_free(void* state) {
  if (!state) return;
  PoolState* ps = static_cast<PoolState*>(state);
  for (auto& g : ps->graphs) (void)hipGraphExecDestroy(g.second);
  delete ps;
}

extern "C" size_t fd_ndac_pool_workspace_bytes(const fd_ndac* m, int B, int T) {
  if (!m || B <= 0 || T <= 0 || fd_ndac_check_ready(m, "fd_ndac_pool_workspace_bytes") != FD_OK) return 0;
  if ((long long)T * m->plan.hop >= (1ll << 31) / 4 || (long long)m->plan.cfg.latent_dim * T >= (1ll << 31)) return 0;
  return layout(m, B, T).total;
}

extern "C" int fd_ndac_pool_decode(fd_ndac* m, const fd_ndac_pool_row* table_dev, const fd_ndac_pool_row* table_host, int B, int T, void* ws,
                                   size_t ws_bytes, int use_graph, void* stream) {
  const char* who = "fd_ndac_pool_decode";
  FD_TRY(fd_ndac_check_ready(m, who));
  FD_REQUIRE(table_dev && table_host && ws && B > 0 && B <= 65535 && T > 0, "%s: bad arguments", who);
  int hl = 0, hr = 0;
  FD_TRY(fd_ndac_decode_halo(m, &hl, &hr));   // refuses odd decoder rates: the decoded length is then not frames * up
  const fd_ndac_config& c = m->plan.cfg;
  const PoolCodebooks v{m->d_wout, m->d_bout, m->d_cb, c.latent_dim, c.codebook_size, c.codebook_dim, c.n_codebooks};
  const size_t need = fd_ndac_pool_workspace_bytes(m, B, T);
  FD_REQUIRE(need, "%s: %d rows of %d frames are beyond the 32-bit indices of a step", who, B, T);
  if (ws_bytes < need) return fd_set_error(FD_ENOMEM, "%s: workspace %zu < required %zu bytes", who, ws_bytes, need);
  FD_TRY(check_table(who, table_host, B, T, 1, c.n_codebooks));
  const PoolLayout p = layout(m, B, T);
  const int up = p.Lo / T;
  FD_REQUIRE(up * T == p.Lo, "%s: the decoder makes %d samples of %d frames: no whole samples per frame", who, p.Lo, T);
  hipStream_t st = fd_stream(stream);
  char* base = (char*)ws;
  int* frames = (int*)(base + p.frames);
  float* zq = (float*)(base + p.zq);
  float* audio = (float*)(base + p.io);
  PoolKey key; key.dir = 0; key.B = B; key.T = T; key.precision = m->precision; key.table = table_dev; key.ws = ws;
  return run_step(m, key, use_graph != 0, st, [&]() -> int {
    hipLaunchKernelGGL(pool_decode_gather_kernel, dim3(grid_x((long long)c.latent_dim * T), B), dim3(256), 0, st, table_dev, v, zq, frames, T);
    FD_LAUNCH_CHECK();
    FD_TRY(fd_ndac_decode_walk(m, who, zq, frames, B, T, audio, base + p.walk, p.walk_bytes, st));
    hipLaunchKernelGGL(pool_decode_emit_kernel, dim3(grid_x(p.Lo), B), dim3(256), 0, st, table_dev, audio, p.Lo, up);
    FD_LAUNCH_CHECK();
    return FD_OK;
  });
}

extern "C" int fd_ndac_pool_encode(fd_ndac* m, const fd_ndac_pool_row* table_dev, const fd_ndac_pool_row* table_host, int B, int T, int n_quantizers,
                                   void* ws, size_t ws_bytes, int use_graph, void* stream) {
  const char* who = "fd_ndac_pool_encode";
  FD_TRY(fd_ndac_check_ready(m, who));
  FD_REQUIRE(table_dev && table_host && ws && B > 0 && B <= 65535 && T > 0, "%s: bad arguments", who);
  int hl = 0, hr = 0;
  FD_TRY(fd_ndac_encode_halo(m, &hl, &hr));   // refuses a rate of 1: n hops of samples are then not n frames
  const int hop = m->plan.hop, ncb = m->plan.cfg.n_codebooks;
  FD_REQUIRE(n_quantizers >= 1 && n_quantizers <= ncb, "%s: n_quantizers = %d but the model has %d codebooks", who, n_quantizers, ncb);
  const size_t need = fd_ndac_pool_workspace_bytes(m, B, T);
  FD_REQUIRE(need, "%s: %d rows of %d frames are beyond the 32-bit indices of a step", who, B, T);
  if (ws_bytes < need) return fd_set_error(FD_ENOMEM, "%s: workspace %zu < required %zu bytes", who, ws_bytes, need);
  FD_TRY(check_table(who, table_host, B, T, hop, n_quantizers));
  const PoolLayout p = layout(m, B, T);
  hipStream_t st = fd_stream(stream);
  char* base = (char*)ws;
  int* frames = (int*)(base + p.frames);
  float* zq = (float*)(base + p.zq);
  float* x = (float*)(base + p.io);
  int* codes = (int*)(base + p.codes);
  const int L = T * hop;
  PoolKey key; key.dir = 1; key.B = B; key.T = T; key.nq = n_quantizers; key.precision = m->precision; key.table = table_dev; key.ws = ws;
  return run_step(m, key, use_graph != 0, st, [&]() -> int {
    hipLaunchKernelGGL(pool_encode_gather_kernel, dim3(grid_x(L), B), dim3(256), 0, st, table_dev, x, frames, T, hop);
    FD_LAUNCH_CHECK();
    FD_TRY(fd_ndac_encode_walk(m, who, x, frames, B, L, n_quantizers, zq, codes, nullptr, base + p.walk, p.walk_bytes, st));
    hipLaunchKernelGGL(pool_encode_emit_kernel, dim3(grid_x((long long)n_quantizers * T), B), dim3(256), 0, st, table_dev, codes, n_quantizers, T);
    FD_LAUNCH_CHECK();
    return FD_OK;
  });
}
