// stream.hip -- the two device steps around fd_enhance_chunks in a streaming session pool (include/flowdec_hip.h "Streaming";
// flowdec_amd/stream.py).  Both are stateless, one launch per step whatever the number of sessions, and driven by ONE device table with
// an entry per row (fd_stream_row): fd_stream_gather assembles the rows of the model call from the sessions' input rings,
// fd_stream_emit writes what the call finished -- cross-faded against the tail each session carries -- and hands the next tail over.
// Every index a table can steer is clamped into the row it addresses: a wrong table gives wrong samples, never an access outside a
// row of y / x_hat.  (The pointers of the table -- ring, tails, out -- are the caller's, as everywhere in this ABI.)
#include "common.h"

namespace {

// One 1024-thread workgroup per row, as absmax_kernel (stft.hip): the row's maximum is complete when the workgroup ends, so the same
// launch can fold it into the session's running peak and write the row's factor -- a row split over workgroups would need a second
// pass (or a last-block election) for that.  A row of 256 frames is 98 303 floats: 96 per thread, microseconds beside the solve.
__global__ __launch_bounds__(1024) void stream_gather_kernel(const fd_stream_row* __restrict__ table, float* __restrict__ y, int Lrow,
                                                             float* __restrict__ peak, float* __restrict__ normfac) {
  const int b = blockIdx.x;
  const fd_stream_row r = table[b];
  const int cap = r.ring_cap < 1 ? 1 : r.ring_cap;
  int len = r.length < 0 ? 0 : r.length;
  if (len > Lrow) len = Lrow;
  if (len > cap) len = cap;                                  // (a row longer than its ring has no meaning; keeps k - cap below in [0, cap))
  long long s0 = r.start % cap;
  if (s0 < 0) s0 += cap;
  float* __restrict__ dst = y + (size_t)b * Lrow;
  float m = 0.f;
  for (int i = threadIdx.x; i < Lrow; i += 1024) {
    float v = 0.f;                                           // the row's tail [len, Lrow) is zero, as enhance_long leaves it
    if (i < len) {
      long long k = s0 + i;                                  // ring index = absolute sample mod capacity
      if (k >= cap) k -= cap;
      v = r.ring[k];
      m = fmaxf(m, fabsf(v));
    }
    dst[i] = v;
  }
  if (!peak) return;                                         // (uniform: a kernel argument)
  m = fd_wave_max(m);
  __shared__ float red[16];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    float p = peak[r.peak_slot];                             // one row per session per launch: nobody else touches this slot
    for (int i = 0; i < 16; ++i) p = fmaxf(p, red[i]);
    peak[r.peak_slot] = p;
    normfac[b] = (fabsf(p) <= 1e-8f) ? 1.0f : p;             // fd_normfac's rule (torch.isclose(., 0) with the default atol)
  }
}

// grid (ceil(Lrow / 256), B): thread i of row b writes finished sample i and, for i < xfade, sample i of the new tail.  The carried tail
// is READ and the new one WRITTEN in the same launch by different threads: the caller gives two distinct buffers (row parity).
__global__ __launch_bounds__(256) void stream_emit_kernel(const fd_stream_row* __restrict__ table, const float* __restrict__ x_hat, int Lrow,
                                                          const float* __restrict__ weights, int xfade) {
#pragma clang fp contract(off)   // a + w * (b - a) in three roundings, as stitch_kernel (solver_ops.hip): no fma
  const int b = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Lrow) return;
  const fd_stream_row r = table[b];
  const float* __restrict__ row = x_hat + (size_t)b * Lrow;
  auto at = [&](long long k) { return row[k < 0 ? 0 : (k >= Lrow ? Lrow - 1 : k)]; };
  const int count = r.emit_count > Lrow ? Lrow : r.emit_count;
  if (i < count) {
    const float vb = at((long long)r.emit_lo + i);
    float o = vb;
    if (r.tail_in && i < xfade) {                            // the finished range starts at (boundary - xfade / 2): its first xfade samples
      const float va = r.tail_in[i];
      const float d = vb - va;
      const float p = weights[i] * d;
      o = va + p;
    }
    r.out[i] = o;
  }
  if (r.tail_out && i < xfade) r.tail_out[i] = at((long long)r.tail_lo + i);
}

}  // namespace

extern "C" int fd_stream_gather(const fd_stream_row* table, int B, float* y, int L, float* peak, float* normfac_out, void* stream) {
  FD_REQUIRE(table && y && B > 0 && L > 0 && L <= 0x7fffffff - 1024, "fd_stream_gather: bad arguments");   // (the kernel's int index steps by 1024)
  FD_REQUIRE((peak == nullptr) == (normfac_out == nullptr), "fd_stream_gather: peak and normfac_out go together (both or neither)");
  hipLaunchKernelGGL(stream_gather_kernel, dim3(B), dim3(1024), 0, fd_stream(stream), table, y, L, peak, normfac_out);
  FD_LAUNCH_CHECK();
  return FD_OK;
}

extern "C" int fd_stream_emit(const fd_stream_row* table, int B, const float* x_hat, int L, const float* weights, int xfade, void* stream) {
  FD_REQUIRE(table && x_hat && B > 0 && B <= 65535 && L > 0 && L <= 0x7fffffff - 256, "fd_stream_emit: bad arguments");
  FD_REQUIRE(xfade >= 0 && xfade % 2 == 0 && xfade <= L && (xfade == 0 || weights), "fd_stream_emit: xfade must be even, at most L, and come with its weights");
  hipLaunchKernelGGL(stream_emit_kernel, dim3((unsigned)((L + 255) / 256), (unsigned)B), dim3(256), 0, fd_stream(stream), table, x_hat, L, weights, xfade);
  FD_LAUNCH_CHECK();
  return FD_OK;
}
