// ndac_internal.h -- what the codec's files share: the codec object itself (ndac.hip owns its life; ndac_rvq.hip and ndac_pool.hip read
// it), the direct convolution launchers (ndac_conv1d.hip), the quantiser runs (ndac_rvq.hip), the layer walks of the ragged entry points
// (ndac.hip, also ndac_pool.hip's) and the from_codes term.
#pragma once
#include <vector>

#include "internal.h"
#include "ndac_plan.h"

struct RvqQuant {         // one quantiser's parameters (device pointers)
  const float* win; const float* bin;     // [cd][D], [cd]
  const float* wout; const float* bout;   // [D][cd], [D]
  const float* cb;        // [J][cd] raw codebook
  const float* cbn;       // [J][cd] L2-normalised rows (host, the oracle's float32 operation order)
  const float* c2;        // [J] sum of squares of the normalised rows
};

struct fd_ndac {
  ndac::Plan plan;                       // structure, parameter table, layer records (device pointers resolved by fd_ndac_finalize)
  std::vector<std::vector<float>> host;  // per parameter: the values fd_ndac_set_param took, until finalize
  std::vector<float*> dev;               // per parameter: its device copy
  std::vector<void*> allocs;
  // per-codebook device pointer tables for rvq_from_codes_kernel
  const float** d_wout = nullptr; const float** d_bout = nullptr; const float** d_cb = nullptr;
  std::vector<RvqQuant> quant;           // per codebook: the pointers the RVQ kernels take
  const RvqQuant* d_quant = nullptr;     // the same table on the device (rvq_chain_kernel walks it)
  int precision = FD_NDAC_MFMA_DECODER;
  bool finalized = false;
  void* pool_state = nullptr;            // ndac_pool.hip's graph cache: created there on first use, released through fd_ndac_pool_state_free
};

inline int fd_ndac_check_ready(const fd_ndac* m, const char* who) {
  FD_REQUIRE(m, "%s: null codec", who);
  if (!m->finalized) return fd_set_error(FD_ESTATE, "%s: codec not finalised (call fd_ndac_finalize)", who);
  return FD_OK;
}
inline int fd_ndac_resolve_nq(const fd_ndac* m, int n_quantizers) {
  return n_quantizers <= 0 || n_quantizers > m->plan.cfg.n_codebooks ? m->plan.cfg.n_codebooks : n_quantizers;
}
// The frame table of a ragged call, checked on the host before anything is launched (B ints: one small copy and a synchronisation).
int fd_ndac_check_frames(const char* who, const int* frames, int B, int T, hipStream_t st);

// ndac_conv1d.hip: the direct (exact f32) kernels.  wt: weight layout, 0 = PyTorch's, 1 = [Ci][K][Co]; out_act = snake(result, alpha_out)
int fd_launch_conv1d(const float* x, const float* w, const float* bias, const float* alpha, const float* res, float* out, int B, int Ci, int T, int Co,
                     int K, int stride, int pad, int dil, int tanh_out, hipStream_t st, int wt = 0, float* out_act = nullptr,
                     const float* alpha_out = nullptr, fd_ndac_lens lens = {});
int fd_launch_convtr1d(const float* x, const float* w, const float* bias, const float* alpha, float* out, int B, int Ci, int T, int Co, int K, int stride,
                       int pad, hipStream_t st, int wt = 0, float* out_act = nullptr, const float* alpha_out = nullptr, fd_ndac_lens lens = {});

// ndac_rvq.hip: the chain of rvq_step_kernel launches (residual: z on entry, destroyed) / the one-launch chain where fd_rvq_chain_supported
// (z read-only).  frames (device int32 [B]) or nullptr: a step at or behind frames[b] is never read and gets code 0, z_q 0, latents 0.
int fd_rvq_run(fd_ndac* m, float* residual, const int* frames, int B, int T, int nq, float* zq, int* codes, float* latents, hipStream_t st);
int fd_rvq_run_chain(fd_ndac* m, const float* z, const int* frames, int B, int T, int nq, float* zq, int* codes, float* latents, hipStream_t st);

// ndac.hip: the decoder / encoder walk of fd_ndac_decode_ragged / fd_ndac_encode_ragged under a DEVICE frame table the caller vouches for
// (every entry in [1, T] resp. [1, L / hop]; frames == nullptr: dense): no copy to the host, no synchronisation.
// ws: fd_ndac_workspace_bytes(m, B, max(decoded length, T * hop)) resp. (m, B, L).  latents may be null.
int fd_ndac_decode_walk(fd_ndac* m, const char* who, const float* z, const int* frames, int B, int T, float* audio, void* ws, size_t ws_bytes, hipStream_t st);
int fd_ndac_encode_walk(fd_ndac* m, const char* who, const float* x, const int* frames, int B, int L, int n_quantizers, float* z_q, int* codes,
                        float* latents, void* ws, size_t ws_bytes, hipStream_t st);
void fd_ndac_pool_state_free(void* state);   // ndac_pool.hip

// One codebook's term of ResidualVectorQuantize.from_codes for latent channel c: f32( sum_d wout[c][d] cb[code][d] + bout[c] ), f64 inside,
// no fused multiply-add; the caller adds the terms in codebook order with f32 adds.  An index outside the codebook is clamped into it.
__device__ __forceinline__ float fd_rvq_code_term(const float* cb, const float* wout, const float* bout, int code, int J, int cd, int c) {
#pragma clang fp contract(off)
  code = code < 0 ? 0 : (code >= J ? J - 1 : code);
  const float* e = cb + (size_t)code * cd;
  const float* wp = wout + (size_t)c * cd;
  double acc = 0.0;
  for (int d = 0; d < cd; ++d) acc += (double)wp[d] * (double)e[d];
  return (float)(acc + (double)bout[c]);
}
