// ndac_internal.h -- what ndac.hip shares with ndac_pool.hip: the layer walks of the ragged entry points, the from_codes term, a read-only
// view of the codec's tables and the slot where the pool keeps its captured graphs.  fd_ndac itself stays private to ndac.hip.
#pragma once
#include "internal.h"

struct fd_ndac_view {
  const float* const* wout; const float* const* bout; const float* const* cb;   // DEVICE arrays [n_codebooks] of device pointers (rvq_from_codes_kernel's)
  int latent_dim, codebook_size, codebook_dim, n_codebooks;
  int hop;            // samples per latent frame on the encoder side
  int precision;      // FD_NDAC_* flags of the next call
};
fd_ndac_view fd_ndac_get_view(const fd_ndac* m);
int fd_ndac_check_ready(const fd_ndac* m, const char* who);
// The decoder / encoder walk of fd_ndac_decode_ragged / fd_ndac_encode_ragged under a DEVICE frame table the caller vouches for (every entry
// in [1, T] resp. [1, L / hop]): no copy to the host, no synchronisation.  ws: fd_ndac_workspace_bytes(m, B, max(decoded length, T * hop)) resp.
// (m, B, L).  latents may be null.
int fd_ndac_decode_walk(fd_ndac* m, const char* who, const float* z, const int* frames, int B, int T, float* audio, void* ws, size_t ws_bytes, hipStream_t st);
int fd_ndac_encode_walk(fd_ndac* m, const char* who, const float* x, const int* frames, int B, int L, int n_quantizers, float* z_q, int* codes,
                        float* latents, void* ws, size_t ws_bytes, hipStream_t st);
// ndac_pool.hip's per-codec state (graph cache): created there on first use, released by fd_ndac_destroy through fd_ndac_pool_state_free
void** fd_ndac_pool_state(fd_ndac* m);
void fd_ndac_pool_state_free(void* state);

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
