// ndac_rvq.hip -- the codec's residual vector quantiser: per codebook in_proj (1x1) -> L2-normalised nearest neighbour over the codebook ->
// out_proj (1x1); residual chain.  Kernels:
//   rvq_step_kernel     one residual quantiser: in_proj with f64 accumulation, nearest neighbour with the float32 operation order the
//                       oracle defines (code indices BIT-EXACT; ties -> lowest index), straight-through value, out_proj, residual update
//   rvq_chain_kernel    the whole chain of quantisers in ONE launch: the residual tile stays in LDS, z_q in registers; the same phase
//                       functions as rvq_step_kernel, the same bits (fd_rvq_encode_chain; the quantiser of fd_ndac_encode_ragged)
//   rvq_from_codes_kernel   codes -> sum_i out_proj_i(codebook_i[code])
#include <math.h>

#include "ndac_internal.h"

namespace {

constexpr int RT = 8;    // time steps per workgroup
constexpr int NP = 256 / RT;       // codebook slices / output-channel lanes per time step
static_assert(NP == 32, "the in_proj split below is 8 dims x 4 channel quarters");

struct RvqArgs {
  float* residual;        // [B][D][T] in / out
  float* zq;              // [B][D][T] accumulated
  int* codes;             // [B][nq][T], this quantiser writes row q
  float* latents;         // [B][nq * cd][T] or null
  RvqQuant p;
  const int* frames;      // device int32 [B] or null: clip b is its row's first frames[b] steps; steps behind it are never read and get code 0 / latents 0
  int B, D, T, J, cd, q, nq;
};

struct RvqTile {                     // the small per-tile arrays of one quantiser step (LDS)
  double pz[4][RT][8];
  float ze[RT][9];                   // in_proj output per time step (cd <= 8: fd_ndac_create), +1 pad
  float en[RT][9];
  float e2s[RT];
  float bestd[NP][RT];
  int besti[NP][RT];
  float stv[RT][9];                  // straight-through value z_e + (c - z_e)
  int code[RT];
};

constexpr int RVQ_PF = 16;           // operand loads in flight per thread in the in_proj sum (a channel quarter of D = 64 is 16 long)

// One slice [j0, j1) of the normalised codebook scanned in ascending order with a strict '<' (ties -> lowest index): dot product
// sequential over the dimensions, dist = (e2 - 2 dot) + c2[j].  CD: the codebook dimension at compile time, 0 = cd at run time.
template <int CD>
__device__ __forceinline__ void rvq_scan_slice(const float* e, float e2, const float* cbn, const float* c2, int cd, int j0, int j1, float& bd, int& bi) {
#pragma clang fp contract(off)
  const int n = CD ? CD : cd;
#pragma unroll 4
  for (int j = j0; j < j1; ++j) {
    const float* c = cbn + (size_t)j * n;
    float dot = 0.f;
#pragma unroll
    for (int d = 0; d < n; ++d) dot = dot + e[d] * c[d];
    const float dist = (e2 - 2.0f * dot) + c2[j];
    if (dist < bd) { bd = dist; bi = j; }
  }
}

// Phases (1)-(3) of one quantiser on one tile of 8 time steps, stated once for rvq_step_kernel and rvq_chain_kernel: the float32 /
// float64 operation order of oracle/ndac_oracle.py `pointwise_f64` / `vq_nearest` / `l2_normalize_rows_f32` (no fused multiply-add
// anywhere).  The 256 threads (tt = tid % 8, part = tid / 8) are
//   (1) 8 steps x 8 codebook dims x 4 quarters of the latent channels (f64 partial sums, combined in a fixed order),
//   (3) 8 steps x 32 slices of the codebook, each scanned in ascending order with a strict '<', slices merged in ascending order
//       (ties -> lowest index).
// rp: this thread's time step of the residual, channel c at rp[c * rstride] (global memory, stride T / the chain's LDS tile, stride RT).
// tv: the step holds data (else z_e = 0 and nothing of it is written by the caller).  Every thread of the workgroup calls it; on return
// (behind a barrier) s.ze, s.stv and s.code hold the step's in_proj output, straight-through value and code index.
__device__ __forceinline__ void rvq_tile_quantise(RvqTile& s, const RvqQuant& p, const float* rp, size_t rstride, bool tv, int D, int J, int cd, int tt,
                                                  int part) {
#pragma clang fp contract(off)
  // (1) z_e[d] = sum_c win[d][c] * residual[c] + bin[d]: exact f32 products accumulated in f64, rounded to f32 once
  {
    const int d = part & 7, qd = part >> 3;   // NP = 32: 8 dims x 4 channel quarters
    double acc = 0.0;
    if (tv && d < cd) {
      const int c0 = (int)((long long)D * qd / 4), c1 = (int)((long long)D * (qd + 1) / 4);
      const float* wp = p.win + (size_t)d * D;
      int c = c0;
      for (; c + RVQ_PF <= c1; c += RVQ_PF) {   // RVQ_PF loads of each operand in flight, then the same sequential sum: the loop is latency-bound
        float w[RVQ_PF], r[RVQ_PF];
#pragma unroll
        for (int i = 0; i < RVQ_PF; ++i) { w[i] = wp[c + i]; r[i] = rp[(size_t)(c + i) * rstride]; }
#pragma unroll
        for (int i = 0; i < RVQ_PF; ++i) acc += (double)w[i] * (double)r[i];
      }
      for (; c < c1; ++c) acc += (double)wp[c] * (double)rp[(size_t)c * rstride];
    }
    s.pz[qd][tt][d] = acc;
  }
  __syncthreads();
  if (part < 8) {
    const int d = part;
    s.ze[tt][d] = d < cd && tv ? (float)((((s.pz[0][tt][d] + s.pz[1][tt][d]) + s.pz[2][tt][d]) + s.pz[3][tt][d]) + (double)p.bin[d]) : 0.f;
  }
  __syncthreads();
  // (2) normalise: s = sum x^2 (sequential), n = sqrt(s), x / max(n, 1e-12); e2 = sum en^2
  if (part == 0) {
    float sq = 0.f;
    for (int d = 0; d < cd; ++d) sq = sq + s.ze[tt][d] * s.ze[tt][d];
    const float n = fmaxf(sqrtf(sq), 1e-12f);
    float e2 = 0.f;
    for (int d = 0; d < cd; ++d) {
      const float v = s.ze[tt][d] / n;
      s.en[tt][d] = v;
      e2 = e2 + v * v;
    }
    s.e2s[tt] = e2;
  }
  __syncthreads();
  // (3) nearest neighbour
  {
    float e[8];
    for (int d = 0; d < 8; ++d) e[d] = d < cd ? s.en[tt][d] : 0.f;
    const float e2 = s.e2s[tt];
    const int j0 = (int)((long long)J * part / NP), j1 = (int)((long long)J * (part + 1) / NP);
    float bd = INFINITY; int bi = j0;
    if (cd == 8) rvq_scan_slice<8>(e, e2, p.cbn, p.c2, cd, j0, j1, bd, bi);   // DAC's codebook dimension: the row as two wide loads
    else rvq_scan_slice<0>(e, e2, p.cbn, p.c2, cd, j0, j1, bd, bi);
    s.bestd[part][tt] = bd; s.besti[part][tt] = bi;
  }
  __syncthreads();
  if (part == 0) {
    float bd = s.bestd[0][tt]; int bi = s.besti[0][tt];
    for (int q = 1; q < NP; ++q)
      if (s.bestd[q][tt] < bd) { bd = s.bestd[q][tt]; bi = s.besti[q][tt]; }
    s.code[tt] = bi;
    for (int d = 0; d < cd; ++d) {
      const float z = s.ze[tt][d];
      s.stv[tt][d] = z + (p.cb[(size_t)bi * cd + d] - z);     // z_e + (z_q - z_e).detach()
    }
  }
  __syncthreads();
}

// (4) z_q_i[c] = sum_d wout[c][d] * st[d] + bout[c] (f64, rounded once)
__device__ __forceinline__ float rvq_out_proj(const RvqQuant& p, const float* st, int cd, int c) {
#pragma clang fp contract(off)
  double acc = 0.0;
  const float* wp = p.wout + (size_t)c * cd;
  for (int d = 0; d < cd; ++d) acc += (double)wp[d] * (double)st[d];
  return (float)(acc + (double)p.bout[c]);
}

// codes / latents of one step: the values where the step holds data, 0 behind a clip (tv false, t < T only under a frame table)
__device__ __forceinline__ void rvq_write_step(const RvqTile& s, int* codes, float* latents, bool tv, int b, int t, int tt, int T, int cd, int q, int nq) {
  if (t >= T) return;
  codes[((size_t)b * nq + q) * T + t] = tv ? s.code[tt] : 0;
  if (latents)
    for (int d = 0; d < cd; ++d) latents[((size_t)b * nq * cd + (size_t)q * cd + d) * T + t] = tv ? s.ze[tt][d] : 0.f;
}

// One residual quantiser per launch, 8 time steps per workgroup (a 2 s clip has 150 frames: small tiles are what fills the chip);
// (4) runs as 8 steps x 32 output-channel lanes: zq += z_q_i; residual -= z_q_i, both through global memory.
__global__ __launch_bounds__(256) void rvq_step_kernel(RvqArgs a) {
#pragma clang fp contract(off)
  __shared__ RvqTile s;
  const int b = blockIdx.y, t0 = blockIdx.x * RT, tid = threadIdx.x;
  const int tt = tid % RT, part = tid / RT;
  const int t = t0 + tt;
  const bool tv = t < (a.frames ? a.frames[b] : a.T);
  rvq_tile_quantise(s, a.p, a.residual + (size_t)b * a.D * a.T + t, (size_t)a.T, tv, a.D, a.J, a.cd, tt, part);
  if (part == 0) rvq_write_step(s, a.codes, a.latents, tv, b, t, tt, a.T, a.cd, a.q, a.nq);
  if (tv) {
    for (int c = part; c < a.D; c += NP) {
      const float zi = rvq_out_proj(a.p, s.stv[tt], a.cd, c);
      const size_t o = ((size_t)b * a.D + c) * a.T + t;
      a.zq[o] = a.zq[o] + zi;
      a.residual[o] = a.residual[o] - zi;
    }
  }
}

// All n_quantizers quantisers in ONE launch, same tiling.  The [D][RT] residual tile is loaded once and lives in LDS across the
// quantisers (never written back; z is read-only), a thread's z_q values (channels part, part + 32, ...: NI of them) accumulate in
// registers from 0 in quantiser order and are stored once.  Same arithmetic per value as the chain of rvq_step_kernel launches (the
// phases are the functions above): the same bits.  LDS: in (1) a wave reads ONE channel row of the tile per step -- 8 consecutive
// words, each broadcast to the wave's 8 codebook dims -- and in (4) 64 consecutive words: conflict-free.
// Under a frame table, steps at and behind frames[b] are not read; they get code 0, z_q 0, latents 0.
struct RvqChainArgs {
  const float* z; float* zq; int* codes; float* latents;
  const RvqQuant* quant;  // [n_codebooks] (device)
  const int* frames;
  int B, D, T, J, cd, nq;
};

template <int NI>
__global__ __launch_bounds__(256) void rvq_chain_kernel(RvqChainArgs a) {
#pragma clang fp contract(off)
  extern __shared__ float rs[];      // [D][RT] residual tile
  __shared__ RvqTile s;
  const int b = blockIdx.y, t0 = blockIdx.x * RT, tid = threadIdx.x;
  const int tt = tid % RT, part = tid / RT;
  const int t = t0 + tt;
  const bool tv = t < (a.frames ? a.frames[b] : a.T);
  float zq[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int c = part + NP * i;
    zq[i] = 0.f;
    if (c < a.D) rs[c * RT + tt] = tv ? a.z[((size_t)b * a.D + c) * a.T + t] : 0.f;
  }
  __syncthreads();
  if (t0 < (a.frames ? a.frames[b] : a.T)) {      // (uniform per workgroup; a tile wholly behind its clip only writes the zeros below)
    for (int q = 0; q < a.nq; ++q) {
      const RvqQuant p = a.quant[q];
      rvq_tile_quantise(s, p, rs + tt, (size_t)RT, tv, a.D, a.J, a.cd, tt, part);
      if (part == 0) rvq_write_step(s, a.codes, a.latents, tv, b, t, tt, a.T, a.cd, q, a.nq);
      if (tv) {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
          const int c = part + NP * i;
          if (c < a.D) {
            const float zi = rvq_out_proj(p, s.stv[tt], a.cd, c);
            zq[i] = zq[i] + zi;
            rs[c * RT + tt] = rs[c * RT + tt] - zi;
          }
        }
      }
      __syncthreads();               // the tile's next in_proj reads what (4) wrote; s is reused
    }
  } else if (part == 0) {
    for (int q = 0; q < a.nq; ++q) rvq_write_step(s, a.codes, a.latents, false, b, t, tt, a.T, a.cd, q, a.nq);
  }
  if (t < a.T) {
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int c = part + NP * i;
      if (c < a.D) a.zq[((size_t)b * a.D + c) * a.T + t] = zq[i];
    }
  }
}

struct FromCodesArgs {
  const int* codes; float* zq; const float* const* wout; const float* const* bout; const float* const* cb;
  int B, D, T, J, cd, nq;
};
// z_q[b][c][t] = sum_i ( f32( sum_d wout_i[c][d] cb_i[code][d] + bout_i[c] ) ), i ascending, f32 adds  (ResidualVectorQuantize.from_codes)
__global__ __launch_bounds__(256) void rvq_from_codes_kernel(FromCodesArgs a) {
#pragma clang fp contract(off)
  const long long n = (long long)a.B * a.D * a.T;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int t = (int)(i % a.T);
    const int c = (int)((i / a.T) % a.D);
    const int b = (int)(i / ((long long)a.T * a.D));
    float z = 0.f;
    for (int q = 0; q < a.nq; ++q) z = z + fd_rvq_code_term(a.cb[q], a.wout[q], a.bout[q], a.codes[((size_t)b * a.nq + q) * a.T + t], a.J, a.cd, c);
    a.zq[i] = z;
  }
}

constexpr int RVQ_CHAIN_MAX_NI = 32;   // z_q values a thread of rvq_chain_kernel keeps in registers: channels part + 32 i

}  // namespace

int fd_rvq_run(fd_ndac* m, float* residual /* in: z, destroyed */, const int* frames, int B, int T, int nq, float* zq, int* codes, float* latents,
            hipStream_t st) {
  const fd_ndac_config& c = m->plan.cfg;
  FD_HIP(hipMemsetAsync(zq, 0, sizeof(float) * (size_t)B * c.latent_dim * T, st));
  for (int q = 0; q < nq; ++q) {
    RvqArgs a{residual, zq, codes, latents, m->quant[q], frames, B, c.latent_dim, T, c.codebook_size, c.codebook_dim, q, nq};
    hipLaunchKernelGGL(rvq_step_kernel, dim3(fd_cdiv(T, RT), B), dim3(256), 0, st, a);
  }
  FD_LAUNCH_CHECK();
  return FD_OK;
}

// One launch for the whole chain (rvq_chain_kernel); the caller has checked fd_rvq_chain_supported.  z is read-only.
int fd_rvq_run_chain(fd_ndac* m, const float* z, const int* frames, int B, int T, int nq, float* zq, int* codes, float* latents, hipStream_t st) {
  const fd_ndac_config& c = m->plan.cfg;
  RvqChainArgs a{z, zq, codes, latents, m->d_quant, frames, B, c.latent_dim, T, c.codebook_size, c.codebook_dim, nq};
  const dim3 grid(fd_cdiv(T, RT), B);
  const size_t lds = sizeof(float) * (size_t)c.latent_dim * RT;
  const int ni = fd_cdiv(c.latent_dim, NP);
  if (ni <= 4) hipLaunchKernelGGL(rvq_chain_kernel<4>, grid, dim3(256), lds, st, a);
  else if (ni <= 8) hipLaunchKernelGGL(rvq_chain_kernel<8>, grid, dim3(256), lds, st, a);
  else if (ni <= 16) hipLaunchKernelGGL(rvq_chain_kernel<16>, grid, dim3(256), lds, st, a);
  else hipLaunchKernelGGL(rvq_chain_kernel<RVQ_CHAIN_MAX_NI>, grid, dim3(256), lds, st, a);
  FD_LAUNCH_CHECK();
  return FD_OK;
}

extern "C" int fd_rvq_encode(fd_ndac* m, const float* z, int B, int T, int n_quantizers, float* z_q, int* codes, float* latents, void* ws, size_t ws_bytes,
                             void* stream) {
  FD_TRY(fd_ndac_check_ready(m, "fd_rvq_encode"));
  FD_REQUIRE(z && z_q && codes && ws && B > 0 && T > 0, "fd_rvq_encode: bad arguments");
  const int nq = fd_ndac_resolve_nq(m, n_quantizers);
  const size_t need = sizeof(float) * (size_t)B * m->plan.cfg.latent_dim * T;
  if (ws_bytes < need) return fd_set_error(FD_ENOMEM, "fd_rvq_encode: workspace %zu < required %zu bytes", ws_bytes, need);
  hipStream_t st = fd_stream(stream);
  FD_HIP(hipMemcpyAsync(ws, z, need, hipMemcpyDeviceToDevice, st));   // the residual chain works in place on a copy
  return fd_rvq_run(m, (float*)ws, nullptr, B, T, nq, z_q, codes, latents, st);
}

extern "C" int fd_rvq_chain_supported(int D, int cd) {   // host only: the [D][8] float32 tile beside the small arrays within LDS, D / 32 z_q registers per thread
  return D >= 1 && cd >= 1 && cd <= 8 && fd_cdiv(D, NP) <= RVQ_CHAIN_MAX_NI && sizeof(float) * (size_t)D * RT + sizeof(RvqTile) <= 64 * 1024;
}

extern "C" int fd_rvq_encode_chain(fd_ndac* m, const float* z, const int* frames, int B, int T, int n_quantizers, float* z_q, int* codes, float* latents,
                                   void* stream) {
  FD_TRY(fd_ndac_check_ready(m, "fd_rvq_encode_chain"));
  FD_REQUIRE(z && z_q && codes && B > 0 && T > 0, "fd_rvq_encode_chain: bad arguments");
  FD_REQUIRE(fd_rvq_chain_supported(m->plan.cfg.latent_dim, m->plan.cfg.codebook_dim), "fd_rvq_encode_chain: latent_dim %d is beyond the one-launch kernel (at most %d)",
             m->plan.cfg.latent_dim, NP * RVQ_CHAIN_MAX_NI);
  hipStream_t st = fd_stream(stream);
  if (frames) FD_TRY(fd_ndac_check_frames("fd_rvq_encode_chain", frames, B, T, st));
  return fd_rvq_run_chain(m, z, frames, B, T, fd_ndac_resolve_nq(m, n_quantizers), z_q, codes, latents, st);
}

extern "C" int fd_rvq_from_codes(fd_ndac* m, const int* codes, int B, int n_quantizers, int T, float* z_q, void* stream) {
  FD_TRY(fd_ndac_check_ready(m, "fd_rvq_from_codes"));
  FD_REQUIRE(codes && z_q && B > 0 && T > 0 && n_quantizers >= 1 && n_quantizers <= m->plan.cfg.n_codebooks, "fd_rvq_from_codes: bad arguments");
  FromCodesArgs a{codes, z_q, m->d_wout, m->d_bout, m->d_cb, B, m->plan.cfg.latent_dim, T, m->plan.cfg.codebook_size, m->plan.cfg.codebook_dim, n_quantizers};
  const long long n = (long long)B * a.D * T;
  hipLaunchKernelGGL(rvq_from_codes_kernel, dim3((unsigned)(n / 256 + 1 > 65535 ? 65535 : n / 256 + 1)), dim3(256), 0, fd_stream(stream), a);
  FD_LAUNCH_CHECK();
  return FD_OK;
}
