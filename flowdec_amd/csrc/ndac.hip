// ndac.hip -- the NDAC codec in front of the FlowDec post-filter (demo.ipynb cells 2-3: `DAC.load`, `dac_model.encode(x,
// n_quantizers=nq)`, `dac_model.quantizer.from_codes(codes)`, `dac_model.decode(zq)`): the Descript Audio Codec architecture
// (descript-audio-codec==1.0.0, /root/reference/requirements.txt:4 -- third party, NOT under /root/reference: the algorithm is the
// published one, restated; oracle/ndac_oracle.py names the upstream definitions; PARITY UNPINNED).
//
// This file is the MODEL: the codec object, its parameters, and the encoder and decoder stacks run as a loop over the layer records of
// ndac_plan.h (which states the structure, the lengths and the halos once).  The kernels live beside it: ndac_conv1d.hip (the exact f32
// convolutions), ndac_mfma.hip (the wide layers as split-bf16 implicit GEMMs on the matrix cores: the decoder's default, the encoder's
// opt-in -- fd_ndac_set_precision), ndac_rvq.hip (the quantiser).  Layout [B][C][T] float32.
// Ragged decode (fd_ndac_decode_ragged): every convolution kernel reads input positions at and behind T as the zero padding; under a frame
// table (fd_ndac_lens) that bound is the CLIP's own length at the layer, so a clip in a batch of longer rows sees exactly the padding it
// sees alone -- the same bits -- and nothing behind it is read as data.  No table (every dense call): the bound is T.
// Ragged encode (fd_ndac_encode_ragged) is the same table on the way down: a clip of f frames is f * hop / (the strides so far) positions.
#include <math.h>

#include <utility>
#include <vector>

#include "ndac_internal.h"

extern "C" int fd_ndac_create(const fd_ndac_config* cfg, fd_ndac** out) {
  FD_REQUIRE(cfg && out, "fd_ndac_create: null pointer");
  FD_REQUIRE(cfg->encoder_dim > 0 && cfg->decoder_dim > 0 && cfg->latent_dim > 0, "fd_ndac_create: bad widths");
  FD_REQUIRE(cfg->n_encoder_rates >= 1 && cfg->n_encoder_rates <= 8 && cfg->n_decoder_rates >= 1 && cfg->n_decoder_rates <= 8, "fd_ndac_create: 1..8 rates per stack");
  FD_REQUIRE(cfg->decoder_dim % (1 << cfg->n_decoder_rates) == 0, "fd_ndac_create: decoder_dim must be divisible by 2^len(decoder_rates)");
  FD_REQUIRE(cfg->n_codebooks >= 1 && cfg->n_codebooks <= 64 && cfg->codebook_size >= 8 && cfg->codebook_dim >= 1 && cfg->codebook_dim <= 8,
             "fd_ndac_create: 1..64 codebooks of >= 8 entries and 1..8 dimensions (DAC: 8)");
  for (int i = 0; i < cfg->n_encoder_rates; ++i)
    FD_REQUIRE(cfg->encoder_rates[i] >= 1 && cfg->encoder_rates[i] <= 16, "fd_ndac_create: encoder rate %d out of range [1, 16]", cfg->encoder_rates[i]);
  for (int i = 0; i < cfg->n_decoder_rates; ++i)
    FD_REQUIRE(cfg->decoder_rates[i] >= 1 && cfg->decoder_rates[i] <= 16, "fd_ndac_create: decoder rate %d out of range [1, 16]", cfg->decoder_rates[i]);
  fd_ndac* m = new fd_ndac();
  m->plan = ndac::make_plan(*cfg);
  m->host.resize(m->plan.params.size());
  *out = m;
  return FD_OK;
}

extern "C" void fd_ndac_destroy(fd_ndac* m) {
  if (!m) return;
  fd_ndac_pool_state_free(m->pool_state);
  for (void* p : m->allocs) (void)hipFree(p);
  delete m;
}

extern "C" int fd_ndac_hop_length(const fd_ndac* m) { return m ? m->plan.hop : 0; }
extern "C" int fd_ndac_num_params(const fd_ndac* m) { return m ? (int)m->plan.params.size() : 0; }

extern "C" int fd_ndac_param_info(const fd_ndac* m, int i, const char** name, int* ndim, int shape[3]) {
  FD_REQUIRE(m && name && ndim && shape && i >= 0 && i < (int)m->plan.params.size(), "fd_ndac_param_info: bad arguments");
  const ndac::Param& p = m->plan.params[i];
  *name = p.name.c_str(); *ndim = (int)p.shape.size();
  for (int k = 0; k < 3; ++k) shape[k] = k < (int)p.shape.size() ? p.shape[k] : 1;
  return FD_OK;
}

extern "C" int fd_ndac_set_param(fd_ndac* m, const char* name, const float* host_data, long long numel) {
  FD_REQUIRE(m && name && host_data, "fd_ndac_set_param: null pointer");
  FD_REQUIRE(!m->finalized, "fd_ndac_set_param: codec already finalised");
  const int i = m->plan.find(name);   // the one place a parameter is looked up by name
  if (i < 0) return fd_set_error(FD_EINVAL, "fd_ndac_set_param: unknown parameter '%s'", name);
  const long long want = m->plan.params[i].numel();
  FD_REQUIRE(numel == want, "fd_ndac_set_param: '%s' expects %lld values (got %lld)", name, want, numel);
  m->host[i].assign(host_data, host_data + numel);
  return FD_OK;
}

void fd_ndac_weight_ci_k_co(const float* w, int Ci, int Co, int K, int transposed, float* dst) {
  for (int ci = 0; ci < Ci; ++ci)
    for (int k = 0; k < K; ++k)
      for (int co = 0; co < Co; ++co)
        dst[((size_t)ci * K + k) * Co + co] = transposed ? w[((size_t)ci * Co + co) * K + k] : w[((size_t)co * Ci + ci) * K + k];
}

extern "C" int fd_ndac_finalize(fd_ndac* m, void* stream) {
  FD_REQUIRE(m, "fd_ndac_finalize: null codec");
  if (m->finalized) return FD_OK;
  hipStream_t st = fd_stream(stream);
  ndac::Plan& plan = m->plan;
  for (size_t i = 0; i < plan.params.size(); ++i)
    if (m->host[i].empty()) return fd_set_error(FD_ESTATE, "fd_ndac_finalize: parameter '%s' missing", plan.params[i].name.c_str());
  auto upload = [&](const std::vector<float>& h, float** out) -> int {
    float* d = nullptr;
    FD_HIP(hipMalloc(&d, sizeof(float) * h.size()));
    m->allocs.push_back(d);
    FD_HIP(hipMemcpyAsync(d, h.data(), sizeof(float) * h.size(), hipMemcpyHostToDevice, st));
    *out = d;
    return FD_OK;
  };
  // the conv stacks keep their weights as [Ci][K][Co] (output channel fastest: the kernels stage 32 consecutive channels per row);
  // state_dict layout is [Co][Ci][K] for Conv1d and [Ci][Co][K] for ConvTranspose1d
  std::vector<ndac::Layer*> layer_of(plan.params.size(), nullptr);   // weight's parameter index -> its layer
  for (std::vector<ndac::Layer>* stack : {&plan.enc, &plan.dec})
    for (ndac::Layer& l : *stack) layer_of[l.weight] = &l;
  m->dev.resize(plan.params.size());
  for (size_t i = 0; i < plan.params.size(); ++i) {   // device memory in table order, a layer's packed copy in front of its weight
    if (ndac::Layer* l = layer_of[i]) {
      std::vector<float>& w = m->host[i];
      std::vector<float> t(w.size());
      fd_ndac_weight_ci_k_co(w.data(), l->Ci, l->Co, l->K, l->transposed, t.data());
      w.swap(t);
      // (dilation 9: the widest staged tile of a K = 7 layer)
      if (fd_ndac_mfma_supported(l->Ci, l->Co, l->K, l->stride, l->stride > 1 || l->K == 1 ? 1 : 9, l->transposed)) {
        const size_t nb = fd_ndac_mfma_packed_bytes(l->Ci, l->Co, l->K, l->stride, l->transposed);
        std::vector<unsigned char> hp(nb);
        fd_ndac_mfma_pack(w.data(), l->Ci, l->Co, l->K, l->stride, l->transposed, hp.data());
        void* dp = nullptr;
        FD_HIP(hipMalloc(&dp, nb));
        m->allocs.push_back(dp);
        FD_HIP(hipMemcpy(dp, hp.data(), nb, hipMemcpyHostToDevice));
        l->packed = dp;
      }
    }
    FD_TRY(upload(m->host[i], &m->dev[i]));
  }
  for (std::vector<ndac::Layer>* stack : {&plan.enc, &plan.dec})
    for (ndac::Layer& l : *stack) { l.w = m->dev[l.weight]; l.b = m->dev[l.bias]; l.alpha = l.alpha_out >= 0 ? m->dev[l.alpha_out] : nullptr; }
  // L2-normalised codebooks and their squared norms, in the float32 operation order of the oracle (plain C float arithmetic on the
  // host: products and sums rounded separately -- this file is compiled without fast-math / contraction on the host side)
  const fd_ndac_config& c = plan.cfg;
  std::vector<const float*> hw, hb, hc;
  for (const ndac::Quantizer& q : plan.quant) {
    const std::vector<float>& cb = m->host[q.codebook];
    std::vector<float> cn(cb.size()), c2(c.codebook_size);
    for (int j = 0; j < c.codebook_size; ++j) {
      volatile float s = 0.f;
      for (int d = 0; d < c.codebook_dim; ++d) { volatile float pr = cb[(size_t)j * c.codebook_dim + d] * cb[(size_t)j * c.codebook_dim + d]; s = s + pr; }
      float nrm = sqrtf(s);
      if (nrm < 1e-12f) nrm = 1e-12f;
      volatile float s2 = 0.f;
      for (int d = 0; d < c.codebook_dim; ++d) {
        const float v = cb[(size_t)j * c.codebook_dim + d] / nrm;
        cn[(size_t)j * c.codebook_dim + d] = v;
        volatile float pr = v * v; s2 = s2 + pr;
      }
      c2[j] = s2;
    }
    float *dcn = nullptr, *dc2 = nullptr;
    FD_TRY(upload(cn, &dcn)); FD_TRY(upload(c2, &dc2));
    FD_HIP(hipStreamSynchronize(st));   // cn / c2 are locals
    m->quant.push_back(RvqQuant{m->dev[q.in_w], m->dev[q.in_b], m->dev[q.out_w], m->dev[q.out_b], m->dev[q.codebook], dcn, dc2});
    hw.push_back(m->dev[q.out_w]); hb.push_back(m->dev[q.out_b]); hc.push_back(m->dev[q.codebook]);
  }
  auto upload_ptrs = [&](const std::vector<const float*>& h, const float*** out) -> int {
    const float** d = nullptr;
    FD_HIP(hipMalloc(&d, sizeof(float*) * h.size()));
    m->allocs.push_back((void*)d);
    FD_HIP(hipMemcpy((void*)d, h.data(), sizeof(float*) * h.size(), hipMemcpyHostToDevice));
    *out = d;
    return FD_OK;
  };
  FD_TRY(upload_ptrs(hw, &m->d_wout)); FD_TRY(upload_ptrs(hb, &m->d_bout)); FD_TRY(upload_ptrs(hc, &m->d_cb));
  {
    RvqQuant* dq = nullptr;
    FD_HIP(hipMalloc(&dq, sizeof(RvqQuant) * m->quant.size()));
    m->allocs.push_back((void*)dq);
    FD_HIP(hipMemcpy((void*)dq, m->quant.data(), sizeof(RvqQuant) * m->quant.size(), hipMemcpyHostToDevice));
    m->d_quant = dq;
  }
  FD_HIP(hipStreamSynchronize(st));
  m->host.clear();
  m->finalized = true;
  return FD_OK;
}

extern "C" int fd_ndac_set_precision(fd_ndac* m, int flags) {
  FD_REQUIRE(m, "fd_ndac_set_precision: null codec");
  FD_REQUIRE((flags & ~(FD_NDAC_MFMA_DECODER | FD_NDAC_MFMA_ENCODER)) == 0, "fd_ndac_set_precision: unknown flags 0x%x", flags);
  m->precision = flags;
  return FD_OK;
}
extern "C" int fd_ndac_get_precision(const fd_ndac* m) { return m ? m->precision : -1; }

extern "C" int fd_ndac_latent_frames(const fd_ndac* m, int L) { return m && L > 0 ? (int)m->plan.latent_frames(L) : 0; }
extern "C" int fd_ndac_decoded_length(const fd_ndac* m, int T) { return m && T > 0 ? (int)m->plan.decoded_length(T) : 0; }

// {raw, activated} of the current tensor, {raw, activated} of the next, one mid-unit tensor
static size_t slot_bytes(int B, long long elems) { return fd_align(sizeof(float) * (size_t)B * elems); }
extern "C" size_t fd_ndac_workspace_bytes(const fd_ndac* m, int B, int L) { return m && B > 0 && L > 0 ? 5 * slot_bytes(B, m->plan.slot_elems(L)) + 256 : 0; }

extern "C" int fd_ndac_encode_halo(const fd_ndac* m, int* left, int* right) {
  FD_REQUIRE(m && left && right, "fd_ndac_encode_halo: null pointer");
  FD_REQUIRE(m->plan.whole_frames_error.empty(), "fd_ndac_encode_halo: %s", m->plan.whole_frames_error.c_str());
  m->plan.encode_halo(left, right);
  return FD_OK;
}

extern "C" int fd_ndac_decode_halo(const fd_ndac* m, int* left, int* right) {
  FD_REQUIRE(m && left && right, "fd_ndac_decode_halo: null pointer");
  FD_REQUIRE(m->plan.even_rates_error.empty(), "fd_ndac_decode_halo: %s", m->plan.even_rates_error.c_str());
  m->plan.decode_halo(left, right);
  return FD_OK;
}

int fd_ndac_check_frames(const char* who, const int* frames, int B, int T, hipStream_t st) {
  std::vector<int> h(B);
  FD_HIP(hipMemcpyAsync(h.data(), frames, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost, st));
  FD_HIP(hipStreamSynchronize(st));
  for (int b = 0; b < B; ++b) FD_REQUIRE(h[b] >= 1 && h[b] <= T, "%s: frames[%d] = %d is outside [1, %d]", who, b, h[b], T);
  return FD_OK;
}

namespace {

// Ragged decode: row b of the audio behind its clip's own decoded length is zero, whatever the last convolution computed there.
__global__ __launch_bounds__(256) void ndac_zero_tail_kernel(float* audio, fd_ndac_lens lens, int L) {
  const int b = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
  if (t < L && t >= lens.frames[b] * lens.mul + lens.add) audio[(size_t)b * L + t] = 0.f;
}

// One stack over the five workspace slots of `slot` bytes each.  Every layer reads an ALREADY ACTIVATED input (raw for the first) and is
// computed over the whole row; under a frame table (lens.frames, advanced here to the clips' lengths at each layer's input) a kernel
// bounds its INPUT reads by the clip's own length, so what a layer wrote behind a clip is never read as data.  A ResidualUnit's 7-tap
// convolution writes only the activated mid tensor; its 1x1 reads that, adds the unit's raw input and is the unit's result.  The last
// layer's raw result goes to `result` (null: to a slot; `result` then says which).  The wide layers run on the matrix cores where `mfma`
// says so and a packed copy exists; never the tanh layer.  T: the row length, in / out.
int run_stack(const std::vector<ndac::Layer>& stack, bool mfma, const float* x, int B, int& T, fd_ndac_lens& lens, void* ws, size_t slot, float*& result,
              hipStream_t st) {
  float* buf[5];
  for (int i = 0; i < 5; ++i) buf[i] = (float*)((char*)ws + i * slot);
  float *nxt_raw = buf[0], *nxt_act = buf[1], *cur_raw = buf[2], *cur_act = buf[3], *mid = buf[4];
  for (size_t i = 0; i < stack.size(); ++i) {
    const ndac::Layer& l = stack[i];
    const bool last = i + 1 == stack.size(), to_mid = !last && stack[i + 1].residual;
    const float* in = i == 0 ? x : (l.residual ? mid : cur_act);
    const float* res = l.residual ? cur_raw : nullptr;
    float* out = !l.keep_raw ? nullptr : (last && result ? result : nxt_raw);
    float* act = to_mid ? mid : (l.alpha_out >= 0 ? nxt_act : nullptr);
    if (last) result = out;
    if (l.packed && mfma && !l.tanh_out)
      FD_TRY(fd_ndac_mfma_conv(in, l.packed, l.b, res, out, act, l.alpha, B, l.Ci, T, l.Co, l.K, l.stride, l.pad, l.dil, l.transposed, st, lens));
    else if (l.transposed)
      FD_TRY(fd_launch_convtr1d(in, l.w, l.b, nullptr, out, B, l.Ci, T, l.Co, l.K, l.stride, l.pad, st, /*wt*/ 1, act, l.alpha, lens));
    else
      FD_TRY(fd_launch_conv1d(in, l.w, l.b, nullptr, res, out, B, l.Ci, T, l.Co, l.K, l.stride, l.pad, l.dil, l.tanh_out, st, /*wt*/ 1, act, l.alpha, lens));
    if (!to_mid) { std::swap(cur_raw, nxt_raw); std::swap(cur_act, nxt_act); }
    T = (int)l.out_len(T);
    l.advance(lens.mul, lens.add);
  }
  return FD_OK;
}

}  // namespace

// The encoder and the quantiser of fd_ndac_encode / fd_ndac_encode_ragged.  The quantiser runs as ONE launch under a frame table
// (rvq_chain_kernel; the step kernels where fd_rvq_chain_supported says no), as the chain of step launches without one.
int fd_ndac_encode_walk(fd_ndac* m, const char* who, const float* x, const int* frames, int B, int L, int n_quantizers, float* z_q, int* codes, float* latents,
                        void* ws, size_t ws_bytes, hipStream_t st) {
  const size_t slot = slot_bytes(B, m->plan.slot_elems(L)), need = 5 * slot + 256;   // = fd_ndac_workspace_bytes(m, B, L)
  if (ws_bytes < need) return fd_set_error(FD_ENOMEM, "%s: workspace %zu < required %zu bytes", who, ws_bytes, need);
  const fd_ndac_config& c = m->plan.cfg;
  fd_ndac_lens lens;
  lens.frames = frames; lens.mul = m->plan.hop;
  int T = L;
  float* z = nullptr;
  FD_TRY(run_stack(m->plan.enc, (m->precision & FD_NDAC_MFMA_ENCODER) != 0, x, B, T, lens, ws, slot, z, st));
  const int nq = fd_ndac_resolve_nq(m, n_quantizers);
  if (frames && fd_rvq_chain_supported(c.latent_dim, c.codebook_dim)) return fd_rvq_run_chain(m, z, frames, B, T, nq, z_q, codes, latents, st);
  return fd_rvq_run(m, z, frames, B, T, nq, z_q, codes, latents, st);
}

extern "C" int fd_ndac_encode(fd_ndac* m, const float* x, int B, int L, int n_quantizers, float* z_q, int* codes, float* latents, void* ws,
                              size_t ws_bytes, void* stream) {
  FD_TRY(fd_ndac_check_ready(m, "fd_ndac_encode"));
  FD_REQUIRE(x && z_q && codes && ws && B > 0 && L > 0, "fd_ndac_encode: bad arguments");
  FD_REQUIRE(L % m->plan.hop == 0, "fd_ndac_encode: pad the waveform to a multiple of the hop length %d first (DAC.preprocess); got %d samples", m->plan.hop, L);
  return fd_ndac_encode_walk(m, "fd_ndac_encode", x, nullptr, B, L, n_quantizers, z_q, codes, latents, ws, ws_bytes, fd_stream(stream));
}

extern "C" int fd_ndac_encode_ragged(fd_ndac* m, const float* x, const int* frames, int B, int L, int n_quantizers, float* z_q, int* codes, float* latents,
                                     void* ws, size_t ws_bytes, void* stream) {
  FD_TRY(fd_ndac_check_ready(m, "fd_ndac_encode_ragged"));
  FD_REQUIRE(x && frames && z_q && codes && ws && B > 0 && L > 0, "fd_ndac_encode_ragged: bad arguments");
  FD_REQUIRE(L % m->plan.hop == 0, "fd_ndac_encode_ragged: the row length must be a multiple of the hop length %d; got %d samples", m->plan.hop, L);
  FD_REQUIRE(m->plan.whole_frames_error.empty(), "fd_ndac_encode_ragged: %s", m->plan.whole_frames_error.c_str());
  hipStream_t st = fd_stream(stream);
  FD_TRY(fd_ndac_check_frames("fd_ndac_encode_ragged", frames, B, L / m->plan.hop, st));
  return fd_ndac_encode_walk(m, "fd_ndac_encode_ragged", x, frames, B, L, n_quantizers, z_q, codes, latents, ws, ws_bytes, st);
}

int fd_ndac_decode_walk(fd_ndac* m, const char* who, const float* z, const int* frames, int B, int T, float* audio, void* ws, size_t ws_bytes, hipStream_t st) {
  const size_t slot = slot_bytes(B, ndac::stack_widest(m->plan.dec, T));
  if (ws_bytes < 5 * slot) return fd_set_error(FD_ENOMEM, "%s: workspace %zu < required %zu bytes", who, ws_bytes, 5 * slot);
  fd_ndac_lens lens;
  lens.frames = frames;
  FD_TRY(run_stack(m->plan.dec, (m->precision & FD_NDAC_MFMA_DECODER) != 0, z, B, T, lens, ws, slot, audio, st));
  if (frames) {
    hipLaunchKernelGGL(ndac_zero_tail_kernel, dim3(fd_cdiv(T, 256), B), dim3(256), 0, st, audio, lens, T);
    FD_LAUNCH_CHECK();
  }
  return FD_OK;
}

extern "C" int fd_ndac_decode(fd_ndac* m, const float* z, int B, int T, float* audio, void* ws, size_t ws_bytes, void* stream) {
  FD_TRY(fd_ndac_check_ready(m, "fd_ndac_decode"));
  FD_REQUIRE(z && audio && ws && B > 0 && T > 0, "fd_ndac_decode: bad arguments");
  return fd_ndac_decode_walk(m, "fd_ndac_decode", z, nullptr, B, T, audio, ws, ws_bytes, fd_stream(stream));
}

extern "C" int fd_ndac_decode_ragged(fd_ndac* m, const float* z, const int* frames, int B, int T, float* audio, void* ws, size_t ws_bytes, void* stream) {
  FD_TRY(fd_ndac_check_ready(m, "fd_ndac_decode_ragged"));
  FD_REQUIRE(z && frames && audio && ws && B > 0 && T > 0, "fd_ndac_decode_ragged: bad arguments");
  hipStream_t st = fd_stream(stream);
  FD_TRY(fd_ndac_check_frames("fd_ndac_decode_ragged", frames, B, T, st));   // the bounds the kernels index with are checked before anything is launched
  return fd_ndac_decode_walk(m, "fd_ndac_decode_ragged", z, frames, B, T, audio, ws, ws_bytes, st);
}
