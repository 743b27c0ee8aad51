// ndac_plan.h -- the structure of the NDAC codec, stated ONCE and host-only (plain C++17, no HIP; tests/c/ndac_plan_check.cpp builds it
// alone): the parameter table, one record per convolution of the encoder and of the decoder in execution order, and everything that
// follows from walking those records -- lengths, the workspace's widest tensor, the frame-table advance, the preconditions of the
// whole-frame arithmetic and the two streaming halos.  ndac.hip builds a plan at fd_ndac_create, resolves the records' device pointers at
// fd_ndac_finalize and runs both stacks as a loop over them.
//
//   encoder  WNConv1d(1, d, 7) -> [ 3 x ResidualUnit(dilation 1, 3, 9) -> Snake -> WNConv1d(k = 2 s, stride s) ] per rate -> Snake -> WNConv1d(., latent, 3)
//   decoder  WNConv1d(latent, D, 7) -> [ Snake -> WNConvTranspose1d(k = 2 s, stride s) -> 3 x ResidualUnit ] per rate -> Snake -> WNConv1d(., 1, 7) -> tanh
//   ResidualUnit(x) = x + WNConv1d(k = 1)(Snake(WNConv1d(k = 7, dilation)(Snake(x))))
#pragma once
#include <string>
#include <vector>

#include "flowdec_hip.h"

namespace ndac {

struct Param {
  std::string name;          // state_dict name, `.weight` in place of `.weight_g` / `.weight_v`
  std::vector<int> shape;
  long long numel() const { long long n = 1; for (int s : shape) n *= s; return n; }
};

// Inside the codec every Snake is applied ONCE, by the layer that produces the tensor (second output of its epilogue), never by the
// consumers: the activated input of a 768-channel convolution would otherwise be recomputed by each of its 24 channel-tile workgroups
// (sinf + a division per element).  Same function on the same float32 values: bit-identical to activating at the consumer.
struct Layer {
  bool transposed = false;
  int Ci = 0, Co = 0, K = 0, stride = 1, pad = 0, dil = 1;
  int weight = -1, bias = -1;   // parameter-table indices
  int alpha_out = -1;           // the Snake behind this layer, fused into its epilogue (parameter index), or -1
  bool residual = false;        // the closing 1x1 of a ResidualUnit: adds the unit's raw input; its input is the unit's mid tensor
  bool keep_raw = false;        // the raw result is stored too: a ResidualUnit's input (its residual operand), or the stack's result
  bool tanh_out = false;        // the decoder's output layer
  // device pointers, resolved by fd_ndac_finalize: weight as [Ci][K][Co], bias, the split-bf16 copy for ndac_mfma.hip or null, alpha_out's values or null
  const float* w = nullptr; const float* b = nullptr; const void* packed = nullptr; const float* alpha = nullptr;

  long long out_len(long long T) const {
    return transposed ? (T - 1) * stride - 2 * pad + (long long)dil * (K - 1) + 1 : (T + 2 * pad - (long long)dil * (K - 1) - 1) / stride + 1;
  }
  // A clip of frames * mul + add positions at this layer's input is frames * mul' + add' at its output (the length rule is affine in the
  // frame count: exactly for the transposed layers, and for a strided one on the whole-frame lengths Plan::whole_frames_error admits).
  void advance(int& mul, int& add) const {
    if (stride == 1) return;
    if (transposed) { mul *= stride; add = add * stride + K - stride - 2 * pad; }
    else mul /= stride;
  }
  // the input positions that outputs [lo, hi] depend on (real arithmetic: no clamping at the signal's ends)
  void depends_on(long long& lo, long long& hi) const {
    auto fl = [](long long a, long long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); };
    if (transposed) { lo = -fl(-(lo + pad - (K - 1)), stride); hi = fl(hi + pad, stride); }   // ceil((lo + p - (K - 1)) / s) .. floor((hi + p) / s)
    else { lo = lo * stride - pad; hi = hi * stride - pad + (long long)(K - 1) * dil; }
  }
};

struct Quantizer { int in_w, in_b, out_w, out_b, codebook; };   // parameter-table indices of one codebook

inline long long stack_out_len(const std::vector<Layer>& s, long long T) { for (const Layer& l : s) T = l.out_len(T); return T; }

// widest tensor a stack writes (elements per batch item) for an input of length T: what one workspace slot must hold
inline long long stack_widest(const std::vector<Layer>& s, long long T) {
  long long mx = 0;
  for (const Layer& l : s) { T = l.out_len(T); if ((long long)l.Co * T > mx) mx = (long long)l.Co * T; }
  return mx;
}

inline void stack_depends_on(const std::vector<Layer>& s, long long& lo, long long& hi) {
  for (size_t i = s.size(); i-- > 0;) s[i].depends_on(lo, hi);
}

struct Plan {
  fd_ndac_config cfg{};
  int hop = 1;   // samples per latent frame on the encoder side
  int up = 1;    // decoded samples per latent frame where the decoder rates are even
  std::vector<Param> params;
  std::vector<Layer> enc, dec;
  std::vector<Quantizer> quant;
  // Frame tables and windows count in whole frames: n hops of samples must be n frames, and n hops / (the strides so far) positions at
  // every layer.  A strided convolution (K = 2 s, padding ceil(s / 2)) maps a length n s to n for every s >= 2, even or odd; a rate of 1
  // maps n to n + 1 (a later stride can absorb that in the frame count, but not at the layers in between).  Empty = the encoder qualifies.
  std::string whole_frames_error;
  // The decoder makes T * up samples of T frames only with even rates (an odd one leaves (T - 1) s + s - 1).  Empty = it does.
  std::string even_rates_error;

  int find(const char* name) const {
    for (size_t i = 0; i < params.size(); ++i) if (params[i].name == name) return (int)i;
    return -1;
  }
  long long latent_frames(long long L) const { return stack_out_len(enc, L); }
  long long decoded_length(long long T) const { return stack_out_len(dec, T); }
  // elements per batch item of ONE of the five workspace slots that cover encode of L samples and decode of its frames
  long long slot_elems(long long L) const {
    long long T = latent_frames(L);
    if (T < 1) T = 1;
    long long e = stack_widest(enc, L);
    for (long long o : {stack_widest(dec, T), (long long)cfg.latent_dim * T}) if (o > e) e = o;
    return e;
  }
  // Latent frames before / after a frame whose samples can reach that frame: frame 0 walked backwards through the encoder, in whole hops
  // of samples around the frame's own [0, hop).
  void encode_halo(int* left, int* right) const {
    long long lo = 0, hi = 0;
    stack_depends_on(enc, lo, hi);
    *left = (int)((-lo + hop - 1) / hop);
    *right = (int)((hi - (hop - 1) + hop - 1) / hop);
  }
  // Latent frames before / after a frame that can reach that frame's output samples: each sample of frame 0 walked backwards through
  // the decoder, the maximum over the frame.
  void decode_halo(int* left, int* right) const {
    long long hl = 0, hr = 0;
    for (int n = 0; n < up; ++n) {
      long long lo = n, hi = n;
      stack_depends_on(dec, lo, hi);
      if (-lo > hl) hl = -lo;
      if (hi > hr) hr = hi;
    }
    *left = (int)hl; *right = (int)hr;
  }
};

inline Plan make_plan(const fd_ndac_config& c) {
  Plan p;
  p.cfg = c;
  std::vector<Layer>* stack = &p.enc;
  auto add = [&](const std::string& n, std::vector<int> shape) { p.params.push_back({n, std::move(shape)}); return (int)p.params.size() - 1; };
  auto conv = [&](const std::string& n, int ci, int co, int k, int stride, int pad, int dil, bool tr = false) {
    Layer l;
    l.transposed = tr; l.Ci = ci; l.Co = co; l.K = k; l.stride = stride; l.pad = pad; l.dil = dil;
    l.weight = add(n + ".weight", tr ? std::vector<int>{ci, co, k} : std::vector<int>{co, ci, k});   // nn.ConvTranspose1d keeps [Ci][Co][K]
    l.bias = add(n + ".bias", {co});
    stack->push_back(l);
  };
  auto snake = [&](const std::string& n, int ch) { stack->back().alpha_out = add(n + ".alpha", {1, ch, 1}); };
  auto res_unit = [&](const std::string& n, int dim, int dil) {
    snake(n + ".block.0", dim); conv(n + ".block.1", dim, dim, 7, 1, 3 * dil, dil);
    snake(n + ".block.2", dim); conv(n + ".block.3", dim, dim, 1, 1, 0, 1);
    stack->back().residual = true;
  };
  auto finish = [&] {   // raw results: only where a ResidualUnit starts behind the layer (its 1x1 sits two records on), and the stack's own
    std::vector<Layer>& s = *stack;
    for (size_t i = 0; i < s.size(); ++i) s[i].keep_raw = i + 1 == s.size() || (i + 2 < s.size() && s[i + 2].residual);
  };
  const int dils[3] = {1, 3, 9};
  auto num = [](int i) { return std::to_string(i); };

  int d = c.encoder_dim;
  conv("encoder.block.0", 1, d, 7, 1, 3, 1);
  for (int i = 0; i < c.n_encoder_rates; ++i) {
    const int s = c.encoder_rates[i];
    const std::string b = "encoder.block." + num(i + 1);
    for (int j = 0; j < 3; ++j) res_unit(b + ".block." + num(j), d, dils[j]);
    snake(b + ".block.3", d); conv(b + ".block.4", d, 2 * d, 2 * s, s, (s + 1) / 2, 1);
    d *= 2;
    p.hop *= s;
    if (s < 2 && p.whole_frames_error.empty())
      p.whole_frames_error = "encoder rate " + num(i) + " is a rate of 1 (a layer that makes n + 1 positions of n: no whole-frame arithmetic)";
  }
  snake("encoder.block." + num(c.n_encoder_rates + 1), d);
  conv("encoder.block." + num(c.n_encoder_rates + 2), d, c.latent_dim, 3, 1, 1, 1);
  finish();
  for (int n = 1; n <= 3 && p.whole_frames_error.empty(); ++n)
    if (p.latent_frames((long long)n * p.hop) != n)
      p.whole_frames_error = "the encoder rates give " + num((int)p.latent_frames((long long)n * p.hop)) + " frames for " + num(n) + " hops of samples";

  for (int i = 0; i < c.n_codebooks; ++i) {   // 1x1 convolutions in state_dict form; the RVQ kernels take them as matrices
    const std::string q = "quantizer.quantizers." + num(i);
    Quantizer r;
    r.in_w = add(q + ".in_proj.weight", {c.codebook_dim, c.latent_dim, 1}); r.in_b = add(q + ".in_proj.bias", {c.codebook_dim});
    r.out_w = add(q + ".out_proj.weight", {c.latent_dim, c.codebook_dim, 1}); r.out_b = add(q + ".out_proj.bias", {c.latent_dim});
    r.codebook = add(q + ".codebook.weight", {c.codebook_size, c.codebook_dim});
    p.quant.push_back(r);
  }

  stack = &p.dec;
  d = c.decoder_dim;
  conv("decoder.model.0", c.latent_dim, d, 7, 1, 3, 1);
  for (int i = 0; i < c.n_decoder_rates; ++i) {
    const int s = c.decoder_rates[i];
    const std::string b = "decoder.model." + num(i + 1);
    snake(b + ".block.0", d); conv(b + ".block.1", d, d / 2, 2 * s, s, (s + 1) / 2, 1, /*transposed*/ true);
    d /= 2;
    for (int j = 0; j < 3; ++j) res_unit(b + ".block." + num(j + 2), d, dils[j]);
    p.up *= s;
    if (s % 2 && p.even_rates_error.empty())
      p.even_rates_error = "decoder rate " + num(s) + " is odd (the decoded length is not frames * hop: no window arithmetic)";
  }
  snake("decoder.model." + num(c.n_decoder_rates + 1), d);
  conv("decoder.model." + num(c.n_decoder_rates + 2), d, 1, 7, 1, 3, 1);
  stack->back().tanh_out = true;
  finish();
  return p;
}

}  // namespace ndac
