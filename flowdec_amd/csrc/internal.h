// internal.h -- cross-file (non-ABI) declarations of libflowdec_hip.so.
#pragma once
#include "common.h"

struct fd_temb_job {
  const float* dense_w;  // [Cout][temb_dim]
  const float* dense_b;  // [Cout]
  const float* conv_b;   // [Cout]
  float* out;            // [nt][Cout]
  int Cout;
};

// Where a [B][F][T] plane of sampler noise comes from: a caller-filled buffer (`ptr`), or the clips' seeds (DEVICE uint64 [B]) and the
// index of the draw -- then the consuming kernel generates the plane in registers (noise.h).  frame0 (DEVICE int32 [B], with seeds
// only; nullptr = zeros): the absolute frame of every row's first column -- the rows are chunks of longer recordings
struct fd_noise_src {
  const float* ptr = nullptr;
  const unsigned long long* seeds = nullptr;
  int draw = 0;
  const int* frame0 = nullptr;
};

struct fd_edge_args {
  const void* x = nullptr;   // main input (4-channel NHWC tensor, or complex x for pack)
  const void* y = nullptr;   // second input (complex y for pack; h for combine)
  const float* w = nullptr;
  const float* bias = nullptr;
  void* out = nullptr;
  const void* base = nullptr;  // output_update
  const void* kold = nullptr;
  void* ksave = nullptr;
  float* stats = nullptr;      // combine: [B][fd_combine_tiles][Cout][2] GroupNorm partials of the output
  float coef = 1.f;
  fd_noise_src z;              // score update: dst = cb*base + cy*y + coef*v + cz*z
  float cb = 1.f, cy = 0.f, cz = 0.f;
  const float* ctab = nullptr; // score update, per-clip form: (cb, cy, coef) of clip b from ctab[b][0..2] (DEVICE [B][3]); no noise term
  int B = 0, H = 0, W = 0, Cout = 0;
  int ks = 1;                  // output layer (output_update, score_update): 1x1 or 3x3 (zero padding 'same'; w = [2][4][3][3])
};

// net_edges.hip
int fd_time_embedding_impl(const float* t, float t_imm, int nt, const float* gfp_w, int nf, const float* w1, const float* b1,
                           const float* w2, const float* b2, float* temb, hipStream_t st);
int fd_temb_bias_batched(const fd_temb_job* jobs_dev, int njobs, const float* temb, int nt, int temb_dim, hipStream_t st);
// ops_api.hip: the argument checks of the public time-conditioning entry points (fd_time_embedding, fd_temb_bias and their fd_op_*
// forms): FD_EINVAL with a message that names the argument, before any device call.  `who` = the entry point's name.
int fd_check_time_embedding(const char* who, int nt, const float* gfp_w, int nf, const float* w1, const float* b1, const float* w2,
                            const float* b2, const float* temb);
int fd_check_temb_bias(const char* who, const float* temb, int nt, int temb_dim);
int fd_check_temb_job(const char* who, int job, const float* dense_w, const float* dense_b, const float* out, int Cout);
// net_edges.hip: the edge ops, each on the fields of fd_edge_args it names there -- pack_input; combine (1x1 4->Cout + h); output layer +
// state update; output layer + score-sampler update (per clip when a.ctab is set); input convolution 3x3 4 -> Cout (x = packed input,
// w = [Cout][4][3][3] f32) with the GroupNorm partials of its output in `stats` ([B][(H / 16) * (W / 16)][Cout][2])
int fd_edge_pack_input(const fd_edge_args& a, int dtype, hipStream_t st);
int fd_edge_combine(const fd_edge_args& a, int dtype, hipStream_t st);
int fd_edge_output_update(const fd_edge_args& a, int dtype, hipStream_t st);
int fd_edge_score_update(const fd_edge_args& a, int dtype, hipStream_t st);
int fd_edge_conv_in(const fd_edge_args& a, int dtype, hipStream_t st);
int fd_combine_tiles(int H, int W);
// solver_ops.hip
int fd_init_state(const float* Y, const fd_noise_src& noise, const double* sigma_dev, int sigma_n, float sigma_fac, float* x0, int B,
                  int F, int T, hipStream_t st);
// adaptive solver helpers: dst = cx * x + dt * sum c[i] k[i];  partial[b] = sum |p - q|^2 / (atol + rtol max(|r|, |s|))^2
int fd_ode_lincomb(const float* x, float cx, float dt, const float* const* k, const float* c, int nk, float* dst, long long n, hipStream_t st);
int fd_ode_scaled_sq(const float* p, const float* q, const float* r, const float* s, float atol, float rtol, double* partial, int nblocks,
                     long long n, hipStream_t st);
// the same per clip of a [B][n] state: dt_dev = DEVICE float [B]; partial = [B][nblocks], row b = what fd_ode_scaled_sq gives on clip b alone
int fd_ode_lincomb_clips(const float* x, float cx, const float* dt_dev, const float* const* k, const float* c, int nk, float* dst, int B, long long n,
                         hipStream_t st);
int fd_ode_scaled_sq_clips(const float* p, const float* q, const float* r, const float* s, float atol, float rtol, double* partial, int nblocks, int B,
                           long long n, hipStream_t st);
// clips with accept[b] != 0 (DEVICE int32 [B]): x <- x_new, k0 <- k6, and traj[ckpt[b]][b] <- x_new where ckpt[b] > 0 and traj is given
int fd_ode_commit_clips(const int* accept, const int* ckpt, const float* x_new, const float* k6, float* x, float* k0, float* traj, int B, long long n,
                        hipStream_t st);
// dst = a + cq * q, q = a [B][F][T] plane of noise
int fd_caxpy(const float* a, const fd_noise_src& q, float cq, float* dst, int B, int F, int T, hipStream_t st);
// conv_mfma.hip
int fd_conv_init_attributes();
// stft.hip
// (fd_stft_plan / fd_stft_plan_create / fd_stft_plan_destroy: public, include/flowdec_hip.h)
// lens: device int32 [B] per-clip sample counts of a ragged batch, or nullptr (every clip is L samples long)
// normfac_in: device float [B] factors given by the caller (the rows are chunks of files normalised as a whole), or nullptr; when given,
// no maximum is taken and `normfac` is not written
int fd_stft_forward(fd_stft_plan* p, const float* y, const int* lens, int B, int L, float alpha, float beta, int normalize, float* normfac,
                    float* Y, int T_pad, void* ws, size_t ws_bytes, hipStream_t st, const float* normfac_in = nullptr);
int fd_stft_inverse(fd_stft_plan* p, const float* X, const int* lens, int B, int T, int T_pad, float alpha, float beta, const float* normfac,
                    float* y, int L, void* ws, size_t ws_bytes, hipStream_t st);
size_t fd_stft_ws_bytes(int B, int L, int n_fft, int hop);
// for metrics.hip: the plan's geometry, the GEMM width of one n_fft, and framing (no normalisation) + DFT GEMM into caller buffers
// frames / spec, both [B * (1 + L / hop)][kpad] float32
void fd_stft_plan_dims(const fd_stft_plan* p, int* n_fft, int* hop, int* n_freq, int* kpad);
int fd_stft_kpad(int n_fft);
int fd_stft_raw_spectrum(fd_stft_plan* p, const float* y, const int* lens, int B, int L, float* frames, float* spec, hipStream_t st);
// resample.hip, for stoi.hip: the plan's rates and bank geometry (any pointer may be null)
void fd_resample_plan_dims(const fd_resample_plan* p, int* o, int* n, int* width, int* K);
// ndac_mfma.hip: the codec's wide convolutions on the matrix cores (split-bf16 operands, f32 tolerance)
bool fd_ndac_mfma_supported(int Ci, int Co, int K, int stride, int dil, int transposed);
// (fd_ndac_mfma_packed_bytes: public, include/flowdec_hip.h)
void fd_ndac_mfma_pack(const float* w_ci_k_co, int Ci, int Co, int K, int stride, int transposed, void* dst);
// Ragged decode (fd_ndac_decode_ragged): clip b of a layer's input is frames[b] * mul + add positions long (frames: device int32 [B], the
// clips' LATENT frame counts; every decoder layer's length rule is affine in them).  frames == nullptr: every clip fills the row.
struct fd_ndac_lens { const int* frames = nullptr; int mul = 1, add = 0; };
int fd_ndac_mfma_conv(const float* x, const void* wp, const float* bias, const float* res, float* out, float* out_act, const float* alpha_out, int B,
                      int Ci, int T, int Co, int K, int stride, int pad, int dil, int transposed, hipStream_t st, fd_ndac_lens lens = {});
// ndac.hip: PyTorch weight layout ([Co][Ci][K] conv, [Ci][Co][K] transposed) -> the codec's own [Ci][K][Co] (host memory)
void fd_ndac_weight_ci_k_co(const float* w, int Ci, int Co, int K, int transposed, float* dst);
// attn.hip: the bottleneck attention block (x -> out, GroupNorm affine given); qkv = f32 workspace of fd_attn_qkv_bytes; stats (optional) =
// GroupNorm partials of out, [B][fd_attn_stats_tiles(H, W)][C][2]
size_t fd_attn_qkv_bytes(int B, int N, int C);
int fd_attn_stats_tiles(int H, int W);
int fd_attn_launch(const void* x, const float* affine, const fd_attn_desc& d, float* qkv, void* out, float* stats, int B, int N, int dtype,
                   hipStream_t st);
