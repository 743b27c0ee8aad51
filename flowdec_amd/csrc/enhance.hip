// enhance.hip -- the waveform entry points of the three model classes (FlowModel.enhance, model.py:476-528; ScoreModel / RegressionModel,
// model.py:539-690): one front end / back end, enhance_common (STFT -> body -> iSTFT, hipGraph-captured), over one workspace layout,
// enhance_layout, with the flow / score / regression bodies from solve.hip and model.hip; and the validation loss fd_valid_loss.
#include <stdint.h>

#include "model_internal.h"
#include "step_ctl.h"

using namespace fdm;

// The workspace of every enhance entry point: Y | X | normfac[B] | rest (the larger of the transform's and the body's scratch).
namespace {
struct enhance_layout_t { size_t state, normfac, rest, total; int T, Tp; };
bool enhance_layout(const fd_model* m, int B, int L, enhance_layout_t& s) {
  if (!m || B <= 0 || L <= 0) return false;
  s.T = 1 + L / m->cfg.hop; s.Tp = fd_padded_frames(s.T);
  if (check_shape(m, B, s.Tp) != FD_OK) return false;
  const size_t state = fd_align(sizeof(float) * 2 * (size_t)B * m->n_freq * s.Tp);
  s.state = state;
  s.normfac = 2 * state;
  s.rest = 2 * state + fd_align(sizeof(float) * B);
  const size_t a = fd_stft_ws_bytes(B, L, m->cfg.n_fft, m->cfg.hop), b = ode_ws_bytes(m, B, s.Tp);
  s.total = s.rest + (a > b ? a : b) + 256;
  return true;
}
}  // namespace

extern "C" size_t fd_enhance_workspace_bytes(const fd_model* m, int B, int L) {
  enhance_layout_t s;
  return enhance_layout(m, B, L, s) ? s.total : 0;
}

extern "C" size_t fd_enhance_normfac_offset(const fd_model* m, int B, int L) {
  enhance_layout_t s;
  return enhance_layout(m, B, L, s) ? s.normfac : 0;
}

// Shared front end / back end of the three enhancement models:  STFT -> body(Y, X) -> iSTFT.  lens (device int32 [B]) = a ragged batch
// (see fd_enhance_ragged), nullptr = every clip is L samples long.  normfac_in (device float [B], fd_enhance_chunks) replaces the clips' own
// maxima: the front end divides by it, the back end multiplies by it, and the workspace's normfac slot stays unwritten.
template <typename Body>
static int enhance_common(fd_model* m, const char* who, const float* y, const int* lens, float* x_hat, int B, int L, void* ws, size_t ws_bytes,
                          GraphKey key, int use_graph, void* stream, Body&& body, const float* normfac_in = nullptr) {
  FD_TRY(check_ready(m));
  FD_REQUIRE(y && x_hat && ws, "%s: null pointer", who);
  FD_REQUIRE(B > 0 && L > m->cfg.n_fft / 2, "%s: clips must be longer than %d samples", who, m->cfg.n_fft / 2);
  enhance_layout_t lay;
  if (!enhance_layout(m, B, L, lay)) return FD_EINVAL;   // check_shape has left the message
  if (ws_bytes < lay.total) return fd_set_error(FD_ENOMEM, "%s: workspace %zu < required %zu bytes", who, ws_bytes, lay.total);
  hipStream_t st = fd_stream(stream);
  const int T = lay.T, Tp = lay.Tp;
  float* Y = (float*)ws;
  float* X = (float*)((char*)ws + lay.state);
  float* normfac = (float*)((char*)ws + lay.normfac);
  char* rest = (char*)ws + lay.rest;
  const size_t rest_bytes = ws_bytes - lay.rest;
  key.y = y; key.xhat = x_hat; key.ws = ws; key.lens = lens; key.B = B; key.L = L; key.normalize = m->normalize; key.normfac_in = normfac_in;
  return run_maybe_graph(m, key, use_graph != 0, st, [&]() {
    FD_TRY(fd_stft_forward(m->stft, y, lens, B, L, m->cfg.alpha, m->cfg.beta, m->normalize, normfac, Y, Tp, rest, rest_bytes, st, normfac_in));
    FD_TRY(body(Y, X, Tp, (void*)rest, rest_bytes, st));
    FD_TRY(fd_stft_inverse(m->stft, X, lens, B, T, Tp, m->cfg.alpha, m->cfg.beta, normfac_in ? normfac_in : normfac, x_hat, L, rest, rest_bytes, st));
    return FD_OK;
  });
}

// The flow model's entry points: the noise source, N and the solver are theirs; the body is the fixed-step solver.
static int flow_enhance_impl(fd_model* m, const char* who, const float* y, const int* lens, const fd_noise_src& noise, float sigma_fac, int N, int solver,
                             float* x_hat, int B, int L, void* ws, size_t ws_bytes, int use_graph, void* stream, const float* normfac_in = nullptr) {
  FD_TRY(check_ready(m));
  FD_REQUIRE(noise.ptr || noise.seeds, "%s: null pointer", who);
  FD_REQUIRE(N >= 1 && solver_nfe(solver, N) > 0, "%s: bad N / solver", who);
  GraphKey key; key.noise = noise.ptr; key.seeds = noise.seeds; key.frame0 = noise.frame0; key.N = N; key.solver = solver; key.sigma_fac = sigma_fac; key.kind = 2;
  return enhance_common(m, who, y, lens, x_hat, B, L, ws, ws_bytes, key, use_graph, stream,
                        [&](float* Y, float* X, int Tp, void* rest, size_t rest_bytes, hipStream_t st) {
                          return ode_enqueue(m, Y, noise, sigma_fac, N, solver, X, nullptr, B, Tp, rest, rest_bytes, st);
                        }, normfac_in);
}

extern "C" int fd_enhance(fd_model* m, const float* y, const float* noise, float sigma_fac, int N, int solver, float* x_hat, int B, int L, void* ws,
                          size_t ws_bytes, int use_graph, void* stream) {
  FD_MODEL_ENTER(m, "fd_enhance");
  return flow_enhance_impl(m, "fd_enhance", y, nullptr, fd_noise_src{noise}, sigma_fac, N, solver, x_hat, B, L, ws, ws_bytes, use_graph, stream);
}

// FlowModel.enhance on a RAGGED batch: the reference's driver enhances a directory file by file (enhance.py:96-137), every file its
// own length; here the files whose spectrograms pad to the same T_pad (util/other.py:25-52) run as ONE batch.  y / x_hat are [B][L]
// rows (L = the longest clip; workspace as for fd_enhance(B, L)), lengths (device int32 [B]) the clips' own sample counts -- the
// CALLER guarantees fd_padded_frames(fd_num_frames(lengths[b])) == fd_padded_frames(fd_num_frames(L)) for every b (the kernels
// clamp a length into (n_fft/2, L]).  Clip b's result is bit-identical to fd_enhance on that clip alone with the same noise
// (noise is [B][1][F][T_pad] as usual); samples [lengths[b], L) of a row of x_hat are zero.  The hipGraph of a (B, L) bucket is
// keyed on the POINTER `lengths`: its contents may change between replays.
extern "C" int fd_enhance_ragged(fd_model* m, const float* y, const int* lengths, const float* noise, float sigma_fac, int N, int solver,
                                 float* x_hat, int B, int L, void* ws, size_t ws_bytes, int use_graph, void* stream) {
  FD_MODEL_ENTER(m, "fd_enhance_ragged");
  FD_REQUIRE(lengths, "fd_enhance_ragged: null lengths");
  return flow_enhance_impl(m, "fd_enhance_ragged", y, lengths, fd_noise_src{noise}, sigma_fac, N, solver, x_hat, B, L, ws, ws_bytes, use_graph, stream);
}

// fd_enhance (lengths == NULL) / fd_enhance_ragged with the initial noise generated from the clips' seeds (DEVICE uint64 [B], draw index 0):
// no noise buffer exists.  A captured graph is keyed on the POINTERS `seeds` and `lengths`; their contents may change between replays.
extern "C" int fd_enhance_seeded(fd_model* m, const float* y, const int* lengths, const unsigned long long* seeds, float sigma_fac, int N, int solver,
                                 float* x_hat, int B, int L, void* ws, size_t ws_bytes, int use_graph, void* stream) {
  FD_MODEL_ENTER(m, "fd_enhance_seeded");
  return flow_enhance_impl(m, "fd_enhance_seeded", y, lengths, fd_noise_src{nullptr, seeds, 0}, sigma_fac, N, solver, x_hat, B, L, ws, ws_bytes, use_graph, stream);
}

// Long-form: the rows are CHUNKS of longer recordings.  fd_enhance_seeded on ragged rows plus two optional device arrays: frame0 (int32 [B]:
// the absolute frame of each row's first column -- the seeded noise is then the recording's, z(seed, 0, f, frame0[b] + t)) and normfac_in
// (float [B]: the recording's normalisation factor from fd_normfac -- no per-row maximum is taken; the front end divides by it, the back
// end multiplies by it, and the workspace's normfac slot is not written).  Both NULL = fd_enhance_seeded, bit for bit.  A captured graph is
// additionally keyed on the two POINTERS.
extern "C" int fd_enhance_chunks(fd_model* m, const float* y, const int* lengths, const unsigned long long* seeds, const int* frame0,
                                 const float* normfac_in, float sigma_fac, int N, int solver, float* x_hat, int B, int L, void* ws, size_t ws_bytes,
                                 int use_graph, void* stream) {
  FD_MODEL_ENTER(m, "fd_enhance_chunks");
  FD_REQUIRE(seeds, "fd_enhance_chunks: null seeds");
  return flow_enhance_impl(m, "fd_enhance_chunks", y, lengths, fd_noise_src{nullptr, seeds, 0, frame0}, sigma_fac, N, solver, x_hat, B, L, ws, ws_bytes, use_graph,
                      stream, normfac_in);
}

static int score_enhance_impl(fd_model* m, const char* who, const float* y, const int* lens, const fd_noise_src& noise, const fd_score_config* c,
                              float* x_hat, int B, int L, void* ws, size_t ws_bytes, int use_graph, void* stream, const float* normfac_in = nullptr) {
  FD_REQUIRE(c && (noise.ptr || noise.seeds), "%s: null pointer", who);
  FD_REQUIRE(c->N >= 1, "%s: N must be >= 1", who);
  FD_REQUIRE(c->predictor >= FD_PREDICTOR_REVERSE_DIFFUSION && c->predictor <= FD_PREDICTOR_NONE, "%s: unknown predictor id %d", who, c->predictor);
  FD_REQUIRE(c->corrector == FD_CORRECTOR_ALD || c->corrector == FD_CORRECTOR_NONE, "%s: unknown corrector id %d", who, c->corrector);
  FD_REQUIRE(c->corrector_steps >= 0 && c->corrector_steps <= 64, "%s: corrector_steps out of range", who);
  FD_REQUIRE(c->sigma_min > 0.f && c->sigma_max > c->sigma_min && c->theta > 0.f, "%s: bad OUVE parameters", who);
  FD_REQUIRE(c->t_eps > 0.f && c->t_eps < 1.f, "%s: t_eps must be in (0, 1)", who);
  GraphKey key; key.noise = noise.ptr; key.seeds = noise.seeds; key.frame0 = noise.frame0; key.kind = 3; key.score = *c;
  const fd_score_config cfg = *c;
  return enhance_common(m, who, y, lens, x_hat, B, L, ws, ws_bytes, key, use_graph, stream,
                        [&](float* Y, float* X, int Tp, void* rest, size_t rest_bytes, hipStream_t st) {
                          return score_enqueue(m, Y, noise, cfg, X, B, Tp, rest, rest_bytes, st);
                        }, normfac_in);
}

extern "C" int fd_score_enhance(fd_model* m, const float* y, const float* noise, const fd_score_config* c, float* x_hat, int B, int L, void* ws,
                                size_t ws_bytes, int use_graph, void* stream) {
  FD_MODEL_ENTER(m, "fd_score_enhance");
  return score_enhance_impl(m, "fd_score_enhance", y, nullptr, fd_noise_src{noise}, c, x_hat, B, L, ws, ws_bytes, use_graph, stream);
}

// fd_score_enhance with every Gaussian plane generated from the clips' seeds inside the kernel that consumes it: draw index k = the k-th plane
// fd_score_enhance would read
extern "C" int fd_score_enhance_seeded(fd_model* m, const float* y, const unsigned long long* seeds, const fd_score_config* c, float* x_hat, int B,
                                       int L, void* ws, size_t ws_bytes, int use_graph, void* stream) {
  FD_MODEL_ENTER(m, "fd_score_enhance_seeded");
  return score_enhance_impl(m, "fd_score_enhance_seeded", y, nullptr, fd_noise_src{nullptr, seeds, 0}, c, x_hat, B, L, ws, ws_bytes, use_graph, stream);
}

// ScoreModel.enhance on a RAGGED batch: the contract of fd_enhance_ragged (y / x_hat are [B][L] rows, lengths = device int32 [B], the
// CALLER guarantees one T_pad bucket, clip b bit-identical to the one-clip call with the same noise or seed, samples [lengths[b], L) of a
// row of x_hat zero, workspace fd_enhance_workspace_bytes(m, B, L)).  Exactly one of noise ([draws][B][F][T_pad]) and seeds (device uint64
// [B]) is given.  The sampler's update kernels work per element of [B][F][T_pad] and the network never mixes batch items, so the lengths
// only reach the STFT / iSTFT.  A captured graph is keyed on the POINTERS lengths / noise / seeds and on the score configuration.
extern "C" int fd_score_enhance_ragged(fd_model* m, const float* y, const int* lengths, const float* noise, const unsigned long long* seeds,
                                       const fd_score_config* c, float* x_hat, int B, int L, void* ws, size_t ws_bytes, int use_graph, void* stream) {
  FD_MODEL_ENTER(m, "fd_score_enhance_ragged");
  FD_REQUIRE(lengths, "fd_score_enhance_ragged: null lengths");
  FD_REQUIRE((noise != nullptr) != (seeds != nullptr), "fd_score_enhance_ragged: exactly one of noise and seeds must be given (got %s)",
             noise ? "both" : "neither");
  FD_REQUIRE(B > 0, "fd_score_enhance_ragged: B must be positive (got %d)", B);
  const fd_noise_src src = noise ? fd_noise_src{noise} : fd_noise_src{nullptr, seeds, 0};
  return score_enhance_impl(m, "fd_score_enhance_ragged", y, lengths, src, c, x_hat, B, L, ws, ws_bytes, use_graph, stream);
}

// Long-form for the score sampler: fd_score_enhance_ragged on seeds plus the two optional device arrays of fd_enhance_chunks.  frame0 (int32
// [B]) makes EVERY one of the fd_score_num_draws planes the recording's -- z(seed, draw, f, frame0[b] + t): the prior and each predictor /
// corrector step of two overlapping rows see bit-identical noise where they overlap; normfac_in (float [B]) replaces the per-row maximum in
// the front and back end.  Both NULL = fd_score_enhance_ragged(seeds), bit for bit.  A captured graph is keyed on the POINTERS lengths, seeds,
// frame0 and normfac_in and on the values of *c.
extern "C" int fd_score_enhance_chunks(fd_model* m, const float* y, const int* lengths, const unsigned long long* seeds, const int* frame0,
                                       const float* normfac_in, const fd_score_config* c, float* x_hat, int B, int L, void* ws, size_t ws_bytes,
                                       int use_graph, void* stream) {
  FD_MODEL_ENTER(m, "fd_score_enhance_chunks");
  FD_REQUIRE(lengths, "fd_score_enhance_chunks: null lengths");
  FD_REQUIRE(seeds, "fd_score_enhance_chunks: null seeds");
  FD_REQUIRE(B > 0, "fd_score_enhance_chunks: B must be positive (got %d)", B);
  return score_enhance_impl(m, "fd_score_enhance_chunks", y, lengths, fd_noise_src{nullptr, seeds, 0, frame0}, c, x_hat, B, L, ws, ws_bytes, use_graph,
                            stream, normfac_in);
}

// ---- the ODE sampler from waveform to waveform: enhance_common's front end and back end around score_ode_run (solve.hip), eagerly -- the
// adaptive loop reads an error norm back per attempt, so there is nothing to capture.  Workspace: Y | X | normfac[B] | rest, rest = the
// larger of the transform's and the adaptive driver's.
namespace {
bool score_ode_layout(const fd_model* m, int B, int L, bool per_clip, enhance_layout_t& s) {
  if (!enhance_layout(m, B, L, s)) return false;
  const size_t a = fd_stft_ws_bytes(B, L, m->cfg.n_fft, m->cfg.hop), b = score_ode_ws_bytes(m, B, s.Tp, per_clip);
  s.total = s.rest + (a > b ? a : b) + 256;
  return true;
}
}  // namespace

extern "C" size_t fd_score_ode_enhance_workspace_bytes(const fd_model* m, int B, int L, int step_control) {
  enhance_layout_t s;
  if (step_control != FD_STEP_CONTROL_BATCH && step_control != FD_STEP_CONTROL_CLIP) return 0;
  if (step_control == FD_STEP_CONTROL_CLIP && B > fd_model::MAX_NT) return 0;
  return score_ode_layout(m, B, L, step_control == FD_STEP_CONTROL_CLIP, s) ? s.total : 0;
}

extern "C" int fd_score_ode_enhance(fd_model* m, const float* y, const int* lengths, const float* noise, const unsigned long long* seeds,
                                    const fd_score_config* cfg, float rtol, float atol, int step_control, float* x_hat, int* nfe_out,
                                    int* rejected_out, int* evals_out, int B, int L, void* ws, size_t ws_bytes, void* stream) {
  FD_MODEL_ENTER(m, "fd_score_ode_enhance");
  FD_TRY(check_ready(m));
  FD_REQUIRE(y && x_hat && ws && nfe_out, "fd_score_ode_enhance: null pointer");
  FD_REQUIRE((noise != nullptr) != (seeds != nullptr), "fd_score_ode_enhance: give exactly one of noise and seeds");
  FD_REQUIRE(B > 0 && L > m->cfg.n_fft / 2, "fd_score_ode_enhance: clips must be longer than %d samples", m->cfg.n_fft / 2);
  FD_TRY(score_ode_check("fd_score_ode_enhance", cfg, rtol, atol, step_control, B));
  const bool per_clip = step_control == FD_STEP_CONTROL_CLIP;
  enhance_layout_t lay;
  if (!score_ode_layout(m, B, L, per_clip, lay)) return FD_EINVAL;   // check_shape has left the message
  if (ws_bytes < lay.total) return fd_set_error(FD_ENOMEM, "fd_score_ode_enhance: workspace %zu < required %zu bytes", ws_bytes, lay.total);
  hipStream_t st = fd_stream(stream);
  float* Y = (float*)ws;
  float* X = (float*)((char*)ws + lay.state);
  float* normfac = (float*)((char*)ws + lay.normfac);
  char* rest = (char*)ws + lay.rest;
  const size_t rest_bytes = ws_bytes - lay.rest;
  const int n = per_clip ? B : 1;
  std::vector<int> nfe(n), rejected(n);
  int evals = 0;
  FD_TRY(fd_stft_forward(m->stft, y, lengths, B, L, m->cfg.alpha, m->cfg.beta, m->normalize, normfac, Y, lay.Tp, rest, rest_bytes, st));
  FD_TRY(score_ode_run(m, "fd_score_ode_enhance", Y, seeds ? fd_noise_src{nullptr, seeds, 0} : fd_noise_src{noise}, *cfg, rtol, atol, per_clip, X,
                       nfe.data(), rejected.data(), &evals, B, lay.Tp, rest, rest_bytes, st));
  FD_TRY(fd_stft_inverse(m->stft, X, lengths, B, lay.T, lay.Tp, m->cfg.alpha, m->cfg.beta, normfac, x_hat, L, rest, rest_bytes, st));
  FD_HIP(hipStreamSynchronize(st));
  for (int b = 0; b < n; ++b) { nfe_out[b] = nfe[b]; if (rejected_out) rejected_out[b] = rejected[b]; }
  if (evals_out) *evals_out = evals;
  return FD_OK;
}

static int regression_enhance_impl(fd_model* m, const char* who, const float* y, const int* lens, float* x_hat, int B, int L, void* ws, size_t ws_bytes,
                                   int use_graph, void* stream, const float* normfac_in = nullptr) {
  GraphKey key; key.kind = 4;
  return enhance_common(m, who, y, lens, x_hat, B, L, ws, ws_bytes, key, use_graph, stream,
                        [&](float* Y, float* X, int Tp, void* rest, size_t rest_bytes, hipStream_t st) {
                          OutSpec os; os.dst = X; os.coef = 1.f;                                 // X_hat = backbone(Y, Y, t = 0), model.py:566-578
                          return forward_call(m, Y, Y, nullptr, 0.f, 1, os, B, Tp, rest, rest_bytes, st);
                        }, normfac_in);
}

extern "C" int fd_regression_enhance(fd_model* m, const float* y, float* x_hat, int B, int L, void* ws, size_t ws_bytes, int use_graph,
                                     void* stream) {
  FD_MODEL_ENTER(m, "fd_regression_enhance");
  return regression_enhance_impl(m, "fd_regression_enhance", y, nullptr, x_hat, B, L, ws, ws_bytes, use_graph, stream);
}

// RegressionModel.enhance on a RAGGED batch: the contract of fd_enhance_ragged without a noise argument (y / x_hat [B][L] rows, lengths =
// device int32 [B] of one T_pad bucket, clip b bit-identical to the one-clip call, samples [lengths[b], L) of a row of x_hat zero).  A
// captured graph is keyed on the POINTER lengths.
extern "C" int fd_regression_enhance_ragged(fd_model* m, const float* y, const int* lengths, float* x_hat, int B, int L, void* ws, size_t ws_bytes,
                                            int use_graph, void* stream) {
  FD_MODEL_ENTER(m, "fd_regression_enhance_ragged");
  FD_REQUIRE(lengths, "fd_regression_enhance_ragged: null lengths");
  FD_REQUIRE(B > 0, "fd_regression_enhance_ragged: B must be positive (got %d)", B);
  return regression_enhance_impl(m, "fd_regression_enhance_ragged", y, lengths, x_hat, B, L, ws, ws_bytes, use_graph, stream);
}

// Long-form for the regression model: fd_regression_enhance_ragged plus normfac_in (device float [B], may be NULL) in place of the per-row
// maximum, as in fd_enhance_chunks (there is no noise, so no frame0).  NULL = fd_regression_enhance_ragged, bit for bit.  A captured graph is
// keyed on the POINTERS lengths and normfac_in.
extern "C" int fd_regression_enhance_chunks(fd_model* m, const float* y, const int* lengths, const float* normfac_in, float* x_hat, int B, int L,
                                            void* ws, size_t ws_bytes, int use_graph, void* stream) {
  FD_MODEL_ENTER(m, "fd_regression_enhance_chunks");
  FD_REQUIRE(lengths, "fd_regression_enhance_chunks: null lengths");
  FD_REQUIRE(B > 0, "fd_regression_enhance_chunks: B must be positive (got %d)", B);
  return regression_enhance_impl(m, "fd_regression_enhance_chunks", y, lengths, x_hat, B, L, ws, ws_bytes, use_graph, stream, normfac_in);
}

// ---- validation loss (include/flowdec_hip.h "Validation loss"; kernels: loss.hip) ---------------------------------------------------
// _loss of the three model classes without gradients: _preprocess(y, x = x) -> fd_loss_state -> ONE network evaluation at the per-clip
// times -> fd_loss_sqerr.  Workspace: Y | X | Xt | target | V (five states), t [B], std [B], the reduction's partials, then the larger
// of the transform's and the network's scratch.
namespace {
struct loss_layout { size_t state, vec, sq, rest, total; int T, Tp; };
bool loss_bytes(const fd_model* m, int B, int L, loss_layout& s) {
  if (!m || B <= 0 || B > fd_model::MAX_NT || L <= m->cfg.n_fft / 2 || L > 0x7fffffff - 1024) return false;
  s.T = 1 + L / m->cfg.hop; s.Tp = fd_padded_frames(s.T);
  if (check_shape(m, B, s.Tp) != FD_OK) return false;
  s.state = fd_align(sizeof(float) * 2 * (size_t)B * m->n_freq * s.Tp);
  s.vec = fd_align(sizeof(float) * B);
  s.sq = fd_loss_sqerr_workspace_bytes(B, m->n_freq, s.Tp);
  if (!s.sq) return false;
  const size_t a = fd_stft_ws_bytes(B, L, m->cfg.n_fft, m->cfg.hop), b = forward_ws_bytes(m, B, s.Tp);
  s.rest = a > b ? a : b;
  s.total = 5 * s.state + 2 * s.vec + s.sq + s.rest + 256;
  return true;
}
}  // namespace

extern "C" size_t fd_valid_loss_workspace_bytes(const fd_model* m, int B, int L) {
  loss_layout s;
  if (!m || !m->finalized || !loss_bytes(m, B, L, s)) return 0;
  return s.total;
}

extern "C" int fd_valid_loss(fd_model* m, const fd_loss_config* cfg, const float* x, const float* y, const int* lengths, const float* noise,
                             const unsigned long long* seeds, const float* t, double* sums_out, long long* bad_out, float* normfac_out, int B, int L,
                             void* ws, size_t ws_bytes, void* stream) {
  FD_MODEL_ENTER(m, "fd_valid_loss");
  FD_TRY(check_ready(m));
  FD_REQUIRE(cfg, "fd_valid_loss: null cfg");
  FD_REQUIRE(x, "fd_valid_loss: null x");
  FD_REQUIRE(y, "fd_valid_loss: null y");
  FD_REQUIRE(sums_out, "fd_valid_loss: null sums_out");
  FD_REQUIRE(bad_out, "fd_valid_loss: null bad_out");
  FD_REQUIRE(normfac_out, "fd_valid_loss: null normfac_out");
  FD_REQUIRE(ws, "fd_valid_loss: null ws");
  const int kind = cfg->kind;
  FD_REQUIRE(kind == FD_LOSS_FLOW || kind == FD_LOSS_SCORE || kind == FD_LOSS_REGRESSION, "fd_valid_loss: unknown kind %d", kind);
  FD_REQUIRE(B > 0 && B <= fd_model::MAX_NT, "fd_valid_loss: B = %d clips (1 <= B <= %d: one time per clip)", B, fd_model::MAX_NT);
  FD_REQUIRE(L > m->cfg.n_fft / 2 && L <= 0x7fffffff - 1024, "fd_valid_loss: clips must be longer than %d samples (L = %d)", m->cfg.n_fft / 2, L);
  float lo = 0.f;
  if (kind != FD_LOSS_REGRESSION) {
    FD_REQUIRE((noise != nullptr) != (seeds != nullptr), "fd_valid_loss: exactly one of noise and seeds must be given (got %s)", noise ? "both" : "neither");
    FD_REQUIRE(t || seeds, "fd_valid_loss: t is NULL and there are no seeds to draw it from");
  }
  if (kind == FD_LOSS_FLOW) FD_REQUIRE(cfg->sigma_x >= 0.f, "fd_valid_loss: sigma_x must not be negative");
  if (kind == FD_LOSS_SCORE) {
    FD_REQUIRE(cfg->sigma_min > 0.f && cfg->sigma_max > cfg->sigma_min && cfg->theta > 0.f, "fd_valid_loss: bad OUVE parameters");
    FD_REQUIRE(cfg->t_eps > 0.f && cfg->t_eps < 1.f, "fd_valid_loss: t_eps must be in (0, 1)");
    lo = cfg->t_eps;
  }
  loss_layout s;
  FD_REQUIRE(loss_bytes(m, B, L, s), "fd_valid_loss: bad shape B %d L %d for this model", B, L);
  FD_REQUIRE(ws_bytes >= s.total, "fd_valid_loss: workspace too small (%zu < %zu bytes, fd_valid_loss_workspace_bytes)", ws_bytes, s.total);
  hipStream_t st = fd_stream(stream);
  char* base = reinterpret_cast<char*>(((uintptr_t)ws + 255) / 256 * 256);
  float* Y = (float*)base;
  float* X = (float*)(base + s.state);
  float* Xt = (float*)(base + 2 * s.state);
  float* target = (float*)(base + 3 * s.state);
  float* V = (float*)(base + 4 * s.state);
  float* t_ws = (float*)(base + 5 * s.state);
  float* std_ws = (float*)(base + 5 * s.state + s.vec);
  char* sq = base + 5 * s.state + 2 * s.vec;
  char* rest = sq + s.sq;
  const int F = m->n_freq, Tp = s.Tp;
  // _preprocess(y, x = x): the factor comes from y alone; x is divided by the same one
  FD_TRY(fd_stft_forward(m->stft, y, lengths, B, L, m->cfg.alpha, m->cfg.beta, m->normalize, normfac_out, Y, Tp, rest, s.rest, st));
  FD_TRY(fd_stft_forward(m->stft, x, lengths, B, L, m->cfg.alpha, m->cfg.beta, m->normalize, nullptr, X, Tp, rest, s.rest, st, normfac_out));
  OutSpec os; os.dst = V; os.coef = 1.f;
  if (kind == FD_LOSS_REGRESSION) {
    FD_TRY(forward_call(m, Y, Y, nullptr, 0.f, 1, os, B, Tp, rest, s.rest, st));
    return fd_loss_sqerr(kind, V, X, nullptr, sums_out, bad_out, B, F, Tp, sq, s.sq, stream);
  }
  if (!t) {
    FD_TRY(fd_loss_times(seeds, B, lo, 1.0f, t_ws, stream));
    t = t_ws;
  }
  FD_TRY(fd_loss_state(cfg, Y, X, t, noise, seeds, m->sigma_dev, m->sigma_n, Xt, target, std_ws, nullptr, B, F, Tp, stream));
  FD_TRY(forward_call(m, Xt, Y, t, 0.f, B, os, B, Tp, rest, s.rest, st));
  return fd_loss_sqerr(kind, V, target, std_ws, sums_out, bad_out, B, F, Tp, sq, s.sq, stream);
}
