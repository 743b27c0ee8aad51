// solve.hip -- everything that integrates the network (model.hip: forward_call) over time, host side: the fixed-step ODE loop
// (model.py:503-515; torchdyn fixed-step semantics restated) behind fd_ode_solve with hipGraph capture, the ScoreDec
// predictor-corrector sampler and fd_score_eval, and the adaptive dopri5 / tsit5 solvers: ONE host loop over step_ctl.h's controllers,
// driven batch-globally (fd_ode_solve_adaptive*) or per clip (fd_ode_solve_adaptive_clips) -- and, on the ScoreDec probability-flow drift
// under scipy RK45's step-size rule, the ODE sampler of the score model (fd_score_ode_solve; waveform form: enhance.hip).
#include <math.h>
#include <string.h>

#include <utility>
#include <vector>

#include "model_internal.h"
#include "step_ctl.h"

using namespace fdm;

namespace fdm {

size_t ode_ws_bytes(const fd_model* m, int B, int T) {
  const size_t state = fd_align(sizeof(float) * 2 * (size_t)B * m->n_freq * T);
  return 2 * state + forward_ws_bytes(m, B, T);
}

// the solver loop; everything is enqueued on `st` (eagerly or inside a capture)
int ode_enqueue(fd_model* m, const float* Y, const fd_noise_src& noise, float sigma_fac, int N, int solver, float* X, float* traj, int B, int T, void* ws,
                size_t ws_bytes, hipStream_t st) {
  const size_t nstate = (size_t)B * m->n_freq * T;
  const size_t state = fd_align(sizeof(float) * 2 * nstate);
  float* xtmp = (float*)ws;
  float* k1 = (float*)((char*)ws + state);
  void* fws = (char*)ws + 2 * state;
  const size_t fws_bytes = ws_bytes - 2 * state;
  FD_TRY(fd_init_state(Y, noise, m->sigma_dev, m->sigma_n, sigma_fac, X, B, m->n_freq, T, st));
  if (traj) FD_HIP(hipMemcpyAsync(traj, X, sizeof(float) * 2 * nstate, hipMemcpyDeviceToDevice, st));
  const std::vector<float> ts = t_span_linspace(N);
  float t = ts[0];
  float dt = ts[1] - ts[0];
  for (int i = 1; i <= N; ++i) {
    OutSpec os;
    if (solver == FD_SOLVER_EULER) {
      os.base = X; os.coef = dt; os.dst = X;
      FD_TRY(forward_call(m, X, Y, nullptr, t, 1, os, B, T, fws, fws_bytes, st));
    } else if (solver == FD_SOLVER_MIDPOINT) {
      const float half = 0.5f * dt;
      os.base = X; os.coef = half; os.dst = xtmp;
      FD_TRY(forward_call(m, X, Y, nullptr, t, 1, os, B, T, fws, fws_bytes, st));
      OutSpec o2; o2.base = X; o2.coef = dt; o2.dst = X;
      FD_TRY(forward_call(m, xtmp, Y, nullptr, t + half, 1, o2, B, T, fws, fws_bytes, st));
    } else {  // heun2 / heun2_eulerlast (sampling/solvers.py:15-57)
      const bool last = solver == FD_SOLVER_HEUN2_EULERLAST && fabsf((t + dt) - 1.0f) <= 1e-8f + 1e-5f;
      if (last) {
        os.base = X; os.coef = dt; os.dst = X;
        FD_TRY(forward_call(m, X, Y, nullptr, t, 1, os, B, T, fws, fws_bytes, st));
      } else {
        os.base = X; os.coef = dt; os.dst = xtmp; os.ksave = k1;
        FD_TRY(forward_call(m, X, Y, nullptr, t, 1, os, B, T, fws, fws_bytes, st));
        OutSpec o2; o2.base = X; o2.kold = k1; o2.coef = dt * 0.5f; o2.dst = X;
        FD_TRY(forward_call(m, xtmp, Y, nullptr, t + dt, 1, o2, B, T, fws, fws_bytes, st));
      }
    }
    if (traj) FD_HIP(hipMemcpyAsync(traj + 2 * nstate * i, X, sizeof(float) * 2 * nstate, hipMemcpyDeviceToDevice, st));
    t = t + dt;
    if (i < N) dt = ts[i + 1] - t;
  }
  return FD_OK;
}

}  // namespace fdm

namespace {
// ---- ScoreDec baseline: OUVE closed forms + predictor-corrector sampler -------------------
// float32 scalar arithmetic like the reference's [B]-shaped tensors (sdes.py:168-192)
float ouve_std(const fd_score_config& c, float t) {
  const float th = c.theta, ls = logf(c.sigma_max / c.sigma_min);
  const float num = c.sigma_min * c.sigma_min * expf(-2.f * th * t) * (expf(2.f * (th + ls) * t) - 1.f) * ls;
  return sqrtf(num / (th + ls));
}
float ouve_diffusion(const fd_score_config& c, float t) {
  const float ls = logf(c.sigma_max / c.sigma_min);
  return c.sigma_min * powf(c.sigma_max / c.sigma_min, t) * sqrtf(2.f * ls);
}
// The epilogue coefficients of one fd_score_eval at time t, o = (cb, cy, cn):  out = cb x + cy Y + cn v
void score_coefs(const fd_score_config& c, float t, int mode, float* o) {
  const float std_t = ouve_std(c, t), g = ouve_diffusion(c, t);
  if (mode == FD_SCORE_DENOISE) {   // x_mean = x - (theta (y - x) dt - G^2 score), G = g sqrt(dt), score = -net / std
    const float dt = 1.f / (float)c.N, G = g * sqrtf(dt);
    o[0] = 1.f + c.theta * dt; o[1] = -c.theta * dt; o[2] = -(G * G) / std_t;
  } else {                          // drift = theta (y - x) - g^2 score * (0.5 | 1)
    o[0] = -c.theta; o[1] = c.theta; o[2] = (mode == FD_SCORE_DRIFT_PF ? 0.5f : 1.f) * g * g / std_t;
  }
}
int score_draws(const fd_score_config& c) {
  return 1 + c.N * ((c.corrector == FD_CORRECTOR_ALD ? c.corrector_steps : 0) + (c.predictor != FD_PREDICTOR_NONE ? 1 : 0));
}
}  // namespace

namespace fdm {

// sampling/__init__.py:57-70.  noise = [draws][B][F][T] complex64 (or the clips' seeds: draw indices 0, 1, ...), consumed in the reference's
// order of randn_like calls -- a draw whose coefficient is zero (the last predictor step under `denoise`) still takes its index.  Every draw
// carries the source's frame0 (fd_score_enhance_chunks): all fd_score_num_draws planes are the recording's, at the absolute frame.
int score_enqueue(fd_model* m, const float* Y, const fd_noise_src& noise, const fd_score_config& c, float* X, int B, int T, void* ws, size_t ws_bytes,
                  hipStream_t st) {
  const size_t nstate = (size_t)B * m->n_freq * T;
  fd_noise_src z = noise;
  auto next_z = [&]() { const fd_noise_src r = z; if (z.seeds) ++z.draw; else z.ptr += 2 * nstate; return r; };
  FD_TRY(fd_caxpy(Y, next_z(), ouve_std(c, 1.0f), X, B, m->n_freq, T, st));                 // prior, sdes.py:197-202
  const std::vector<float> ts = linspace_f32(1.0f, c.t_eps, c.N);
  for (int i = 0; i < c.N; ++i) {
    const float t = ts[i], std_t = ouve_std(c, t);
    if (c.corrector == FD_CORRECTOR_ALD) {                                                      // correctors.py:52-66
      for (int k = 0; k < c.corrector_steps; ++k) {
        const float step = (c.snr * std_t) * (c.snr * std_t) * 2.f;
        OutSpec os; os.score = true; os.base = X; os.dst = X; os.coef = -step / std_t; os.z = next_z(); os.cz = sqrtf(step * 2.f);
        FD_TRY(forward_call(m, X, Y, nullptr, t, 1, os, B, T, ws, ws_bytes, st));
      }
    }
    const bool last = i == c.N - 1 && c.denoise;                                                // result = x_mean of the last predictor step
    if (c.predictor == FD_PREDICTOR_REVERSE_DIFFUSION) {                                        // predictors.py:61-71, sdes.py:62-77,111-116
      const float dt = 1.f / (float)c.N, G = ouve_diffusion(c, t) * sqrtf(dt);
      OutSpec os; os.score = true; os.base = X; os.dst = X; os.yv = Y;
      os.cb = 1.f + c.theta * dt; os.cy = -c.theta * dt; os.coef = -(G * G) / std_t; os.z = next_z(); os.cz = last ? 0.f : G;
      FD_TRY(forward_call(m, X, Y, nullptr, t, 1, os, B, T, ws, ws_bytes, st));
    } else if (c.predictor == FD_PREDICTOR_EULER_MARUYAMA) {                                    // predictors.py:48-58, sdes.py:93-109
      const float dt = -1.f / (float)c.N, g = ouve_diffusion(c, t);
      OutSpec os; os.score = true; os.base = X; os.dst = X; os.yv = Y;
      os.cb = 1.f - c.theta * dt; os.cy = c.theta * dt; os.coef = g * g * dt / std_t; os.z = next_z(); os.cz = last ? 0.f : g * sqrtf(-dt);
      FD_TRY(forward_call(m, X, Y, nullptr, t, 1, os, B, T, ws, ws_bytes, st));
    }
  }
  return FD_OK;
}

}  // namespace fdm

namespace {
int ode_solve_impl(fd_model* m, const char* who, const float* Y, const fd_noise_src& noise, float sigma_fac, int N, int solver, float* X_out, float* traj,
                   int B, int T_pad, void* ws, size_t ws_bytes, int use_graph, void* stream) {
  FD_TRY(check_ready(m));
  FD_REQUIRE(Y && (noise.ptr || noise.seeds) && X_out && ws, "%s: null pointer", who);
  FD_REQUIRE(N >= 1, "%s: N must be >= 1", who);
  FD_REQUIRE(solver_nfe(solver, N) > 0, "%s: unknown solver id %d", who, solver);
  FD_TRY(check_shape(m, B, T_pad));
  const size_t need = ode_ws_bytes(m, B, T_pad);
  if (ws_bytes < need) return fd_set_error(FD_ENOMEM, "%s: workspace %zu < required %zu bytes", who, ws_bytes, need);
  hipStream_t st = fd_stream(stream);
  GraphKey key; key.Y = Y; key.noise = noise.ptr; key.seeds = noise.seeds; key.X = X_out; key.traj = traj; key.ws = ws; key.B = B; key.T = T_pad; key.N = N;
  key.solver = solver; key.kind = 1; key.sigma_fac = sigma_fac;
  return run_maybe_graph(m, key, use_graph != 0, st, [&]() { return ode_enqueue(m, Y, noise, sigma_fac, N, solver, X_out, traj, B, T_pad, ws, ws_bytes, st); });
}
}  // namespace

extern "C" int fd_ode_solve(fd_model* m, const float* Y, const float* noise, float sigma_fac, int N, int solver, float* X_out, float* traj, int B,
                            int T_pad, void* ws, size_t ws_bytes, int use_graph, void* stream) {
  FD_MODEL_ENTER(m, "fd_ode_solve");
  return ode_solve_impl(m, "fd_ode_solve", Y, fd_noise_src{noise}, sigma_fac, N, solver, X_out, traj, B, T_pad, ws, ws_bytes, use_graph, stream);
}

// fd_ode_solve with the initial noise generated from the clips' seeds (draw index 0) inside the kernel that forms x0
extern "C" int fd_ode_solve_seeded(fd_model* m, const float* Y, const unsigned long long* seeds, float sigma_fac, int N, int solver, float* X_out,
                                   float* traj, int B, int T_pad, void* ws, size_t ws_bytes, int use_graph, void* stream) {
  FD_MODEL_ENTER(m, "fd_ode_solve_seeded");
  return ode_solve_impl(m, "fd_ode_solve_seeded", Y, fd_noise_src{nullptr, seeds, 0}, sigma_fac, N, solver, X_out, traj, B, T_pad, ws, ws_bytes, use_graph,
                        stream);
}

// ---- adaptive dopri5 / tsit5 (tableaux and step-size controller: step_ctl.h; host-driven: one synchronisation per attempted step for
// the error ratio).  ONE loop, adaptive_solve, over nctl controllers: one for the whole batch (torchdyn's batched call), or one per clip
// -- clip b of the batch then takes the steps, and gives the bits, of the batch-global call on that clip alone; a clip that has reached
// t = 1 rides along with dt = 0 until the slowest clip is done.  What differs between the two modes is a policy (BatchPolicy,
// ClipPolicy): how the state is combined, where the network's time comes from, how the error norm is taken, what reaches the device
// before an attempt (publish) and how an accepted step is committed.
// The loop is also generic in the PROBLEM and in the step-size RULE: the flow model's field from t = 0 up to 1 under torchdyn's rule
// (FlowCtl around StepCtl), or the ScoreDec probability-flow drift from t = 1 down to eps under scipy RK45's (ScipyCtl around Rk45Ctl;
// fd_score_ode_solve).  The problem lives in AdaptiveCtx (the initial state and how one evaluation of the network becomes the right-hand
// side), the rule in the controller objects the entry point hands over. -------------------------------------------------------------
namespace {
constexpr int DP_NORM_BLOCKS = 512;

// per-clip control: the host table of one attempt, copied to the device in one piece.  Rows of B 32-bit words: dt, the six stage times
// (row 1 doubles as the time of the two initial evaluations), and the commit of the PREVIOUS attempt (accept flag, checkpoint index);
// the score problem appends the epilogue coefficients of the six evaluations ahead, [6][B][3] floats (cb, cy, cn at the clip's time)
enum { TAB_DT = 0, TAB_T1 = 1, TAB_ACCEPT = 7, TAB_CKPT = 8, TAB_ROWS = 9, TAB_COEF = 9, TAB_ROWS_SCORE = TAB_ROWS + 6 * 3 };
size_t clips_tab_bytes(int B, int rows = TAB_ROWS) { return fd_align(sizeof(float) * rows * (size_t)B); }
size_t clips_partial_bytes(int B) { return fd_align(sizeof(double) * DP_NORM_BLOCKS * (size_t)B); }
// the pinned host mirror (fd_model::pin_clips): the largest table, then the partials
size_t pin_partial_offset() { return clips_tab_bytes(fd_model::MAX_NT, TAB_ROWS_SCORE); }
int pin_clips_ready(fd_model* m) {
  if (!m->pin_clips) FD_HIP(hipHostMalloc(&m->pin_clips, pin_partial_offset() + clips_partial_bytes(fd_model::MAX_NT), hipHostMallocDefault));
  return FD_OK;
}

// The workspace of both modes (offsets): x | x_new | err | k[7] (ten states), the norm's partials, the per-clip table, forward scratch
struct adaptive_layout_t { size_t state, partial, tab, fws, total; };
adaptive_layout_t adaptive_layout(const fd_model* m, int B, int T, bool per_clip, bool score = false) {
  adaptive_layout_t s;
  s.state = fd_align(sizeof(float) * 2 * (size_t)B * m->n_freq * T);
  s.partial = 10 * s.state;
  s.tab = s.partial + clips_partial_bytes(per_clip ? B : 1);
  s.fws = s.tab + (per_clip ? clips_tab_bytes(B, score ? TAB_ROWS_SCORE : TAB_ROWS) : 0);
  s.total = s.fws + forward_ws_bytes(m, B, T);
  return s;
}

// What the two policies share: the problem and the carved workspace.  sc == nullptr: the flow model (x0 = Y + sigma_fac sigma_y z, the
// right-hand side is the network's output); sc given: the ScoreDec probability-flow ODE (x_T = Y + std(1) z, the right-hand side is the
// FD_SCORE_DRIFT_PF epilogue of fd_score_eval at the evaluation's time)
struct AdaptiveCtx {
  fd_model* m; const float* Y; float* traj; int B, T; float atol, rtol; hipStream_t st;
  size_t nclip, nstate;   // complex elements of one clip, of the batch
  float *x, *x_new, *err, *k[7]; double* partial; float* tab_dev; void* fws; size_t fws_bytes;
  const fd_score_config* sc = nullptr;
  float sigma_fac = 1.f;
  const char* who = "";
  AdaptiveCtx(fd_model* m_, const float* Y_, float* traj_, int B_, int T_, float atol_, float rtol_, hipStream_t st_, void* ws, size_t ws_bytes,
              const adaptive_layout_t& lay)
      : m(m_), Y(Y_), traj(traj_), B(B_), T(T_), atol(atol_), rtol(rtol_), st(st_), nclip((size_t)m_->n_freq * T_), nstate((size_t)B_ * nclip) {
    char* base = (char*)ws;
    x = (float*)base; x_new = (float*)(base + lay.state); err = (float*)(base + 2 * lay.state);
    for (int i = 0; i < 7; ++i) k[i] = (float*)(base + (3 + i) * lay.state);
    partial = (double*)(base + lay.partial); tab_dev = (float*)(base + lay.tab);
    fws = base + lay.fws; fws_bytes = ws_bytes - lay.fws;
  }
  int tab_rows() const { return sc ? TAB_ROWS_SCORE : TAB_ROWS; }
  int init_state(const fd_noise_src& noise) const {
    if (sc) return fd_caxpy(Y, noise, ouve_std(*sc, 1.0f), x, B, m->n_freq, T, st);   // prior sample, sdes.py:197-202
    return fd_init_state(Y, noise, m->sigma_dev, m->sigma_n, sigma_fac, x, B, m->n_freq, T, st);
  }
  // one right-hand side: the clips' times from the device (t, nt = B; the score problem's coefficients then from ctab, [B][3]) or t_imm
  int forward(const float* xin, const float* t, float t_imm, int nt, const float* ctab, float* kout) const {
    OutSpec os; os.dst = kout; os.coef = 1.f;
    if (sc) {
      os.score = true; os.base = xin; os.yv = Y;
      if (t) os.ctab = ctab;
      else { float co[3]; score_coefs(*sc, t_imm, FD_SCORE_DRIFT_PF, co); os.cb = co[0]; os.cy = co[1]; os.coef = co[2]; }
    }
    return forward_call(m, xin, Y, t, t_imm, nt, os, B, T, fws, fws_bytes, st);
  }
};

// One controller for the whole batch: the step and the stage time are host scalars, handed over with each launch.
struct BatchPolicy : AdaptiveCtx {
  using AdaptiveCtx::AdaptiveCtx;
  std::vector<double> host_partial = std::vector<double>(DP_NORM_BLOCKS);
  int publish(const float*, const float*, const int*, const int*, bool) { return FD_OK; }
  int combine(float cx, const float* dt, const float* const* kk, const float* cc, int nk, float* dst) {
    return fd_ode_lincomb(x, cx, dt[0], kk, cc, nk, dst, (long long)nstate, st);
  }
  int eval(const float* xin, int, const float* t, float* kout) { return forward(xin, nullptr, t[0], 1, nullptr, kout); }
  // Hairer norm of (p - q) / (atol + rtol max(|r|, |s|)): sqrt(mean |.|^2) over the complex elements
  int norm(const float* p_, const float* q_, const float* r_, const float* s_, double* out) {
    FD_TRY(fd_ode_scaled_sq(p_, q_, r_, s_, atol, rtol, partial, DP_NORM_BLOCKS, (long long)nstate, st));
    FD_HIP(hipMemcpyAsync(host_partial.data(), partial, sizeof(double) * DP_NORM_BLOCKS, hipMemcpyDeviceToHost, st));
    FD_HIP(hipStreamSynchronize(st));
    double acc = 0.0;
    for (double v : host_partial) acc += v;
    out[0] = sqrt(acc / (double)nstate);
    return FD_OK;
  }
  int commit(const int* accept, const int* landed) {
    if (!accept[0]) return FD_OK;
    std::swap(x, x_new);
    std::swap(k[0], k[6]);
    if (landed[0] && traj) FD_HIP(hipMemcpyAsync(traj + 2 * nstate * landed[0], x, sizeof(float) * 2 * nstate, hipMemcpyDeviceToDevice, st));
    return FD_OK;
  }
  int step_limit(int, double dt, double t) const { return fd_set_error(FD_ERUNTIME, "%s: step limit reached (dt = %g at t = %g)", who, dt, t); }
  int too_small(int, double dt, double t) const { return fd_set_error(FD_ERUNTIME, "%s: step size too small (dt = %g at t = %g)", who, dt, t); }
};

// One controller per clip: the device side reads the clips' step sizes, stage times and commit flags from the table (TAB_*).
struct ClipPolicy : AdaptiveCtx {
  using AdaptiveCtx::AdaptiveCtx;
  // pinned host mirrors (m->pin_clips: table | partials): free to rewrite after every synchronisation (each copy from / to them is
  // followed by one before the next write).  The table is [TAB_ROWS][B] words: floats by bit pattern, flags as integers -- the loop's
  // dt | tq | accept | landed in that order; its commit rows are those of the PREVIOUS attempt, which is committed here, deferred.
  int publish(const float* dt, const float* tq, const int* accept, const int* landed, bool pending) {
    uint32_t* tab = (uint32_t*)m->pin_clips;
    memcpy(tab + (size_t)TAB_DT * B, dt, sizeof(float) * B);
    memcpy(tab + (size_t)TAB_T1 * B, tq, sizeof(float) * 6 * B);
    memcpy(tab + (size_t)TAB_ACCEPT * B, accept, sizeof(int) * B);
    memcpy(tab + (size_t)TAB_CKPT * B, landed, sizeof(int) * B);
    if (sc) {   // the coefficients fd_score_eval would derive from each clip's time, for the six evaluations ahead
      float* co = (float*)(tab + (size_t)TAB_COEF * B);
      for (size_t i = 0; i < 6 * (size_t)B; ++i) score_coefs(*sc, tq[i], FD_SCORE_DRIFT_PF, co + 3 * i);
    }
    FD_HIP(hipMemcpyAsync(tab_dev, tab, sizeof(float) * tab_rows() * (size_t)B, hipMemcpyHostToDevice, st));
    const int* accept_dev = (const int*)tab_dev + (size_t)TAB_ACCEPT * B;
    const int* ckpt_dev = (const int*)tab_dev + (size_t)TAB_CKPT * B;
    if (pending) FD_TRY(fd_ode_commit_clips(accept_dev, ckpt_dev, x_new, k[6], x, k[0], traj, B, (long long)nclip, st));
    return FD_OK;
  }
  int combine(float cx, const float*, const float* const* kk, const float* cc, int nk, float* dst) {
    return fd_ode_lincomb_clips(x, cx, tab_dev + (size_t)TAB_DT * B, kk, cc, nk, dst, B, (long long)nclip, st);
  }
  int eval(const float* xin, int slot, const float*, float* kout) {   // clip b at time tab[TAB_T1 + slot][b]
    return forward(xin, tab_dev + (size_t)(TAB_T1 + slot) * B, 0.f, B, tab_dev + (size_t)(TAB_COEF + 3 * slot) * B, kout);
  }
  // the Hairer norm of the one-clip call, clip by clip: the clip's DP_NORM_BLOCKS partials summed in index order
  int norm(const float* p_, const float* q_, const float* r_, const float* s_, double* out) {
    const double* host_partial = (const double*)((char*)m->pin_clips + pin_partial_offset());
    FD_TRY(fd_ode_scaled_sq_clips(p_, q_, r_, s_, atol, rtol, partial, DP_NORM_BLOCKS, B, (long long)nclip, st));
    FD_HIP(hipMemcpyAsync((void*)host_partial, partial, sizeof(double) * DP_NORM_BLOCKS * (size_t)B, hipMemcpyDeviceToHost, st));
    FD_HIP(hipStreamSynchronize(st));
    for (int b = 0; b < B; ++b) {
      double acc = 0.0;
      for (int j = 0; j < DP_NORM_BLOCKS; ++j) acc += host_partial[(size_t)b * DP_NORM_BLOCKS + j];
      out[b] = sqrt(acc / (double)nclip);
    }
    return FD_OK;
  }
  int commit(const int*, const int*) { return FD_OK; }   // deferred: the next publish carries the flags and runs fd_ode_commit_clips
  int step_limit(int b, double dt, double t) const {
    return fd_set_error(FD_ERUNTIME, "%s: step limit reached (clip %d: dt = %g at t = %g)", who, b, dt, t);
  }
  int too_small(int b, double dt, double t) const {
    return fd_set_error(FD_ERUNTIME, "%s: step size too small (clip %d: dt = %g at t = %g)", who, b, dt, t);
  }
};

// The two step-size rules behind the one face adaptive_solve drives; times and steps leave as the floats the device is given.
struct FlowCtl {    // torchdyn's (StepCtl) over the checkpoints ts[0..N], forwards
  const std::vector<float>* ts; int N; StepCtl c;
  FlowCtl(const std::vector<float>* ts_, int N_) : ts(ts_), N(N_) { c.t = (*ts_)[0]; }
  float time() const { return c.t; }
  double probe_step(double d0, double d1) const { return StepCtl::probe_step(d0, d1); }
  float probe_dt(double h0) const { return (float)h0; }
  float probe_time(double h0) const { return c.probe_time(h0); }
  void first_step(double h0, double d1, double d2) { c.first_step(h0, d1, d2); }   // d2: not yet divided by h0
  bool active() const { return c.active(*ts, N); }
  bool begin() { c.begin(*ts, N); return true; }
  float dt() const { return c.dt; }
  float stage_time(double cc) const { return c.stage_time(cc); }
  bool end(double ratio, int* landed) { return c.end(ratio, *ts, N, landed); }
};
struct ScipyCtl {   // scipy RK45's (Rk45Ctl) from t0 down to t_bound: double inside, the network and the kernels get (float)t and (float)h
  Rk45Ctl c;
  ScipyCtl(double t0, double t_bound) { c.start(t0, t_bound); }
  float time() const { return (float)c.t; }
  double probe_step(double d0, double d1) const { return c.probe_step(d0, d1); }
  float probe_dt(double h0) const { return (float)(h0 * Rk45Ctl::direction); }
  float probe_time(double h0) const { return (float)c.probe_time(h0); }
  void first_step(double h0, double d1, double d2) { c.first_step(h0, d1, d2 / h0); }
  bool active() const { return c.active(); }
  bool begin() { return c.begin(); }
  float dt() const { return (float)c.h; }
  float stage_time(double cc) const { return (float)c.stage_time(cc); }
  bool end(double err, int* landed) { *landed = 0; return c.end(err); }
};

// The solve: x0, the initial-step probe, then attempts until every controller has reached the end of the span.  nfe / rejected: per
// controller (2 + 6 per attempt it was active in); *evals: network evaluations enqueued.  Ends synchronised, the result in X_out.
template <typename Policy, typename Ctl>
int adaptive_solve(Policy& p, std::vector<Ctl>& c, const Tableau& tb, const fd_noise_src& noise, float* X_out, int* nfe, int* rejected, int* evals) {
  const int nctl = (int)c.size();
  const size_t state_bytes = sizeof(float) * 2 * p.nstate;
  FD_TRY(p.init_state(noise));
  if (p.traj) FD_HIP(hipMemcpyAsync(p.traj, p.x, state_bytes, hipMemcpyDeviceToDevice, p.st));
  std::vector<double> d0(nctl), d1(nctl), d2(nctl), h0(nctl), ratio(nctl);
  std::vector<float> dt(nctl, 0.f), tq(6 * (size_t)nctl, 0.f);   // per controller: the step, and the times of the (up to) six evaluations ahead
  std::vector<int> accept(nctl, 0), landed(nctl, 0);
  std::vector<char> act(nctl, 0);
  *evals = 0;
  auto eval = [&](const float* xin, int slot, float* kout) { ++*evals; return p.eval(xin, slot, &tq[(size_t)slot * nctl], kout); };
  auto publish = [&](bool pending) { return p.publish(dt.data(), tq.data(), accept.data(), landed.data(), pending); };
  for (int b = 0; b < nctl; ++b) tq[b] = c[b].time();
  FD_TRY(publish(false));
  FD_TRY(eval(p.x, 0, p.k[0]));
  FD_TRY(p.norm(p.x, nullptr, p.x, p.x, d0.data()));
  FD_TRY(p.norm(p.k[0], nullptr, p.x, p.x, d1.data()));
  for (int b = 0; b < nctl; ++b) {
    h0[b] = c[b].probe_step(d0[b], d1[b]);
    dt[b] = c[b].probe_dt(h0[b]);
    tq[b] = c[b].probe_time(h0[b]);
  }
  FD_TRY(publish(false));
  {
    const float* kk[1] = {p.k[0]}; const float cc[1] = {1.f};
    FD_TRY(p.combine(1.f, dt.data(), kk, cc, 1, p.x_new));
    FD_TRY(eval(p.x_new, 0, p.k[1]));
    FD_TRY(p.norm(p.k[1], p.k[0], p.x, p.x, d2.data()));
  }
  for (int b = 0; b < nctl; ++b) { c[b].first_step(h0[b], d1[b], d2[b]); nfe[b] = 2; rejected[b] = 0; }
  int steps = 0;
  bool pending = false;   // the previous attempt's accepted steps still wait for a deferred commit
  for (;;) {
    bool any = false;
    for (int b = 0; b < nctl; ++b) {
      act[b] = c[b].active();
      any = any || act[b];
      if (act[b] && !c[b].begin()) return p.too_small(b, (double)c[b].dt(), (double)c[b].time());
      dt[b] = act[b] ? c[b].dt() : 0.f;                              // a finished clip: dt = 0, evaluated at its final time, never committed
      for (int s = 1; s < 7; ++s) tq[(size_t)(s - 1) * nctl + b] = act[b] ? c[b].stage_time(tb.C[s]) : c[b].time();
    }
    if (!any && !pending) break;
    FD_TRY(publish(pending));
    if (!any) break;
    if (++steps > ADAPTIVE_MAX_ATTEMPTS) {
      int b = 0;
      while (!act[b]) ++b;
      return p.step_limit(b, (double)c[b].dt(), (double)c[b].time());
    }
    for (int s = 1; s < 7; ++s) {                                    // stages 2..7; stage 7 is evaluated at the 5th-order solution (FSAL)
      const float* kk[6]; float cc[6];
      for (int j = 0; j < s; ++j) { kk[j] = p.k[j]; cc[j] = (float)tb.A[s][j]; }
      float* xs = s == 6 ? p.x_new : p.err;                          // `err` doubles as the stage input buffer
      FD_TRY(p.combine(1.f, dt.data(), kk, cc, s, xs));
      FD_TRY(eval(xs, s - 1, p.k[s]));
    }
    {
      const float* kk[7]; float cc[7];
      for (int j = 0; j < 7; ++j) { kk[j] = p.k[j]; cc[j] = (float)tb.E[j]; }
      FD_TRY(p.combine(0.f, dt.data(), kk, cc, 7, p.err));
    }
    FD_TRY(p.norm(p.err, nullptr, p.x, p.x_new, ratio.data()));
    pending = false;
    for (int b = 0; b < nctl; ++b) {
      accept[b] = landed[b] = 0;
      if (!act[b]) continue;                                        // finished before this attempt
      nfe[b] += 6;
      accept[b] = c[b].end(ratio[b], &landed[b]) ? 1 : 0;
      if (accept[b]) pending = true; else ++rejected[b];
    }
    FD_TRY(p.commit(accept.data(), landed.data()));
  }
  FD_HIP(hipMemcpyAsync(X_out, p.x, state_bytes, hipMemcpyDeviceToDevice, p.st));
  FD_HIP(hipStreamSynchronize(p.st));
  return FD_OK;
}
}  // namespace

extern "C" size_t fd_ode_adaptive_workspace_bytes(const fd_model* m, int B, int T_pad) {
  if (!m || check_shape(m, B, T_pad) != FD_OK) return 0;
  return adaptive_layout(m, B, T_pad, false).total;
}

extern "C" int fd_ode_solve_adaptive_method(fd_model* m, const float* Y, const float* noise, float sigma_fac, int N, int method, float atol, float rtol,
                                            float* X_out, float* traj, int* nfe_out, int B, int T_pad, void* ws, size_t ws_bytes, void* stream) {
  FD_MODEL_ENTER(m, "fd_ode_solve_adaptive");
  FD_REQUIRE(method == FD_ADAPTIVE_DOPRI5 || method == FD_ADAPTIVE_TSIT5, "fd_ode_solve_adaptive: unknown method id %d", method);
  FD_TRY(check_ready(m));
  FD_REQUIRE(Y && noise && X_out && ws, "fd_ode_solve_adaptive: null pointer");
  FD_REQUIRE(N >= 1 && atol > 0.f && rtol >= 0.f, "fd_ode_solve_adaptive: need N >= 1, atol > 0, rtol >= 0");
  FD_TRY(check_shape(m, B, T_pad));
  const adaptive_layout_t lay = adaptive_layout(m, B, T_pad, false);
  if (ws_bytes < lay.total) return fd_set_error(FD_ENOMEM, "fd_ode_solve_adaptive: workspace %zu < required %zu bytes", ws_bytes, lay.total);
  BatchPolicy p(m, Y, traj, B, T_pad, atol, rtol, fd_stream(stream), ws, ws_bytes, lay);
  p.sigma_fac = sigma_fac; p.who = "fd_ode_solve_adaptive";
  const std::vector<float> ts = t_span_linspace(N);
  std::vector<FlowCtl> ctl(1, FlowCtl(&ts, N));
  int nfe = 0, rejected = 0, evals = 0;
  FD_TRY(adaptive_solve(p, ctl, adaptive_tableau(method), fd_noise_src{noise}, X_out, &nfe, &rejected, &evals));
  if (nfe_out) *nfe_out = nfe;
  return FD_OK;
}

extern "C" int fd_ode_solve_adaptive(fd_model* m, const float* Y, const float* noise, float sigma_fac, int N, float atol, float rtol, float* X_out,
                                     float* traj, int* nfe_out, int B, int T_pad, void* ws, size_t ws_bytes, void* stream) {
  return fd_ode_solve_adaptive_method(m, Y, noise, sigma_fac, N, FD_ADAPTIVE_DOPRI5, atol, rtol, X_out, traj, nfe_out, B, T_pad, ws, ws_bytes, stream);
}

extern "C" size_t fd_ode_adaptive_clips_workspace_bytes(const fd_model* m, int B, int T_pad) {
  if (!m || B > fd_model::MAX_NT || check_shape(m, B, T_pad) != FD_OK) return 0;
  return adaptive_layout(m, B, T_pad, true).total;
}

extern "C" int fd_ode_solve_adaptive_clips(fd_model* m, const float* Y, const float* noise, const unsigned long long* seeds, float sigma_fac, int N,
                                           int method, float atol, float rtol, float* X_out, float* traj, int* nfe_out, int* rejected_out,
                                           int* evals_out, int B, int T_pad, void* ws, size_t ws_bytes, void* stream) {
  FD_MODEL_ENTER(m, "fd_ode_solve_adaptive_clips");
  FD_REQUIRE(method == FD_ADAPTIVE_DOPRI5 || method == FD_ADAPTIVE_TSIT5, "fd_ode_solve_adaptive_clips: unknown method id %d", method);
  FD_TRY(check_ready(m));
  FD_REQUIRE(Y && X_out && ws && nfe_out, "fd_ode_solve_adaptive_clips: null pointer");
  FD_REQUIRE((noise != nullptr) != (seeds != nullptr), "fd_ode_solve_adaptive_clips: give exactly one of noise and seeds");
  FD_REQUIRE(N >= 1 && atol > 0.f && rtol >= 0.f, "fd_ode_solve_adaptive_clips: need N >= 1, atol > 0, rtol >= 0");
  FD_REQUIRE(B <= fd_model::MAX_NT, "fd_ode_solve_adaptive_clips: at most %d clips per call (got %d)", fd_model::MAX_NT, B);
  FD_TRY(check_shape(m, B, T_pad));
  const adaptive_layout_t lay = adaptive_layout(m, B, T_pad, true);
  if (ws_bytes < lay.total) return fd_set_error(FD_ENOMEM, "fd_ode_solve_adaptive_clips: workspace %zu < required %zu bytes", ws_bytes, lay.total);
  FD_TRY(pin_clips_ready(m));
  ClipPolicy p(m, Y, traj, B, T_pad, atol, rtol, fd_stream(stream), ws, ws_bytes, lay);
  p.sigma_fac = sigma_fac; p.who = "fd_ode_solve_adaptive_clips";
  const std::vector<float> ts = t_span_linspace(N);
  std::vector<FlowCtl> ctl(B, FlowCtl(&ts, N));
  std::vector<int> nfe(B), rejected(B);
  int evals = 0;
  FD_TRY(adaptive_solve(p, ctl, adaptive_tableau(method), seeds ? fd_noise_src{nullptr, seeds, 0} : fd_noise_src{noise}, X_out, nfe.data(), rejected.data(),
                        &evals));
  for (int b = 0; b < B; ++b) { nfe_out[b] = nfe[b]; if (rejected_out) rejected_out[b] = rejected[b]; }
  if (evals_out) *evals_out = evals;
  return FD_OK;
}

// ---- the ScoreDec ODE sampler (sampling/__init__.py:75-146: scipy.integrate.solve_ivp, method RK45, over (sde.T = 1, eps)) on the
// device: adaptive_solve on the probability-flow drift under scipy's step-size rule (Rk45Ctl, step_ctl.h).  step_control =
// FD_STEP_CONTROL_BATCH: one controller on the norms of the flattened batch, which is what solve_ivp sees and the reference's meaning
// of a batch; FD_STEP_CONTROL_CLIP: one per clip -- clip b takes the steps, and gives the bits, of the one-clip call.  The state planes
// are float32 (scipy carries complex128).  Where scipy's solver gives up on a step below ten spacings of t and the reference goes on
// with the last state, this returns FD_ERUNTIME ("step size too small"). ----------------------------------------------------------------
namespace fdm {

int score_ode_check(const char* who, const fd_score_config* c, float rtol, float atol, int step_control, int B) {
  FD_REQUIRE(c, "%s: null pointer (cfg)", who);
  FD_REQUIRE(c->sigma_min > 0.f && c->sigma_max > c->sigma_min && c->theta > 0.f, "%s: bad OUVE parameters", who);
  FD_REQUIRE(c->t_eps > 0.f && c->t_eps < 1.f, "%s: t_eps must be in (0, 1)", who);
  FD_REQUIRE(!c->denoise || c->N >= 1, "%s: the denoising step needs N >= 1", who);
  FD_REQUIRE(atol > 0.f && rtol >= 0.f, "%s: need atol > 0, rtol >= 0", who);
  FD_REQUIRE(step_control == FD_STEP_CONTROL_BATCH || step_control == FD_STEP_CONTROL_CLIP, "%s: unknown step_control %d", who, step_control);
  FD_REQUIRE(step_control != FD_STEP_CONTROL_CLIP || B <= fd_model::MAX_NT, "%s: at most %d clips per call with per-clip step control (got %d)", who,
             fd_model::MAX_NT, B);
  return FD_OK;
}

size_t score_ode_ws_bytes(const fd_model* m, int B, int T, bool per_clip) { return adaptive_layout(m, B, T, per_clip, true).total; }

// The solve on features: arguments checked by the caller (score_ode_check, check_shape, the workspace).  nfe / rejected: one entry
// (batch) or B (per clip).  Ends synchronised.
int score_ode_run(fd_model* m, const char* who, const float* Y, const fd_noise_src& noise, const fd_score_config& c, float rtol, float atol, bool per_clip,
                  float* X, int* nfe, int* rejected, int* evals, int B, int T, void* ws, size_t ws_bytes, hipStream_t st) {
  const adaptive_layout_t lay = adaptive_layout(m, B, T, per_clip, true);
  const Tableau tb{DP_C, DP_A, DP_E};
  std::vector<ScipyCtl> ctl(per_clip ? B : 1, ScipyCtl(1.0, (double)c.t_eps));
  void* fws = nullptr; size_t fws_bytes = 0;
  if (per_clip) {
    FD_TRY(pin_clips_ready(m));
    ClipPolicy p(m, Y, nullptr, B, T, atol, rtol, st, ws, ws_bytes, lay);
    p.sc = &c; p.who = who;
    FD_TRY(adaptive_solve(p, ctl, tb, noise, X, nfe, rejected, evals));
    fws = p.fws; fws_bytes = p.fws_bytes;
  } else {
    BatchPolicy p(m, Y, nullptr, B, T, atol, rtol, st, ws, ws_bytes, lay);
    p.sc = &c; p.who = who;
    FD_TRY(adaptive_solve(p, ctl, tb, noise, X, nfe, rejected, evals));
    fws = p.fws; fws_bytes = p.fws_bytes;
  }
  if (c.denoise) {   // one noise-free reverse-diffusion step at t = eps with dt = 1 / N (not counted in the NFE, as in the reference)
    float co[3];
    score_coefs(c, c.t_eps, FD_SCORE_DENOISE, co);
    OutSpec os; os.score = true; os.base = X; os.yv = Y; os.dst = X; os.cb = co[0]; os.cy = co[1]; os.coef = co[2];
    FD_TRY(forward_call(m, X, Y, nullptr, c.t_eps, 1, os, B, T, fws, fws_bytes, st));
    FD_HIP(hipStreamSynchronize(st));
  }
  return FD_OK;
}

}  // namespace fdm

extern "C" size_t fd_score_ode_workspace_bytes(const fd_model* m, int B, int T_pad, int step_control) {
  if (!m || (step_control != FD_STEP_CONTROL_BATCH && step_control != FD_STEP_CONTROL_CLIP)) return 0;
  if ((step_control == FD_STEP_CONTROL_CLIP && B > fd_model::MAX_NT) || check_shape(m, B, T_pad) != FD_OK) return 0;
  return score_ode_ws_bytes(m, B, T_pad, step_control == FD_STEP_CONTROL_CLIP);
}

extern "C" int fd_score_ode_solve(fd_model* m, const float* Y, const float* noise, const unsigned long long* seeds, const fd_score_config* cfg, float rtol,
                                  float atol, int step_control, float* X_out, int* nfe_out, int* rejected_out, int* evals_out, int B, int T_pad,
                                  void* ws, size_t ws_bytes, void* stream) {
  FD_MODEL_ENTER(m, "fd_score_ode_solve");
  FD_TRY(check_ready(m));
  FD_REQUIRE(Y && X_out && ws && nfe_out, "fd_score_ode_solve: null pointer");
  FD_REQUIRE((noise != nullptr) != (seeds != nullptr), "fd_score_ode_solve: give exactly one of noise and seeds");
  FD_TRY(score_ode_check("fd_score_ode_solve", cfg, rtol, atol, step_control, B));
  FD_TRY(check_shape(m, B, T_pad));
  const bool per_clip = step_control == FD_STEP_CONTROL_CLIP;
  const size_t need = score_ode_ws_bytes(m, B, T_pad, per_clip);
  if (ws_bytes < need) return fd_set_error(FD_ENOMEM, "fd_score_ode_solve: workspace %zu < required %zu bytes", ws_bytes, need);
  const int n = per_clip ? B : 1;
  std::vector<int> nfe(n), rejected(n);
  int evals = 0;
  FD_TRY(score_ode_run(m, "fd_score_ode_solve", Y, seeds ? fd_noise_src{nullptr, seeds, 0} : fd_noise_src{noise}, *cfg, rtol, atol, per_clip, X_out,
                       nfe.data(), rejected.data(), &evals, B, T_pad, ws, ws_bytes, fd_stream(stream)));
  for (int b = 0; b < n; ++b) { nfe_out[b] = nfe[b]; if (rejected_out) rejected_out[b] = rejected[b]; }
  if (evals_out) *evals_out = evals;
  return FD_OK;
}

extern "C" int fd_score_num_draws(const fd_score_config* c) {
  if (!c || c->N < 1 || c->corrector_steps < 0) return -1;
  return score_draws(*c);
}

// One evaluation of the score network combined into what the black-box ODE sampler of the reference needs
// (sampling/__init__.py:75-146): the probability-flow drift rsde.sde(x, t, y)[0] (sdes.py:93-109) or the noise-free
// reverse-diffusion predictor step used for the final denoising (predictors.py:61-71 with t = eps).
extern "C" int fd_score_eval(fd_model* m, const float* x, const float* Y, float t, const fd_score_config* c, int mode, float* out, int B,
                             int T_pad, void* ws, size_t ws_bytes, void* stream) {
  FD_MODEL_ENTER(m, "fd_score_eval");
  FD_TRY(check_ready(m));
  FD_REQUIRE(x && Y && c && out && ws, "fd_score_eval: null pointer");
  FD_REQUIRE(mode >= FD_SCORE_DRIFT_PF && mode <= FD_SCORE_DENOISE, "fd_score_eval: unknown mode %d", mode);
  FD_REQUIRE(c->sigma_min > 0.f && c->sigma_max > c->sigma_min && c->theta > 0.f, "fd_score_eval: bad OUVE parameters");
  FD_REQUIRE(mode != FD_SCORE_DENOISE || c->N >= 1, "fd_score_eval: the denoising step needs N >= 1");
  FD_TRY(check_shape(m, B, T_pad));
  const size_t need = forward_ws_bytes(m, B, T_pad);
  if (ws_bytes < need) return fd_set_error(FD_ENOMEM, "fd_score_eval: workspace %zu < required %zu bytes", ws_bytes, need);
  float co[3];
  score_coefs(*c, t, mode, co);
  OutSpec os; os.score = true; os.base = x; os.yv = Y; os.dst = out; os.cb = co[0]; os.cy = co[1]; os.coef = co[2];
  return forward_call(m, x, Y, nullptr, t, 1, os, B, T_pad, ws, ws_bytes, fd_stream(stream));
}
