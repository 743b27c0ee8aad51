// solve.hip -- everything that integrates the network (model.hip: forward_call) over time, host side: the fixed-step ODE loop
// (model.py:503-515; torchdyn fixed-step semantics restated) behind fd_ode_solve with hipGraph capture, the ScoreDec
// predictor-corrector sampler and fd_score_eval, and the adaptive dopri5 / tsit5 solvers: ONE host loop over step_ctl.h's controllers,
// driven batch-globally (fd_ode_solve_adaptive*) or per clip (fd_ode_solve_adaptive_clips).
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
int score_draws(const fd_score_config& c) {
  return 1 + c.N * ((c.corrector == FD_CORRECTOR_ALD ? c.corrector_steps : 0) + (c.predictor != FD_PREDICTOR_NONE ? 1 : 0));
}
}  // namespace

namespace fdm {

// sampling/__init__.py:57-70.  noise = [draws][B][F][T] complex64 (or the clips' seeds: draw indices 0, 1, ...), consumed in the reference's
// order of randn_like calls -- a draw whose coefficient is zero (the last predictor step under `denoise`) still takes its index.
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
// before an attempt (publish) and how an accepted step is committed. ---------------------------------------------------------------
namespace {
constexpr int DP_NORM_BLOCKS = 512;

// per-clip control: the host table of one attempt, copied to the device in one piece.  Rows of B 32-bit words: dt, the six stage times
// (row 1 doubles as the time of the two initial evaluations), and the commit of the PREVIOUS attempt (accept flag, checkpoint index)
enum { TAB_DT = 0, TAB_T1 = 1, TAB_ACCEPT = 7, TAB_CKPT = 8, TAB_ROWS = 9 };
size_t clips_tab_bytes(int B) { return fd_align(sizeof(float) * TAB_ROWS * (size_t)B); }
size_t clips_partial_bytes(int B) { return fd_align(sizeof(double) * DP_NORM_BLOCKS * (size_t)B); }

// The workspace of both modes (offsets): x | x_new | err | k[7] (ten states), the norm's partials, the per-clip table, forward scratch
struct adaptive_layout_t { size_t state, partial, tab, fws, total; };
adaptive_layout_t adaptive_layout(const fd_model* m, int B, int T, bool per_clip) {
  adaptive_layout_t s;
  s.state = fd_align(sizeof(float) * 2 * (size_t)B * m->n_freq * T);
  s.partial = 10 * s.state;
  s.tab = s.partial + clips_partial_bytes(per_clip ? B : 1);
  s.fws = s.tab + (per_clip ? clips_tab_bytes(B) : 0);
  s.total = s.fws + forward_ws_bytes(m, B, T);
  return s;
}

// What the two policies share: the problem and the carved workspace
struct AdaptiveCtx {
  fd_model* m; const float* Y; float* traj; int B, T; float atol, rtol; hipStream_t st;
  size_t nclip, nstate;   // complex elements of one clip, of the batch
  float *x, *x_new, *err, *k[7]; double* partial; float* tab_dev; void* fws; size_t fws_bytes;
  AdaptiveCtx(fd_model* m_, const float* Y_, float* traj_, int B_, int T_, float atol_, float rtol_, hipStream_t st_, void* ws, size_t ws_bytes,
              const adaptive_layout_t& lay)
      : m(m_), Y(Y_), traj(traj_), B(B_), T(T_), atol(atol_), rtol(rtol_), st(st_), nclip((size_t)m_->n_freq * T_), nstate((size_t)B_ * nclip) {
    char* base = (char*)ws;
    x = (float*)base; x_new = (float*)(base + lay.state); err = (float*)(base + 2 * lay.state);
    for (int i = 0; i < 7; ++i) k[i] = (float*)(base + (3 + i) * lay.state);
    partial = (double*)(base + lay.partial); tab_dev = (float*)(base + lay.tab);
    fws = base + lay.fws; fws_bytes = ws_bytes - lay.fws;
  }
  int forward(const float* xin, const float* t, float t_imm, int nt, float* kout) const {
    OutSpec os; os.dst = kout; os.coef = 1.f;
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
  int eval(const float* xin, int, const float* t, float* kout) { return forward(xin, nullptr, t[0], 1, kout); }
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
  int step_limit(int, const StepCtl& c) const {
    return fd_set_error(FD_ERUNTIME, "fd_ode_solve_adaptive: step limit reached (dt = %g at t = %g)", (double)c.dt, (double)c.t);
  }
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
    FD_HIP(hipMemcpyAsync(tab_dev, tab, sizeof(float) * TAB_ROWS * (size_t)B, hipMemcpyHostToDevice, st));
    const int* accept_dev = (const int*)tab_dev + (size_t)TAB_ACCEPT * B;
    const int* ckpt_dev = (const int*)tab_dev + (size_t)TAB_CKPT * B;
    if (pending) FD_TRY(fd_ode_commit_clips(accept_dev, ckpt_dev, x_new, k[6], x, k[0], traj, B, (long long)nclip, st));
    return FD_OK;
  }
  int combine(float cx, const float*, const float* const* kk, const float* cc, int nk, float* dst) {
    return fd_ode_lincomb_clips(x, cx, tab_dev + (size_t)TAB_DT * B, kk, cc, nk, dst, B, (long long)nclip, st);
  }
  int eval(const float* xin, int slot, const float*, float* kout) {   // clip b at time tab[TAB_T1 + slot][b]
    return forward(xin, tab_dev + (size_t)(TAB_T1 + slot) * B, 0.f, B, kout);
  }
  // the Hairer norm of the one-clip call, clip by clip: the clip's DP_NORM_BLOCKS partials summed in index order
  int norm(const float* p_, const float* q_, const float* r_, const float* s_, double* out) {
    const double* host_partial = (const double*)((char*)m->pin_clips + clips_tab_bytes(fd_model::MAX_NT));
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
  int step_limit(int b, const StepCtl& c) const {
    return fd_set_error(FD_ERUNTIME, "fd_ode_solve_adaptive_clips: step limit reached (clip %d: dt = %g at t = %g)", b, (double)c.dt, (double)c.t);
  }
};

// The solve: x0, the initial-step probe, then attempts until every controller has reached the end of the span.  nfe / rejected: per
// controller (2 + 6 per attempt it was active in); *evals: network evaluations enqueued.  Ends synchronised, the result in X_out.
template <typename Policy>
int adaptive_solve(Policy& p, const Tableau& tb, int N, const fd_noise_src& noise, float sigma_fac, float* X_out, int nctl, int* nfe, int* rejected,
                   int* evals) {
  const size_t state_bytes = sizeof(float) * 2 * p.nstate;
  FD_TRY(fd_init_state(p.Y, noise, p.m->sigma_dev, p.m->sigma_n, sigma_fac, p.x, p.B, p.m->n_freq, p.T, p.st));
  if (p.traj) FD_HIP(hipMemcpyAsync(p.traj, p.x, state_bytes, hipMemcpyDeviceToDevice, p.st));
  const std::vector<float> ts = t_span_linspace(N);
  std::vector<StepCtl> c(nctl);
  std::vector<double> d0(nctl), d1(nctl), d2(nctl), h0(nctl), ratio(nctl);
  std::vector<float> dt(nctl, 0.f), tq(6 * (size_t)nctl, 0.f);   // per controller: the step, and the times of the (up to) six evaluations ahead
  std::vector<int> accept(nctl, 0), landed(nctl, 0);
  std::vector<char> act(nctl, 0);
  *evals = 0;
  auto eval = [&](const float* xin, int slot, float* kout) { ++*evals; return p.eval(xin, slot, &tq[(size_t)slot * nctl], kout); };
  auto publish = [&](bool pending) { return p.publish(dt.data(), tq.data(), accept.data(), landed.data(), pending); };
  for (int b = 0; b < nctl; ++b) { c[b].t = ts[0]; tq[b] = c[b].t; }
  FD_TRY(publish(false));
  FD_TRY(eval(p.x, 0, p.k[0]));
  FD_TRY(p.norm(p.x, nullptr, p.x, p.x, d0.data()));
  FD_TRY(p.norm(p.k[0], nullptr, p.x, p.x, d1.data()));
  for (int b = 0; b < nctl; ++b) {
    h0[b] = StepCtl::probe_step(d0[b], d1[b]);
    dt[b] = (float)h0[b];
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
      act[b] = c[b].active(ts, N);
      any = any || act[b];
      if (act[b]) c[b].begin(ts, N);
      dt[b] = act[b] ? c[b].dt : 0.f;                                // a finished clip: dt = 0, evaluated at its final time, never committed
      for (int s = 1; s < 7; ++s) tq[(size_t)(s - 1) * nctl + b] = act[b] ? c[b].stage_time(tb.C[s]) : c[b].t;
    }
    if (!any && !pending) break;
    FD_TRY(publish(pending));
    if (!any) break;
    if (++steps > ADAPTIVE_MAX_ATTEMPTS) {
      int b = 0;
      while (!act[b]) ++b;
      return p.step_limit(b, c[b]);
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
      accept[b] = c[b].end(ratio[b], ts, N, &landed[b]) ? 1 : 0;
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
  int nfe = 0, rejected = 0, evals = 0;
  FD_TRY(adaptive_solve(p, adaptive_tableau(method), N, fd_noise_src{noise}, sigma_fac, X_out, 1, &nfe, &rejected, &evals));
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
  if (!m->pin_clips) FD_HIP(hipHostMalloc(&m->pin_clips, clips_tab_bytes(fd_model::MAX_NT) + clips_partial_bytes(fd_model::MAX_NT), hipHostMallocDefault));
  ClipPolicy p(m, Y, traj, B, T_pad, atol, rtol, fd_stream(stream), ws, ws_bytes, lay);
  std::vector<int> nfe(B), rejected(B);
  int evals = 0;
  FD_TRY(adaptive_solve(p, adaptive_tableau(method), N, seeds ? fd_noise_src{nullptr, seeds, 0} : fd_noise_src{noise}, sigma_fac, X_out, B, nfe.data(),
                        rejected.data(), &evals));
  for (int b = 0; b < B; ++b) { nfe_out[b] = nfe[b]; if (rejected_out) rejected_out[b] = rejected[b]; }
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
  const float std_t = ouve_std(*c, t), g = ouve_diffusion(*c, t);
  OutSpec os; os.score = true; os.base = x; os.yv = Y; os.dst = out;
  if (mode == FD_SCORE_DENOISE) {   // x_mean = x - (theta (y - x) dt - G^2 score), G = g sqrt(dt), score = -net / std
    const float dt = 1.f / (float)c->N, G = g * sqrtf(dt);
    os.cb = 1.f + c->theta * dt; os.cy = -c->theta * dt; os.coef = -(G * G) / std_t;
  } else {                          // drift = theta (y - x) - g^2 score * (0.5 | 1)
    os.cb = -c->theta; os.cy = c->theta; os.coef = (mode == FD_SCORE_DRIFT_PF ? 0.5f : 1.f) * g * g / std_t;
  }
  return forward_call(m, x, Y, nullptr, t, 1, os, B, T_pad, ws, ws_bytes, fd_stream(stream));
}
