// step_ctl.h -- the host arithmetic of the solvers (solve.hip): the time grids, the fixed-step NFE count, the two embedded Runge-Kutta
// tableaux and the two adaptive step-size controllers (StepCtl: torchdyn's rule, the flow model's dopri5 / tsit5; Rk45Ctl: scipy RK45's rule,
// the ScoreDec ODE sampler).  Host-only: no HIP, so that a plain C++ compiler builds it alone (tests/c/step_ctl_check.cpp,
// tests/c/rk45_ctl_check.cpp); the controllers decide accept / reject on exactly these roundings.
#pragma once
#include <math.h>

#include <vector>

#include "flowdec_hip.h"

namespace fdm {

// torch.linspace(0, 1, N+1) in float32 with ATen's fused multiply-add evaluation (see oracle t_span_linspace)
inline std::vector<float> t_span_linspace(int N) {
  const int steps = N + 1;
  std::vector<float> out(steps);
  const float step = 1.0f / (float)(steps - 1);
  const int half = steps / 2;
  for (int i = 0; i < steps; ++i) out[i] = i < half ? fmaf(step, (float)i, 0.0f) : fmaf(-step, (float)(steps - 1 - i), 1.0f);
  return out;
}

inline int solver_nfe(int solver, int N) {
  switch (solver) {
    case FD_SOLVER_EULER: return N;
    case FD_SOLVER_MIDPOINT: case FD_SOLVER_HEUN2: return 2 * N;
    case FD_SOLVER_HEUN2_EULERLAST: return 2 * N - 1;
  }
  return -1;
}

// torch.linspace(start, end, steps) in float32 (see oracle linspace_f32)
inline std::vector<float> linspace_f32(float start, float end, int steps) {
  std::vector<float> out(steps);
  if (steps == 1) { out[0] = start; return out; }
  const float step = (end - start) / (float)(steps - 1);
  const int half = steps / 2;
  for (int i = 0; i < steps; ++i) out[i] = i < half ? fmaf(step, (float)i, start) : fmaf(-step, (float)(steps - 1 - i), end);
  return out;
}

// ---- adaptive Dormand-Prince 5(4) (torchdyn 'dopri5' semantics restated, see oracle odeint_dopri5; host-driven: one
// synchronisation per attempted step for the error ratio) --------------------------------------------------------------
const double DP_C[7] = {0.0, 1.0 / 5, 3.0 / 10, 4.0 / 5, 8.0 / 9, 1.0, 1.0};
const double DP_A[7][6] = {{0}, {1.0 / 5}, {3.0 / 40, 9.0 / 40}, {44.0 / 45, -56.0 / 15, 32.0 / 9},
                           {19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729},
                           {9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656},
                           {35.0 / 384, 0.0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84}};
// error weights b5 - b4 (the 5th-order weights b5 are the last row of DP_A; its 7th entry is 0)
const double DP_E[7] = {35.0 / 384 - 5179.0 / 57600, 0.0, 500.0 / 1113 - 7571.0 / 16695, 125.0 / 192 - 393.0 / 640,
                        -2187.0 / 6784 + 92097.0 / 339200, 11.0 / 84 - 187.0 / 2100, -1.0 / 40};
// Tsitouras 5(4) (torchdyn's `Tsitouras45` / `construct_tsit5`; coefficients as published, verified against the order conditions in
// tests/test_oracle_golden.py): the same 7-stage FSAL shape, E = the published error weights
const double TS_C[7] = {0.0, 0.161, 0.327, 0.9, 0.9800255409045097, 1.0, 1.0};
const double TS_A[7][6] = {{0}, {0.161}, {-0.008480655492356989, 0.335480655492357}, {2.8971530571054935, -6.359448489975075, 4.3622954328695815},
                           {5.325864828439257, -11.748883564062828, 7.4955393428898365, -0.09249506636175525},
                           {5.86145544294642, -12.92096931784711, 8.159367898576159, -0.071584973281401, -0.028269050394068383},
                           {0.09646076681806523, 0.01, 0.4798896504144996, 1.379008574103742, -3.290069515436081, 2.324710524099774}};
const double TS_E[7] = {-0.00178001105222577714, -0.0008164344596567469, 0.007880878010261995, -0.1447110071732629, 0.5823571654525552,
                        -0.45808210592918697, 0.015151515151515152};
struct Tableau { const double* C; const double (*A)[6]; const double* E; };
inline Tableau adaptive_tableau(int method) { return method == FD_ADAPTIVE_TSIT5 ? Tableau{TS_C, TS_A, TS_E} : Tableau{DP_C, DP_A, DP_E}; }

// The step-size controller of ONE solve over t_span `ts` (torchdyn's `_adaptive_odeint` restated, oracle odeint_adaptive): host scalars
// only.  fd_ode_solve_adaptive_method drives the whole batch with one instance, fd_ode_solve_adaptive_clips every clip with its own --
// the only implementation of this arithmetic, so that a clip of a per-clip batch takes the decisions of the one-clip call.
struct StepCtl {
  float t = 0.f, dt = 0.f, dt_old = 0.f;
  bool flag = false;
  int ckpt = 0;
  // initial step (Hairer): h0 = 0.01 d0 / d1, one explicit Euler probe at t + h0, h1 = (0.01 / max(d1, d2))^(1/6)
  static double probe_step(double d0, double d1) { return (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1; }
  float probe_time(double h0) const { return t + (float)h0; }
  void first_step(double h0, double d1, double d2) {   // d2 = the norm of k(t + h0) - k(t), not yet divided by h0
    d2 /= h0;
    const double h1 = (d1 <= 1e-15 && d2 <= 1e-15) ? fmax(1e-6, h0 * 1e-3) : pow(0.01 / fmax(d1, d2), 1.0 / 6.0);
    dt = (float)fmin(100.0 * h0, h1);
  }
  bool active(const std::vector<float>& ts, int N) const { return t < ts[N]; }
  // the step to attempt (left in dt): clamped to the end of the span, shortened to land on the next checkpoint
  void begin(const std::vector<float>& ts, int N) {
    const float T = ts[N];
    if (t + dt > T) dt = T - t;
    flag = false;
    dt_old = dt;
    if (ckpt < N && t + dt > ts[ckpt + 1]) { dt_old = dt; flag = true; dt = ts[ckpt + 1] - t; }
  }
  float stage_time(double c) const { return t + (float)c * dt; }
  // after the attempt: accept iff ratio <= 1 (-> true; *landed = the checkpoint the step reached, or 0), then the next step size
  bool end(double ratio, const std::vector<float>& ts, int N, int* landed) {
    const bool accept = ratio <= 1.0;
    *landed = 0;
    if (accept) {
      t = t + dt;
      if (ckpt < N && fabs((double)t - (double)ts[ckpt + 1]) <= 1e-7) {
        t = ts[ckpt + 1];
        *landed = ++ckpt;
      }
    }
    if (flag) dt = dt_old - dt;
    if (ratio == 0.0) dt = dt * 10.f;
    else {
      const double minf = ratio < 1.0 ? 1.0 : 0.2;
      dt = (float)((double)dt * fmin(10.0, fmax(0.9 / pow(ratio, 1.0 / 5.0), minf)));
    }
    return accept;
  }
};
// The step-size controller of scipy.integrate.RK45 (scipy/integrate/_ivp/rk.py: RungeKutta._step_impl, common.py: select_initial_step)
// restated for ONE solve backwards in time, from t0 down to t_bound (direction -1: the ScoreDec probability-flow ODE over (sde.T, eps)):
// double precision and scipy's order of operations, so that every t, h and accept flag is scipy's.  What differs from StepCtl: the
// initial step takes the estimator's order 4 (exponent 1/5, not 1/6) and is bounded by the span, a step is accepted on err < 1
// (strictly), the growth factor is capped at 1 once an attempt of the step was rejected, there are no checkpoints, and a step below ten
// spacings of t is an error (begin() -> false; scipy's TOO_SMALL_STEP).  Tableau: DP_C / DP_A / DP_E (scipy's E is -DP_E: the norm does
// not see the sign).  Time is a double here; the network is given (float)t.
struct Rk45Ctl {
  static constexpr double direction = -1.0;
  double t = 0.0, t_bound = 0.0, t_new = 0.0;
  double h = 0.0, h_abs = 0.0, min_step = 0.0;   // the signed step of the attempt, the controller's step size, ten spacings of t
  bool fresh = true, rejected = false;           // the next attempt opens a new step; an attempt of this step was rejected
  void start(double t0, double tb) { t = t0; t_bound = tb; fresh = true; }
  // select_initial_step: h0, then one explicit Euler probe x + direction h0 f0 at t + direction h0, d2 = |f1 - f0| / h0
  double probe_step(double d0, double d1) const {
    const double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
    return fmin(h0, fabs(t_bound - t));
  }
  double probe_time(double h0) const { return t + h0 * direction; }
  void first_step(double h0, double d1, double d2) {   // d2 already divided by h0
    const double h1 = (d1 <= 1e-15 && d2 <= 1e-15) ? fmax(1e-6, h0 * 1e-3) : pow(0.01 / fmax(d1, d2), 1.0 / 5.0);
    h_abs = fmin(fmin(100.0 * h0, h1), fabs(t_bound - t));
  }
  bool active() const { return direction * (t - t_bound) < 0.0; }
  // the attempt to make (left in h, t_new): -> false when the step size has fallen below min_step
  bool begin() {
    if (fresh) {
      min_step = 10.0 * fabs(nextafter(t, direction * INFINITY) - t);
      if (h_abs < min_step) h_abs = min_step;
      fresh = rejected = false;
    }
    if (h_abs < min_step) return false;
    t_new = t + h_abs * direction;
    if (direction * (t_new - t_bound) > 0.0) t_new = t_bound;
    h = t_new - t;
    h_abs = fabs(h);
    return true;
  }
  double stage_time(double c) const { return t + c * h; }
  // after the attempt: accept iff err < 1, then the next step size (a NaN norm rejects and shrinks by 0.2, like Python's max(0.2, nan))
  bool end(double err) {
    if (err < 1.0) {
      double factor = err == 0.0 ? 10.0 : fmin(10.0, 0.9 * pow(err, -1.0 / 5.0));
      if (rejected) factor = fmin(1.0, factor);
      h_abs *= factor;
      t = t_new;
      fresh = true;
      return true;
    }
    const double shrink = 0.9 * pow(err, -1.0 / 5.0);
    h_abs *= shrink > 0.2 ? shrink : 0.2;
    rejected = true;
    return false;
  }
};
constexpr int ADAPTIVE_MAX_ATTEMPTS = 100000;

}  // namespace fdm
