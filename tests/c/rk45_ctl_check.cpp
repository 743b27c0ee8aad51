// rk45_ctl_check.cpp -- the scipy RK45 step-size rule of the ScoreDec ODE sampler (Rk45Ctl, flowdec_amd/csrc/step_ctl.h), stand-alone and
// without a GPU.
//
//   rk45_ctl_check T0 T_BOUND D0 D1 D2 ERR...   drive ONE Rk45Ctl the way solve.hip's adaptive_solve does: the three norms of
//                                               select_initial_step (D2 already divided by h0), then one error norm per attempt
//
// Prints, with %.17g:  "probe h0 H0 t T", "first h_abs H", one "attempt t T h H t_new TN accept A h_abs HN" per attempt (h: the signed
// step, h_abs: the controller's step size after the attempt), and at the end "done attempts N t T", "small attempts N t T h_abs H
// min_step M" (the step size fell below ten spacings of t: the driver's error) or "short attempts N t T" (the error norms ran out).
// tests/test_score_ode_cpu.py compares the lines with scipy.integrate.RK45 itself.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "step_ctl.h"

using namespace fdm;

int main(int argc, char** argv) {
  if (argc < 6) {
    fprintf(stderr, "usage: rk45_ctl_check T0 T_BOUND D0 D1 D2 ERR...\n");
    return 2;
  }
  const double t0 = strtod(argv[1], nullptr), tb = strtod(argv[2], nullptr);
  const double d0 = strtod(argv[3], nullptr), d1 = strtod(argv[4], nullptr), d2 = strtod(argv[5], nullptr);
  std::vector<double> errs;
  for (int i = 6; i < argc; ++i) errs.push_back(strtod(argv[i], nullptr));
  Rk45Ctl c;
  c.start(t0, tb);
  const double h0 = c.probe_step(d0, d1);
  printf("probe h0 %.17g t %.17g\n", h0, c.probe_time(h0));
  c.first_step(h0, d1, d2);
  printf("first h_abs %.17g\n", c.h_abs);
  size_t attempts = 0;
  while (c.active()) {
    if (!c.begin()) {
      printf("small attempts %zu t %.17g h_abs %.17g min_step %.17g\n", attempts, c.t, c.h_abs, c.min_step);
      return 0;
    }
    if (attempts == errs.size()) {
      printf("short attempts %zu t %.17g\n", attempts, c.t);
      return 0;
    }
    const double t = c.t, h = c.h, t_new = c.t_new;
    const bool accept = c.end(errs[attempts++]);
    printf("attempt t %.17g h %.17g t_new %.17g accept %d h_abs %.17g\n", t, h, t_new, accept ? 1 : 0, c.h_abs);
  }
  printf("done attempts %zu t %.17g\n", attempts, c.t);
  return 0;
}
