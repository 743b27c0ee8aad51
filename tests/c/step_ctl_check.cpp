// step_ctl_check.cpp -- the host arithmetic of the solvers (flowdec_amd/csrc/step_ctl.h), stand-alone and without a GPU.
//
//   step_ctl_check trace METHOD N D0 D1 D2 RATIO...   drive ONE StepCtl the way solve.hip's adaptive_solve does, with the given Hairer
//                                                     norms of the initial-step probe and the error ratios used cyclically
//   step_ctl_check grids NMAX START END               t_span_linspace(N), linspace_f32(START, END, N) and solver_nfe(id, N), N = 1..NMAX
//
// Every float is printed as %a (exact).  tests/test_model_host_cpu.py compares `trace` line for line with
// tests/golden/step_ctl_traces.json and `grids` bit for bit with the oracle's functions of the same names.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "step_ctl.h"

using namespace fdm;

static int trace(int argc, char** argv) {
  if (argc < 8) return 2;
  const int method = atoi(argv[2]), N = atoi(argv[3]);
  const double d0 = strtod(argv[4], nullptr), d1 = strtod(argv[5], nullptr), d2 = strtod(argv[6], nullptr);
  std::vector<double> ratios;
  for (int i = 7; i < argc; ++i) ratios.push_back(strtod(argv[i], nullptr));
  const Tableau tb = adaptive_tableau(method);
  const std::vector<float> ts = t_span_linspace(N);
  printf("ts");
  for (float t : ts) printf(" %a", (double)t);
  printf("\n");
  StepCtl c;
  c.t = ts[0];
  const double h0 = StepCtl::probe_step(d0, d1);
  printf("probe h0 %a t %a\n", h0, (double)c.probe_time(h0));
  c.first_step(h0, d1, d2);
  printf("first dt %a\n", (double)c.dt);
  int attempts = 0;
  while (c.active(ts, N)) {
    if (attempts == 10000) { printf("no end after 10000 attempts\n"); return 1; }
    c.begin(ts, N);
    printf("begin dt %a stages", (double)c.dt);
    for (int s = 1; s < 7; ++s) printf(" %a", (double)c.stage_time(tb.C[s]));
    printf("\n");
    int landed = 0;
    const bool accept = c.end(ratios[attempts % ratios.size()], ts, N, &landed);
    printf("end accept %d landed %d t %a dt %a\n", accept ? 1 : 0, landed, (double)c.t, (double)c.dt);
    ++attempts;
  }
  printf("done attempts %d t %a\n", attempts, (double)c.t);
  return 0;
}

static int grids(int argc, char** argv) {
  if (argc != 5) return 2;
  const int nmax = atoi(argv[2]);
  const float start = strtof(argv[3], nullptr), end = strtof(argv[4], nullptr);
  for (int N = 1; N <= nmax; ++N) {
    printf("t_span %d", N);
    for (float t : t_span_linspace(N)) printf(" %a", (double)t);
    printf("\nlinspace %d", N);
    for (float t : linspace_f32(start, end, N)) printf(" %a", (double)t);
    printf("\nnfe %d", N);
    const int ids[5] = {FD_SOLVER_EULER, FD_SOLVER_MIDPOINT, FD_SOLVER_HEUN2, FD_SOLVER_HEUN2_EULERLAST, -1};
    for (int id : ids) printf(" %d", solver_nfe(id, N));
    printf("\n");
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "trace")) return trace(argc, argv);
  if (argc >= 2 && !strcmp(argv[1], "grids")) return grids(argc, argv);
  fprintf(stderr, "usage: step_ctl_check trace METHOD N D0 D1 D2 RATIO... | grids NMAX START END\n");
  return 2;
}
