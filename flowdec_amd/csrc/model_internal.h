// model_internal.h -- what the model's three translation units share (model.hip: structure, parameters, forward walk; solve.hip: the
// solvers and samplers; enhance.hip: the waveform entry points and the validation loss): struct fd_model and its parts, the per-model
// busy guard, the network's output spec, the hipGraph cache, and the functions that cross a file (namespace fdm).  internal.h stays the
// cross-file header of the operator files.
#pragma once
#include <atomic>
#include <map>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "common.h"
#include "internal.h"

namespace fdm {

enum ModKind { M_GFP, M_LINEAR, M_CONV_IN, M_RB, M_COMBINE, M_GN, M_CONV_HEAD, M_ATTN };

// How a model picks the kernel of each convolution (pick_conv): the algorithm flag of its act_dtype, resolved by fd_model_create.  The
// operand modes (FD_BF16_OPERANDS / FD_BF16X3_OPERANDS) and fd_resblock are CS_DIRECT; CS_AUTO_F32 is pure FD_F32 | FD_WINOGRAD_AUTO.
enum ConvSchedule { CS_DIRECT, CS_WINOGRAD, CS_WINOGRAD_LOWRES, CS_AUTO, CS_LATENCY, CS_AUTO_F32 };

// Packed weights of one convolution, one per kernel it may run (null where the schedule or that kernel's shape rules leave it out):
// direct (conv_mfma.hip), Winograd F(2,3) bf16 (conv_wino.hip), F(4,3) bf16 (conv_wino4.hip), 2-D F(4x4, 3x3) float32 (conv_wino44f.hip)
struct ConvW { const void *direct = nullptr, *f23 = nullptr, *f43 = nullptr, *f44 = nullptr; };

struct Mod {
  ModKind kind;
  int idx;              // index in all_modules
  int cin = 0, cout = 0;
  int c0 = 0, c1 = 0;   // virtual-concat split of cin (RB)
  bool up = false, down = false, has_c2 = false;
  int level = 0;                 // resolution level the block's convolutions run at (0 = full resolution)
  // device pointers (filled by finalize)
  ConvW conv0, conv1;   // RB: Conv_0 and Conv_1 (+ the folded 1x1 shortcut Conv_2); conv_in / pyramid head: conv0 (direct)
  float *gn0_g = nullptr, *gn0_b = nullptr, *gn1_g = nullptr, *gn1_b = nullptr;
  float* b1 = nullptr;                     // Conv_1 bias (+ Conv_2 bias when the shortcut conv is folded in)
  float* bias0_eff = nullptr;              // [nt][cout] Conv_0 bias + Dense_0(silu(temb)), model-owned scratch
  float *w_f32 = nullptr, *b_f32 = nullptr;  // small f32 weights (conv_in, combine, head bias, gn affine; attention: NIN_3)
  float *w_qkv = nullptr, *b_qkv = nullptr;  // attention: NIN_0 | NIN_1 | NIN_2 packed side by side ([C][3C], [3C])
};

struct ParamInfo {
  std::string name;
  std::vector<int> shape;
  long long numel() const { long long n = 1; for (int s : shape) n *= s; return n; }
};

// Everything a captured solve bakes into its kernel arguments.  Compared field by field (a memcmp over the struct would read
// its padding bytes).
struct GraphKey {
  const void *Y = nullptr, *noise = nullptr, *X = nullptr, *traj = nullptr, *ws = nullptr, *y = nullptr, *xhat = nullptr, *lens = nullptr, *seeds = nullptr,
             *frame0 = nullptr, *normfac_in = nullptr;   // fd_enhance_chunks
  int B = 0, T = 0, N = 0, solver = 0, L = 0, kind = 0, normalize = 1;
  float sigma_fac = 0.f;
  fd_score_config score{};   // kind 3 only (zero otherwise)
  auto tie() const {
    return std::tie(Y, noise, X, traj, ws, y, xhat, lens, seeds, frame0, normfac_in, B, T, N, solver, L, kind, normalize, sigma_fac, score.theta, score.sigma_min, score.sigma_max,
                    score.t_eps, score.snr, score.N, score.predictor, score.corrector, score.corrector_steps, score.denoise);
  }
  bool operator<(const GraphKey& o) const { return tie() < o.tie(); }
};

}  // namespace fdm

struct fd_model {
  fd_model_config cfg;
  fd_model_arch arch{0, 1};
  int dt = FD_BF16;                 // storage type (cfg.act_dtype without the algorithm flags)
  fdm::ConvSchedule sched = fdm::CS_DIRECT;   // kernel choice per convolution (cfg.act_dtype's algorithm flags)
  int opflag = 0;                   // FD_BF16_OPERANDS / FD_BF16X3_OPERANDS of cfg.act_dtype: or'ed into every packing and launch
  int n_freq = 0, temb_dim = 0;
  std::vector<fdm::Mod> mods;
  std::vector<fdm::ParamInfo> params;
  std::map<std::string, std::vector<float>> host;   // staged parameters
  std::map<std::string, float*> dev_f32;            // uploaded f32 copies
  std::vector<void*> dev_allocs;
  std::vector<double> sigma_host;
  double* sigma_dev = nullptr;
  int sigma_n = 0;
  bool finalized = false;
  float* temb = nullptr;            // [MAX_NT][temb_dim]
  fd_temb_job* jobs_dev = nullptr;
  int njobs = 0;
  float* wo = nullptr;              // output_layer weight [2][4][ks][ks]
  fd_stft_plan* stft = nullptr;
  std::map<fdm::GraphKey, hipGraphExec_t> graphs;
  std::set<fdm::GraphKey> seen;     // keys that ran once eagerly: a solve is captured at its SECOND sighting
  int normalize = 1;                // front end: 1 = per-clip max-abs normalisation ('noisy'), 0 = 'none'
  // second stream for the side branches of one network evaluation (time embedding, pyramid-head chain): forked from / joined into
  // the caller's stream with events, also inside a graph capture (parallel branches of the captured graph)
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  // profiling of the dominant kernel (conv MFMA)
  bool profiling = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
  size_t ev_used = 0;
  double prof_flops = 0.0;
  double prof_flops_exec = 0.0;   // multiply-adds the chosen algorithm executes (Winograd launches: fewer than the direct count)
  double prof_bytes = 0.0;   // algorithmic HBM bytes of the timed launches: every operand read once + output written once
  // second class: the FIR resampling launches (HBM-bound): events + algorithmic bytes
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_fir;
  size_t ev_fir_used = 0;
  double prof_fir_bytes = 0.0;
  static constexpr int MAX_NT = 256;
  void* pin_clips = nullptr;        // pinned host memory of fd_ode_solve_adaptive_clips (per-attempt table + error partials), made at its first call
  // One enqueueing call at a time per model: the entry points below share the model's scratch (time-embedding biases, graph cache,
  // side stream, profiling events).  A second thread entering while one is inside gets FD_EBUSY instead of corrupting that state;
  // callers that want concurrency create one fd_model per thread (weights are ~50 MB).  The reference's own native ops are
  // stateless and re-entrant (upfirdn2d_kernel.cu:224-231) -- so are fd_upfirdn2d / fd_conv2d / the other operator-level calls.
  std::atomic_flag busy = ATOMIC_FLAG_INIT;
};

namespace fdm {

struct BusyGuard {
  fd_model* m; bool ok;
  explicit BusyGuard(fd_model* mm) : m(mm), ok(mm && !mm->busy.test_and_set(std::memory_order_acquire)) {}
  ~BusyGuard() { if (ok) m->busy.clear(std::memory_order_release); }
};

struct OutSpec {           // what to do with v = NCSNpp(x, y, t):  dst = base + coef * (v + kold); ksave = v
  const float* base = nullptr;
  const float* kold = nullptr;
  float coef = 1.f;
  float* dst = nullptr;
  float* ksave = nullptr;
  // score-sampler form (score = true):  dst = cb * base + cy * yv + coef * v + cz * z
  bool score = false;
  const float* yv = nullptr;
  fd_noise_src z;
  float cb = 1.f, cy = 0.f, cz = 0.f;
  // per-clip score form (ctab given; no noise term): clip b reads (cb, cy, coef) from ctab[b][0..2] (DEVICE float [B][3])
  const float* ctab = nullptr;
};

// model.hip
int check_ready(const fd_model* m);
int check_shape(const fd_model* m, int B, int T);
size_t forward_ws_bytes(const fd_model* m, int B, int T);
int forward_call(fd_model* m, const float* x, const float* y, const float* t, float t_imm, int nt, const OutSpec& os, int B, int T, void* ws,
                 size_t ws_bytes, hipStream_t st);
// solve.hip
size_t ode_ws_bytes(const fd_model* m, int B, int T);
int ode_enqueue(fd_model* m, const float* Y, const fd_noise_src& noise, float sigma_fac, int N, int solver, float* X, float* traj, int B, int T, void* ws,
                size_t ws_bytes, hipStream_t st);
int score_enqueue(fd_model* m, const float* Y, const fd_noise_src& noise, const fd_score_config& c, float* X, int B, int T, void* ws, size_t ws_bytes,
                  hipStream_t st);
// the ScoreDec ODE sampler on features (fd_score_ode_solve / fd_score_ode_enhance): argument checks, workspace, the synchronous solve
int score_ode_check(const char* who, const fd_score_config* c, float rtol, float atol, int step_control, int B);
size_t score_ode_ws_bytes(const fd_model* m, int B, int T, bool per_clip);
int score_ode_run(fd_model* m, const char* who, const float* Y, const fd_noise_src& noise, const fd_score_config& c, float rtol, float atol, bool per_clip,
                  float* X, int* nfe, int* rejected, int* evals, int B, int T, void* ws, size_t ws_bytes, hipStream_t st);

template <typename Fn>
int run_maybe_graph(fd_model* m, const GraphKey& key, bool use_graph, hipStream_t st, Fn&& enqueue) {
  if (!use_graph || m->profiling) return enqueue();
  auto it = m->graphs.find(key);
  if (it == m->graphs.end()) {
    // A caller that walks a data set (one clip length per file) would capture and instantiate a ~1600-node graph per call and
    // never replay it: the first sighting of a key runs eagerly, only a repeated key is captured.
    if (!m->seen.count(key)) {
      if (m->seen.size() >= 256) m->seen.clear();
      m->seen.insert(key);
      return enqueue();
    }
    if (m->graphs.size() >= 32) {   // the key holds raw buffer pointers: bound the cache for callers that keep changing them
      FD_HIP(hipStreamSynchronize(st));   // (rare path) nothing captured earlier may still be in flight when it is destroyed
      for (auto& g : m->graphs) (void)hipGraphExecDestroy(g.second);
      m->graphs.clear();
    }
    hipGraph_t graph = nullptr;
    FD_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    const int rc = enqueue();
    const hipError_t e = hipStreamEndCapture(st, &graph);
    if (rc != FD_OK) { if (graph) (void)hipGraphDestroy(graph); return rc; }
    if (e != hipSuccess) return fd_set_error(FD_ERUNTIME, "hipStreamEndCapture failed: %s", hipGetErrorString(e));
    hipGraphExec_t exec = nullptr;
    FD_HIP(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
    (void)hipGraphDestroy(graph);
    it = m->graphs.emplace(key, exec).first;
  }
  FD_HIP(hipGraphLaunch(it->second, st));
  return FD_OK;
}

}  // namespace fdm

#define FD_MODEL_ENTER(m, fn)                                                                                                   \
  FD_REQUIRE(m, fn ": null model");                                                                                             \
  fdm::BusyGuard fd_busy_guard_(m);                                                                                             \
  if (!fd_busy_guard_.ok) return fd_set_error(FD_EBUSY, fn ": the model is serving a call of another thread (one enqueueing call at a time per fd_model)")
