// ops_api.hip -- operator-level C ABI of the kernels between the network and the ODE / SDE solvers and of the time-conditioning kernels
// (include/flowdec_hip.h, "Operator-level: solver and edge kernels").  Every entry point checks its arguments and then calls the launcher
// the model and the solvers call (fd_edge_*, fd_init_state, fd_caxpy, fd_ode_*, fd_time_embedding_impl, fd_temb_bias_batched: internal.h).  No kernel and no launch configuration lives here, so a test
// of one of these functions is a test of the production launch.  A refused call launches nothing.
#include <limits.h>
#include <stdint.h>

#include <vector>

#include "common.h"
#include "internal.h"

namespace {

constexpr int MAX_GRID_Y = 65535;
constexpr int MAX_GRID_X_256 = (1 << 24) - 1;       // HIP: gridDim.x * blockDim.x < 2^32, with the 256-thread blocks of these kernels
// Dynamic LDS one workgroup of the time-conditioning kernels may ask for.  A compile-time figure, so that the refusal needs no device:
// the 64 KiB every CDNA device grants a workgroup (gfx950 itself has 160 KiB); nf <= 2730 and temb_dim <= 16384 are far beyond any model.
constexpr long long MAX_DYN_LDS_BYTES = 64 * 1024;

// fd_row_dot (net_edges.hip) reads a weight row as 16-byte vectors: with a row length that is a multiple of 4 floats every row is
// aligned when the base pointer is
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// dtype, B >= 1 and an H x W image whose pixel count fits the kernels' int arithmetic
int check_image(const char* who, int B, int H, int W, int dtype) {
  FD_REQUIRE(dtype == FD_BF16 || dtype == FD_F32, "%s: dtype must be FD_BF16 or FD_F32 (got %d)", who, dtype);
  FD_REQUIRE(B >= 1 && H >= 1 && W >= 1, "%s: bad shape (B=%d H=%d W=%d)", who, B, H, W);
  FD_REQUIRE((long long)H * W <= INT_MAX, "%s: H * W = %lld does not fit 31 bits", who, (long long)H * W);
  return FD_OK;
}

// exactly one source of a [B][F][T] noise plane
int check_noise(const char* who, const float* buf, const unsigned long long* seeds, int draw) {
  FD_REQUIRE((buf != nullptr) != (seeds != nullptr), "%s: exactly one of a noise buffer or seeds must be given (got %s)", who,
             buf ? "both" : "neither");
  FD_REQUIRE(!seeds || draw >= 0, "%s: bad draw index %d", who, draw);
  return FD_OK;
}

// the k / c tables of a linear combination: at most 7 terms, host arrays present when there is a term
int check_lincomb(const char* who, const float* x, float cx, const float* const* k, const float* c, int nk, const float* dst, long long n) {
  FD_REQUIRE(dst, "%s: null pointer (dst)", who);
  FD_REQUIRE(nk >= 0 && nk <= 7, "%s: nk must be in [0, 7] (got %d)", who, nk);
  FD_REQUIRE(nk == 0 || (k && c), "%s: null pointer (k / c tables)", who);
  FD_REQUIRE(x || cx == 0.f, "%s: null pointer (x with cx != 0)", who);
  FD_REQUIRE(n >= 1, "%s: bad element count n=%lld", who, n);
  return FD_OK;
}

int check_scaled_sq(const char* who, const float* p, const float* r, const float* s, const double* partial, int nblocks, long long n) {
  FD_REQUIRE(p && r && s && partial, "%s: null pointer", who);
  FD_REQUIRE(nblocks >= 1, "%s: nblocks must be >= 1 (got %d)", who, nblocks);
  FD_REQUIRE(n >= 1, "%s: bad element count n=%lld", who, n);
  return FD_OK;
}

}  // namespace

// ---- time conditioning: the checks shared by fd_time_embedding / fd_temb_bias (net_edges.hip) and their fd_op_* forms ---------------
int fd_check_time_embedding(const char* who, int nt, const float* gfp_w, int nf, const float* w1, const float* b1, const float* w2,
                            const float* b2, const float* temb) {
  FD_REQUIRE(gfp_w, "%s: null pointer (gfp_w)", who);
  FD_REQUIRE(w1 && b1, "%s: null pointer (w1 / b1)", who);
  FD_REQUIRE(w2 && b2, "%s: null pointer (w2 / b2)", who);
  FD_REQUIRE(temb, "%s: null pointer (temb)", who);
  FD_REQUIRE(nt >= 1 && nt <= MAX_GRID_X_256, "%s: nt must be in [1, %d] (got %d)", who, MAX_GRID_X_256, nt);
  // rows of 2 nf and 4 nf floats are read as 4-float vectors
  FD_REQUIRE(nf >= 2 && nf % 2 == 0, "%s: nf must be even and >= 2 (got %d)", who, nf);
  FD_REQUIRE(6LL * nf * (long long)sizeof(float) <= MAX_DYN_LDS_BYTES, "%s: nf = %d needs %lld bytes of shared memory (6 nf floats), above the limit of %lld",
             who, nf, 6LL * nf * (long long)sizeof(float), MAX_DYN_LDS_BYTES);
  FD_REQUIRE(aligned16(w1), "%s: w1 is not 16-byte aligned", who);
  FD_REQUIRE(aligned16(w2), "%s: w2 is not 16-byte aligned", who);
  return FD_OK;
}

int fd_check_temb_bias(const char* who, const float* temb, int nt, int temb_dim) {
  FD_REQUIRE(temb, "%s: null pointer (temb)", who);
  FD_REQUIRE(nt >= 1 && nt <= MAX_GRID_X_256, "%s: nt must be in [1, %d] (got %d)", who, MAX_GRID_X_256, nt);
  FD_REQUIRE(temb_dim >= 4 && temb_dim % 4 == 0, "%s: temb_dim must be a multiple of 4 and >= 4 (got %d)", who, temb_dim);
  FD_REQUIRE((long long)temb_dim * (long long)sizeof(float) <= MAX_DYN_LDS_BYTES, "%s: temb_dim = %d needs %lld bytes of shared memory, above the limit of %lld",
             who, temb_dim, (long long)temb_dim * (long long)sizeof(float), MAX_DYN_LDS_BYTES);
  return FD_OK;
}

// job < 0: the single form (no job index in the message)
int fd_check_temb_job(const char* who, int job, const float* dense_w, const float* dense_b, const float* out, int Cout) {
  char where[32] = "";
  if (job >= 0) snprintf(where, sizeof where, " of job %d", job);
  FD_REQUIRE(dense_w && dense_b, "%s: null pointer (dense_w / dense_b%s)", who, where);
  FD_REQUIRE(out, "%s: null pointer (out%s)", who, where);
  FD_REQUIRE(Cout >= 1, "%s: Cout%s must be >= 1 (got %d)", who, where, Cout);
  FD_REQUIRE(aligned16(dense_w), "%s: dense_w%s is not 16-byte aligned", who, where);
  return FD_OK;
}

extern "C" int fd_op_time_embedding(const float* t, float t_imm, int nt, const float* gfp_w, int nf, const float* w1, const float* b1,
                                    const float* w2, const float* b2, float* temb, void* stream) {
  FD_TRY(fd_check_time_embedding("fd_op_time_embedding", nt, gfp_w, nf, w1, b1, w2, b2, temb));
  return fd_time_embedding_impl(t, t_imm, nt, gfp_w, nf, w1, b1, w2, b2, temb, fd_stream(stream));
}

extern "C" int fd_op_temb_bias_jobs(const float* temb, int nt, int temb_dim, const float* const* dense_w, const float* const* dense_b,
                                    const float* const* conv_b, float* const* out, const int* cout, int njobs, void* stream) {
  FD_TRY(fd_check_temb_bias("fd_op_temb_bias_jobs", temb, nt, temb_dim));
  FD_REQUIRE(nt <= MAX_GRID_Y, "fd_op_temb_bias_jobs: nt must be in [1, 65535] (got %d)", nt);
  FD_REQUIRE(njobs >= 1 && njobs <= MAX_GRID_X_256, "fd_op_temb_bias_jobs: njobs must be in [1, %d] (got %d)", MAX_GRID_X_256, njobs);
  FD_REQUIRE(dense_w && dense_b && conv_b && out && cout, "fd_op_temb_bias_jobs: null pointer (job tables)");
  std::vector<fd_temb_job> jobs((size_t)njobs);
  for (int j = 0; j < njobs; ++j) {
    FD_TRY(fd_check_temb_job("fd_op_temb_bias_jobs", j, dense_w[j], dense_b[j], out[j], cout[j]));
    // the batched kernel reads conv_b unconditionally: only fd_temb_bias takes NULL as "no conv bias"
    FD_REQUIRE(conv_b[j], "fd_op_temb_bias_jobs: null pointer (conv_b of job %d)", j);
    jobs[j] = fd_temb_job{dense_w[j], dense_b[j], conv_b[j], out[j], cout[j]};
  }
  fd_temb_job* jobs_dev = nullptr;
  FD_HIP(hipMalloc(&jobs_dev, sizeof(fd_temb_job) * jobs.size()));
  int rc = FD_OK;
  if (hipMemcpy(jobs_dev, jobs.data(), sizeof(fd_temb_job) * jobs.size(), hipMemcpyHostToDevice) != hipSuccess)
    rc = fd_set_error(FD_ERUNTIME, "fd_op_temb_bias_jobs: copying the job table failed");
  if (rc == FD_OK) rc = fd_temb_bias_batched(jobs_dev, njobs, temb, nt, temb_dim, fd_stream(stream));
  // the kernel reads the table: it is released only once the stream has finished with it (a synchronous entry point, for tests)
  if (hipStreamSynchronize(fd_stream(stream)) != hipSuccess && rc == FD_OK)
    rc = fd_set_error(FD_ERUNTIME, "fd_op_temb_bias_jobs: hipStreamSynchronize failed");
  hipFree(jobs_dev);
  return rc;
}

extern "C" int fd_op_pack_input(const float* x, const float* y, void* out8, int B, int H, int W, int dtype, void* stream) {
  FD_REQUIRE(x && y && out8, "fd_op_pack_input: null pointer");
  FD_TRY(check_image("fd_op_pack_input", B, H, W, dtype));
  fd_edge_args a;
  a.x = x; a.y = y; a.out = out8; a.B = B; a.H = H; a.W = W;
  return fd_edge_pack_input(a, dtype, fd_stream(stream));
}

extern "C" int fd_op_combine(const void* p4, const float* w, const float* bias, const void* h, void* out, float* stats, int B, int H, int W,
                             int Cout, int dtype, void* stream) {
  FD_REQUIRE(p4 && w && bias && h && out && stats, "fd_op_combine: null pointer");
  FD_TRY(check_image("fd_op_combine", B, H, W, dtype));
  FD_REQUIRE(B <= MAX_GRID_Y, "fd_op_combine: B must be in [1, 65535] (got %d)", B);
  FD_REQUIRE(Cout >= 8 && Cout <= 256 && (Cout & (Cout - 1)) == 0, "fd_op_combine: Cout must be a power of two in [8, 256] (got %d)", Cout);
  fd_edge_args a;
  a.x = p4; a.w = w; a.bias = bias; a.y = h; a.out = out; a.stats = stats; a.B = B; a.H = H; a.W = W; a.Cout = Cout;
  return fd_edge_combine(a, dtype, fd_stream(stream));
}

extern "C" int fd_op_output_update(const void* pyr, const float* w, const float* base, const float* kold, float coef, float* dst, float* ksave,
                                   int B, int H, int W, int ks, int dtype, void* stream) {
  FD_REQUIRE(pyr && w && dst, "fd_op_output_update: null pointer");
  FD_TRY(check_image("fd_op_output_update", B, H, W, dtype));
  FD_REQUIRE(ks == 1 || ks == 3, "fd_op_output_update: ks must be 1 or 3 (got %d)", ks);
  fd_edge_args a;
  a.x = pyr; a.w = w; a.base = base; a.kold = kold; a.coef = coef; a.out = dst; a.ksave = ksave; a.B = B; a.H = H; a.W = W; a.ks = ks;
  return fd_edge_output_update(a, dtype, fd_stream(stream));
}

static int op_score_update(const char* who, const void* pyr, const float* w, const float* base, float cb, const float* Y, float cy, float cn,
                           const float* z, const unsigned long long* seeds, const int* frame0, int draw, float cz, float* dst, int B, int H, int W,
                           int ks, int dtype, void* stream) {
  FD_REQUIRE(pyr && w && base && dst, "%s: null pointer", who);
  FD_REQUIRE(Y || cy == 0.f, "%s: null pointer (Y with cy != 0)", who);
  FD_TRY(check_image(who, B, H, W, dtype));
  FD_REQUIRE(ks == 1 || ks == 3, "%s: ks must be 1 or 3 (got %d)", who, ks);
  if (cz != 0.f || z || seeds) FD_TRY(check_noise(who, z, seeds, draw));   // cz == 0: the plane is never read, none is needed
  FD_REQUIRE(!frame0 || seeds, "%s: frame0 needs seeds", who);
  fd_edge_args a;
  a.x = pyr; a.w = w; a.base = base; a.cb = cb; a.y = Y; a.cy = cy; a.coef = cn; a.z.ptr = z; a.z.seeds = seeds; a.z.draw = draw; a.z.frame0 = frame0;
  a.cz = cz; a.out = dst; a.B = B; a.H = H; a.W = W; a.ks = ks;
  return fd_edge_score_update(a, dtype, fd_stream(stream));
}

extern "C" int fd_op_score_update(const void* pyr, const float* w, const float* base, float cb, const float* Y, float cy, float cn,
                                  const float* z, const unsigned long long* seeds, int draw, float cz, float* dst, int B, int H, int W, int ks,
                                  int dtype, void* stream) {
  return op_score_update("fd_op_score_update", pyr, w, base, cb, Y, cy, cn, z, seeds, nullptr, draw, cz, dst, B, H, W, ks, dtype, stream);
}

// fd_op_score_update with the seeded plane at absolute frames: column t of image b is frame frame0[b] + t (DEVICE int32 [B]; NULL = zeros =
// fd_op_score_update, bit for bit; frame0 needs seeds)
extern "C" int fd_score_update_at(const void* pyr, const float* w, const float* base, float cb, const float* Y, float cy, float cn,
                                     const float* z, const unsigned long long* seeds, const int* frame0, int draw, float cz, float* dst, int B,
                                     int H, int W, int ks, int dtype, void* stream) {
  return op_score_update("fd_score_update_at", pyr, w, base, cb, Y, cy, cn, z, seeds, frame0, draw, cz, dst, B, H, W, ks, dtype, stream);
}

extern "C" int fd_score_update_clips(const void* pyr, const float* w, const float* base, const float* Y, const float* ctab, float* dst, int B, int H,
                                        int W, int ks, int dtype, void* stream) {
  // cy lives on the device, so Y is always required
  FD_REQUIRE(pyr && w && base && Y && ctab && dst, "fd_score_update_clips: null pointer");
  FD_TRY(check_image("fd_score_update_clips", B, H, W, dtype));
  FD_REQUIRE(B <= MAX_GRID_Y, "fd_score_update_clips: B must be in [1, 65535] (got %d)", B);
  FD_REQUIRE(ks == 1 || ks == 3, "fd_score_update_clips: ks must be 1 or 3 (got %d)", ks);
  fd_edge_args a;
  a.x = pyr; a.w = w; a.base = base; a.y = Y; a.ctab = ctab; a.out = dst; a.B = B; a.H = H; a.W = W; a.ks = ks;
  return fd_edge_score_update(a, dtype, fd_stream(stream));
}

extern "C" int fd_op_init_state(const float* Y, const float* noise, const unsigned long long* seeds, const int* frame0, int draw,
                                const double* sigma, int sigma_n, float sigma_fac, float* x0, int B, int F, int T, void* stream) {
  FD_REQUIRE(Y && sigma && x0, "fd_op_init_state: null pointer");
  FD_REQUIRE(B >= 1 && F >= 1 && T >= 1, "fd_op_init_state: bad shape (B=%d F=%d T=%d)", B, F, T);
  FD_REQUIRE(sigma_n == 1 || sigma_n == F, "fd_op_init_state: sigma_n must be 1 or F = %d (got %d)", F, sigma_n);
  FD_TRY(check_noise("fd_op_init_state", noise, seeds, draw));
  FD_REQUIRE(!frame0 || seeds, "fd_op_init_state: frame0 needs seeds");
  fd_noise_src src;
  src.ptr = noise; src.seeds = seeds; src.draw = draw; src.frame0 = frame0;
  return fd_init_state(Y, src, sigma, sigma_n, sigma_fac, x0, B, F, T, fd_stream(stream));
}

static int op_caxpy(const char* who, const float* a, const float* q, const unsigned long long* seeds, const int* frame0, int draw, float cq,
                    float* dst, int B, int F, int T, void* stream) {
  FD_REQUIRE(a && dst, "%s: null pointer", who);
  FD_REQUIRE(B >= 1 && F >= 1 && T >= 1, "%s: bad shape (B=%d F=%d T=%d)", who, B, F, T);
  FD_TRY(check_noise(who, q, seeds, draw));
  FD_REQUIRE(!frame0 || seeds, "%s: frame0 needs seeds", who);
  fd_noise_src src;
  src.ptr = q; src.seeds = seeds; src.draw = draw; src.frame0 = frame0;
  return fd_caxpy(a, src, cq, dst, B, F, T, fd_stream(stream));
}

extern "C" int fd_op_caxpy(const float* a, const float* q, const unsigned long long* seeds, int draw, float cq, float* dst, int B, int F, int T,
                           void* stream) {
  return op_caxpy("fd_op_caxpy", a, q, seeds, nullptr, draw, cq, dst, B, F, T, stream);
}

// fd_op_caxpy with the seeded plane at absolute frames frame0[b] + t (DEVICE int32 [B]; NULL = fd_op_caxpy, bit for bit; frame0 needs seeds)
extern "C" int fd_caxpy_at(const float* a, const float* q, const unsigned long long* seeds, const int* frame0, int draw, float cq, float* dst,
                              int B, int F, int T, void* stream) {
  return op_caxpy("fd_caxpy_at", a, q, seeds, frame0, draw, cq, dst, B, F, T, stream);
}

extern "C" int fd_op_ode_lincomb(const float* x, float cx, float dt, const float* const* k, const float* c, int nk, float* dst, long long n,
                                 void* stream) {
  FD_TRY(check_lincomb("fd_op_ode_lincomb", x, cx, k, c, nk, dst, n));
  return fd_ode_lincomb(x, cx, dt, k, c, nk, dst, n, fd_stream(stream));
}

extern "C" int fd_op_ode_lincomb_clips(const float* x, float cx, const float* dt_dev, const float* const* k, const float* c, int nk, float* dst,
                                       int B, long long n, void* stream) {
  FD_TRY(check_lincomb("fd_op_ode_lincomb_clips", x, cx, k, c, nk, dst, n));
  FD_REQUIRE(dt_dev, "fd_op_ode_lincomb_clips: null pointer (dt)");
  FD_REQUIRE(B >= 1 && B <= MAX_GRID_Y, "fd_op_ode_lincomb_clips: B must be in [1, 65535] (got %d)", B);
  return fd_ode_lincomb_clips(x, cx, dt_dev, k, c, nk, dst, B, n, fd_stream(stream));
}

extern "C" int fd_op_ode_scaled_sq(const float* p, const float* q, const float* r, const float* s, float atol, float rtol, double* partial,
                                   int nblocks, long long n, void* stream) {
  FD_TRY(check_scaled_sq("fd_op_ode_scaled_sq", p, r, s, partial, nblocks, n));
  return fd_ode_scaled_sq(p, q, r, s, atol, rtol, partial, nblocks, n, fd_stream(stream));
}

extern "C" int fd_op_ode_scaled_sq_clips(const float* p, const float* q, const float* r, const float* s, float atol, float rtol, double* partial,
                                         int nblocks, int B, long long n, void* stream) {
  FD_TRY(check_scaled_sq("fd_op_ode_scaled_sq_clips", p, r, s, partial, nblocks, n));
  FD_REQUIRE(B >= 1 && B <= MAX_GRID_Y, "fd_op_ode_scaled_sq_clips: B must be in [1, 65535] (got %d)", B);
  return fd_ode_scaled_sq_clips(p, q, r, s, atol, rtol, partial, nblocks, B, n, fd_stream(stream));
}

extern "C" int fd_op_ode_commit_clips(const int* accept, const int* ckpt, const float* x_new, const float* k6, float* x, float* k0, float* traj,
                                      int B, long long n, void* stream) {
  FD_REQUIRE(accept && ckpt && x_new && k6 && x && k0, "fd_op_ode_commit_clips: null pointer");
  FD_REQUIRE(B >= 1 && B <= MAX_GRID_Y, "fd_op_ode_commit_clips: B must be in [1, 65535] (got %d)", B);
  FD_REQUIRE(n >= 1, "fd_op_ode_commit_clips: bad element count n=%lld", n);
  return fd_ode_commit_clips(accept, ckpt, x_new, k6, x, k0, traj, B, n, fd_stream(stream));
}
