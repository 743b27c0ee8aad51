// ops_api.hip -- operator-level C ABI of the kernels between the network and the ODE / SDE solvers (include/flowdec_hip.h,
// "Operator-level: solver and edge kernels").  Every entry point checks its arguments and then calls the launcher the model and the
// solvers call (fd_edge_op, fd_init_state, fd_caxpy, fd_ode_*: internal.h).  No kernel and no launch configuration lives here, so a test
// of one of these functions is a test of the production launch.  A refused call launches nothing.
#include <limits.h>

#include "common.h"
#include "internal.h"

namespace {

constexpr int MAX_GRID_Y = 65535;

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

extern "C" int fd_op_pack_input(const float* x, const float* y, void* out8, int B, int H, int W, int dtype, void* stream) {
  FD_REQUIRE(x && y && out8, "fd_op_pack_input: null pointer");
  FD_TRY(check_image("fd_op_pack_input", B, H, W, dtype));
  fd_edge_args a;
  a.x = x; a.y = y; a.out = out8; a.B = B; a.H = H; a.W = W;
  return fd_edge_op(0, a, dtype, fd_stream(stream));
}

extern "C" int fd_op_combine(const void* p4, const float* w, const float* bias, const void* h, void* out, float* stats, int B, int H, int W,
                             int Cout, int dtype, void* stream) {
  FD_REQUIRE(p4 && w && bias && h && out && stats, "fd_op_combine: null pointer");
  FD_TRY(check_image("fd_op_combine", B, H, W, dtype));
  FD_REQUIRE(B <= MAX_GRID_Y, "fd_op_combine: B must be in [1, 65535] (got %d)", B);
  FD_REQUIRE(Cout >= 8 && Cout <= 256 && (Cout & (Cout - 1)) == 0, "fd_op_combine: Cout must be a power of two in [8, 256] (got %d)", Cout);
  fd_edge_args a;
  a.x = p4; a.w = w; a.bias = bias; a.y = h; a.out = out; a.stats = stats; a.B = B; a.H = H; a.W = W; a.Cout = Cout;
  return fd_edge_op(2, a, dtype, fd_stream(stream));
}

extern "C" int fd_op_output_update(const void* pyr, const float* w, const float* base, const float* kold, float coef, float* dst, float* ksave,
                                   int B, int H, int W, int ks, int dtype, void* stream) {
  FD_REQUIRE(pyr && w && dst, "fd_op_output_update: null pointer");
  FD_TRY(check_image("fd_op_output_update", B, H, W, dtype));
  FD_REQUIRE(ks == 1 || ks == 3, "fd_op_output_update: ks must be 1 or 3 (got %d)", ks);
  fd_edge_args a;
  a.x = pyr; a.w = w; a.base = base; a.kold = kold; a.coef = coef; a.out = dst; a.ksave = ksave; a.B = B; a.H = H; a.W = W; a.ks = ks;
  return fd_edge_op(3, a, dtype, fd_stream(stream));
}

extern "C" int fd_op_score_update(const void* pyr, const float* w, const float* base, float cb, const float* Y, float cy, float cn,
                                  const float* z, const unsigned long long* seeds, int draw, float cz, float* dst, int B, int H, int W, int ks,
                                  int dtype, void* stream) {
  FD_REQUIRE(pyr && w && base && dst, "fd_op_score_update: null pointer");
  FD_REQUIRE(Y || cy == 0.f, "fd_op_score_update: null pointer (Y with cy != 0)");
  FD_TRY(check_image("fd_op_score_update", B, H, W, dtype));
  FD_REQUIRE(ks == 1 || ks == 3, "fd_op_score_update: ks must be 1 or 3 (got %d)", ks);
  if (cz != 0.f || z || seeds) FD_TRY(check_noise("fd_op_score_update", z, seeds, draw));   // cz == 0: the plane is never read, none is needed
  fd_edge_args a;
  a.x = pyr; a.w = w; a.base = base; a.cb = cb; a.y = Y; a.cy = cy; a.coef = cn; a.z.ptr = z; a.z.seeds = seeds; a.z.draw = draw; a.cz = cz;
  a.out = dst; a.B = B; a.H = H; a.W = W; a.ks = ks;
  return fd_edge_op(4, a, dtype, fd_stream(stream));
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

extern "C" int fd_op_caxpy(const float* a, const float* q, const unsigned long long* seeds, int draw, float cq, float* dst, int B, int F, int T,
                           void* stream) {
  FD_REQUIRE(a && dst, "fd_op_caxpy: null pointer");
  FD_REQUIRE(B >= 1 && F >= 1 && T >= 1, "fd_op_caxpy: bad shape (B=%d F=%d T=%d)", B, F, T);
  FD_TRY(check_noise("fd_op_caxpy", q, seeds, draw));
  fd_noise_src src;
  src.ptr = q; src.seeds = seeds; src.draw = draw;
  return fd_caxpy(a, src, cq, dst, B, F, T, fd_stream(stream));
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
