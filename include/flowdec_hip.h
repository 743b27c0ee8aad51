/* flowdec_hip.h -- C ABI of libflowdec_hip.so: the MI355X (gfx950) drop-in for the FlowDec
 * inference hot path (FlowModel.enhance: STFT -> NCSN++ x NFE inside a fixed-step ODE loop ->
 * iSTFT).  Everything here is `extern "C"`, plain pointers and sizes; no torch types.
 *
 * Conventions
 *  - Every function returns 0 on success or a negative FD_E* code; fd_last_error() gives the
 *    message of the last failure on the calling thread.  The reference's native ops raise a C++
 *    exception -> Python RuntimeError (op/upfirdn2d.cpp:34-42); the Python binding in
 *    flowdec_amd/_lib.py turns a non-zero return into RuntimeError to keep that behaviour.
 *  - All data pointers are DEVICE pointers owned by the caller unless stated otherwise; nothing on
 *    the hot path allocates.  All work is enqueued asynchronously on `stream` (a hipStream_t passed
 *    as void*; NULL = default stream), no hidden synchronisation, graph-capture safe -- the same
 *    contract as the reference's launches on at::cuda::getCurrentCUDAStream (upfirdn2d_kernel.cu:224-226).
 *  - Activation tensors are NHWC ([B][H][W][C], H = frequency bins, W = time frames) in the storage
 *    type given by `dtype` (FD_F32 or FD_BF16).  Spectrogram / ODE-state tensors at the model boundary
 *    use the reference layout: complex64 [B][1][F=768][T] (interleaved re,im), float32 waveforms [B][L].
 *  - Threading.  The operator-level calls (fd_upfirdn2d, fd_fused_bias_act, fd_conv2d, fd_fir_resample, fd_gn_*, fd_stft_*, ...)
 *    keep no state and are re-entrant from any number of threads, like the reference's ops (upfirdn2d_kernel.cu:224-231).  An
 *    fd_model holds scratch that its enqueueing calls share (time-embedding biases, hipGraph cache, side stream, profiling events):
 *    it serves ONE enqueueing call at a time.  A second thread that enters fd_ncsnpp_forward / fd_ode_solve[_adaptive[_clips]] / fd_enhance /
 *    fd_score_* / fd_regression_enhance while another is inside gets FD_EBUSY (nothing is enqueued, nothing is corrupted); use one
 *    fd_model per thread for concurrent solves.  "Inside" is the host-side enqueue only -- the GPU work itself is asynchronous:
 *    consecutive calls of one model on DIFFERENT streams must be ordered by the caller (record an event after one call, make the
 *    next stream wait for it), because the workspace passed in and the model's own scratch (the per-step time-embedding biases)
 *    are reused from call to call.  The Python binding does both for its callers (flowdec_amd/model.py: _NativeCall).
 */
#ifndef FLOWDEC_HIP_H
#define FLOWDEC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FD_OK 0
#define FD_EINVAL (-1)   /* bad argument / unsupported shape */
#define FD_ERUNTIME (-2) /* HIP runtime error (message has hipGetErrorString) */
#define FD_ENOMEM (-3)   /* caller-provided workspace too small */
#define FD_ESTATE (-4)   /* model not finalised / parameter missing */
#define FD_EBUSY (-5)    /* the fd_model is inside an enqueueing call of another thread (see "Threading" below) */

#define FD_F32 0
#define FD_BF16 1
/* Algorithm flag, OR-ed into the `dtype` / `wdtype` / `act_dtype` arguments that select a convolution (storage type =
 * value & 0xff): 3x3 convolutions with Cout % 128 == 0 and all channel counts % 32 == 0 run as Winograd F(2,3) along W
 * (1.5x fewer MFMAs; bf16 storage, fp16 MFMA operands, f32 accumulation; conv_wino.hip).  The packed weights of the two
 * algorithms differ: pack and launch with the same flag.  Both Winograd packings scale every output channel's transformed weights
 * (and its folded shortcut weights) by a power of two before the fp16 rounding and carry the inverse table behind the packed steps;
 * the kernels undo it exactly in the epilogue -- weights of any magnitude (1e-6 .. 1e2 tested, per channel) keep their mantissa. */
#define FD_WINOGRAD 0x100
/* Same places as FD_WINOGRAD: 3x3 convolutions with Cout == 256, all channel counts % 32 == 0 and whole 16 x 16 pixel tiles
 * (H % 16 == W % 16 == 0) as Winograd F(4,3) along W -- HALF the MFMAs of the direct kernel; 256-cout workgroups with the input
 * transform done once per workgroup when the activated halo is stored (conv_wino4.hip).  bf16 storage, fp16 MFMA operands, f32
 * accumulation; 3x3 inputs, raw or activated, saturate at +-6000 in their fp16 form (a folded shortcut input never passes through
 * fp16).  Pack and launch with the same flag. */
#define FD_WINOGRAD4 0x80000
/* fd_conv2d with FD_WINOGRAD4 only: walk the pixel tiles in DESCENDING order.  Same result, bit for bit; a consumer that starts where
 * its producer stopped finds the producer's last output lines still in the memory-side cache (the model alternates the direction from
 * one F(4,3) launch to the next: 0.5 % of a cfg 2 step). */
/* fd_conv_pack_weights / fd_conv2d with FD_F32 storage: 2-D Winograd F(4x4, 3x3) in exact float32 (conv_wino44f.hip: 2.25 multiply-adds per
 * output and input channel instead of 9; Cout % 128 == 0, channel counts % 8 == 0, H % 16 == W % 16 == 0; folded shortcut and residual
 * input allowed together).  The fp32 mode's kernel (`FD_F32 | FD_WINOGRAD_AUTO`). */
#define FD_WINOGRAD44 0x200000
#define FD_TILE_REVERSED 0x100000
/* fd_model_config.act_dtype only: Winograd for the blocks of resolution level >= 2 (small grids, where its 128-cout workgroups
 * fill the chip better), direct MFMA convolution elsewhere. */
#define FD_WINOGRAD_LOWRES 0x200
/* fd_model_config.act_dtype only: all packings are kept and every launch picks its kernel by the image size: the direct kernel with
 * FD_TILE_BN64_CHUNK for images of at most 16 tiles of 16 x 16 pixels, Winograd F(2,3) up to 96 tiles (the low-resolution levels;
 * not with a folded 1x1 shortcut), Winograd F(4,3) for every other 3x3 convolution with 256 output channels and whole tiles (every
 * other such launch of a forward with FD_TILE_REVERSED), direct for the rest.  Independent of the batch size, so that a clip gives the
 * same bits alone and inside any batch. */
#define FD_WINOGRAD_AUTO 0x400
/* fd_conv_pack_weights / fd_conv2d / fd_model_config.act_dtype, with FD_F32 only: "bf16 operands, f32 residual stream" -- activations,
 * skip tensors and outputs stay f32 in memory; a convolution rounds its (activated) input to bf16 at the LDS store, its weights are
 * packed as bf16, accumulation is f32.  Direct kernel, default workgroup widths. */
#define FD_BF16_OPERANDS 0x10000
/* same places, with FD_F32 only: every conv operand as the two-term bf16 split x = hi + lo (16 mantissa bits) and every product as
 * hi*hi + hi*lo + lo*hi on the bf16 matrix cores, f32 accumulation -- results within the f32 mode's tolerances (a conv is ~1e-5 from
 * the f64 convolution) at 3x the bf16 MFMA work instead of the f32 MFMA's 16x. */
#define FD_BF16X3_OPERANDS 0x20000
/* fd_conv2d only (direct kernel): output channels per workgroup, 32 / 64 / 128 instead of the default min(256, padded Cout).  Narrow
 * workgroups put a SMALL image on more compute units (latency) at the price of re-activating the input once per workgroup
 * (throughput).  The convolution result is bit-identical for every width (same K order per output); the per-tile statistics
 * differ in summation order only. */
#define FD_TILE_BN32 0x1000
#define FD_TILE_BN64 0x2000
#define FD_TILE_BN128 0x3000
#define FD_TILE_BN64_CHUNK 0x4000 /* 64 + the weight slabs of two whole 32-channel chunks resident in LDS: one barrier and one memory
                                     round trip per chunk instead of per tap pair (bf16; falls back to FD_TILE_BN64 otherwise) */
#define FD_TILE_BN32_CHUNK 0x5000 /* same with 32-channel workgroups (4 waves) */
#define FD_TILE_DUO128 0x6000 /* 4 waves x (128 px x 64 cout) with ONE halo buffer: 70 KiB of LDS, two workgroups per CU (bf16, Cout % 128 == 0) */
#define FD_TILE_PERSIST 0x7000 /* "register epilogue, continuous tiles" (bf16, Cout == 128 or 256, H % 16 == W % 16 == 0, no residual input; the
                                  default configuration otherwise): one persistent workgroup per compute unit walks a contiguous range of tiles
                                  as ONE software pipeline, epilogue on the accumulator registers, stores left in flight.  Bit-identical
                                  convolution result.  Measured (profiles/r03_register_epilogue.txt): no prologue, 12 % fewer instructions
                                  around the MFMAs -- and 0.97-1.06x of the default: the K loop loses what the tile boundary gains.  Opt-in. */
#define FD_TILE_MASK 0xf000
/* fd_model_config.act_dtype only: low-latency schedule for ONE short clip -- both packings are kept (as with FD_WINOGRAD_AUTO) and
 * every convolution picks kernel and workgroup width by its IMAGE size (never by the batch size): FD_TILE_BN32_CHUNK for images of
 * at most 24 tiles, Winograd F(2,3) up to 128 tiles (unless a 1x1 shortcut is folded in: direct with FD_TILE_BN128 workgroups there),
 * Winograd F(4,3) above 128 tiles. */
#define FD_LOW_LATENCY 0x800
/* fd_model_config.act_dtype only: keep the side branches of a network evaluation (time embedding, pyramid-head chain) on the caller's
 * stream instead of forking them onto the model's second stream (default: forked; inside a graph capture they become parallel
 * branches of the graph).  Results are bit-identical either way. */
#define FD_NO_SIDE_STREAM 0x40000

/* solver ids (flowdec/model.py:487 'euler'/'midpoint' via torchdyn; sampling/solvers.py:15-57) */
#define FD_SOLVER_EULER 0
#define FD_SOLVER_MIDPOINT 1
#define FD_SOLVER_HEUN2 2
#define FD_SOLVER_HEUN2_EULERLAST 3

const char* fd_last_error(void);
int fd_version(void);
/* Box calibration (bench.py `box_calibration`): `repeats` timed launches of a fixed matrix-core issue loop (register-resident random
 * bf16 operands, no LDS, no memory; iters <= 0: 100000 iterations, ~50 ms per launch) on `stream`; *tflops = the mean rate the box
 * sustains at its power-limited clock, *ms_total (optional) the time of the timed launches.  scratch: 2 KiB of device memory.
 * Synchronises the stream.  No counterpart in the reference (enhance.py:120-136 times one call with two events). */
int fd_calibrate_mfma(float* scratch, int iters, int repeats, double* tflops, double* ms_total, void* stream);
/* Device properties the bench reports: [0]=CU count, [1]=max clock kHz, [2]=wavefront size, [3]=gfx arch number. */
int fd_device_info(int* out4);

/* ------------------------------------------------------------------------------------------------
 * Native-operator parity (the reference's only FFI)
 * ---------------------------------------------------------------------------------------------- */

/* Replaces upfirdn2d_op.upfirdn2d(input[major,in_h,in_w,minor], kernel[kh,kw], up_x,up_y,down_x,down_y,
 * pad_x0,pad_x1,pad_y0,pad_y1) -> out[major,out_h,out_w,minor]
 * (op/upfirdn2d.cpp:38-49; kernel upfirdn2d_kernel.cu:118-218; out_h/out_w formula :248-251).
 * `kernel` is float32 on device.  `out` must hold major*out_h*out_w*minor elements. */
int fd_upfirdn2d(const void* input, const float* kernel, void* out, int major, int in_h, int in_w, int minor,
                 int kernel_h, int kernel_w, int up_x, int up_y, int down_x, int down_y, int pad_x0, int pad_x1,
                 int pad_y0, int pad_y1, int dtype, void* stream);
int fd_upfirdn2d_out_size(int in_size, int up, int down, int pad0, int pad1, int ksize);

/* Replaces fused_bias_act(input, bias, refer, act, grad, alpha, scale) for grad == 0
 * (op/fused_bias_act.cpp:37-46; kernel fused_bias_act_kernel.cu:30-61):
 * out[i] = scale * act(x[i] + bias[(i / step_b) % size_b]); act 1 = linear, 3 = leaky-relu(alpha).
 * bias may be NULL (size_b == 0).  float32 only (dead code on the hot path; kept for API parity). */
int fd_fused_bias_act(const float* x, const float* bias, float* out, long long n, int step_b, int size_b, int act,
                      float alpha, float scale, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Hot-path building blocks (NHWC activations)
 * ---------------------------------------------------------------------------------------------- */

/* StyleGAN2 FIR [1,3,3,1] x2 resampling in polyphase form (upsample_2d / downsample_2d,
 * up_or_down_sampling.py:220-282) on an NHWC tensor.  If `affine` != NULL ([B][C] pairs (a,d)) a second
 * output out_act = FIR(silu(a*x+d)) is produced from the same read (the resample of
 * h = act(GroupNorm_0(x)) and of x in ResnetBlockBigGANpp.forward, layerspp.py:255-267).
 * direction: +1 = up x2, -1 = down x2.  Either output may be NULL. */
int fd_fir_resample(const void* x, const float* affine, void* out_raw, void* out_act, int B, int H, int W, int C,
                    int direction, int dtype, void* stream);
/* Which kernel fd_fir_resample launches for a call (host only, no GPU needed; for tests): the same rule the launch itself goes through.
 * has_affine / want_raw / want_act = whether `affine` / `out_raw` / `out_act` would be non-NULL.  Returns FD_EINVAL where fd_fir_resample
 * refuses the call, else the decimal code  F RR C V A S:
 *   F  = family: FD_FIR_UP (fir_up_kernel: one thread = RR input rows x C input columns), FD_FIR_DOWN (fir_down_kernel: one thread = a
 *        block of RR x C output pixels), FD_FIR_DOWN_MARCH (fir_down_march_kernel: one thread marches down a strip of RR output rows x C
 *        columns);
 *   RR, C = rows (01 .. 16) and columns (1 .. 4) per thread;  V = channels per thread (4 or 8);
 *   A  = 1 if the kernel evaluates silu(a*x + d) (an affine is present);  S = 1 for the form with unconditional stores (every strip and
 *        column block whole, both outputs present).
 * e.g. 2164411 = marching strips of 16 rows x 4 columns, 4 channels, activated, unconditional stores; 11800 = plain 1 x 1 down-sampling
 * on 8-channel vectors. */
#define FD_FIR_UP 0
#define FD_FIR_DOWN 1
#define FD_FIR_DOWN_MARCH 2
int fd_fir_variant(int B, int H, int W, int C, int direction, int dtype, int has_affine, int want_raw, int want_act);

/* The input convolution of NCSN++ (all_modules.3 = conv3x3(4, nf), ncsnpp.py:291 via layers.py:128-134) on the packed NHWC input
 * [B][H][W][8] (channels 0..3 = x.re, x.im, y.re, y.im; 4..7 ignored), zero padding, as f32 vector FMAs (taps ascending, input channels
 * ascending, one fma each), with the GroupNorm partial sums of the output: stats[B][(H / 16) * (W / 16)][Cout][2] = per 16 x 16 pixel
 * tile (sum x, sum x^2) of the f32 values.  w = [Cout][4][3][3] float32 (the checkpoint's layout), Cout in {8, 16, 32, 64, 128},
 * H % 16 == W % 16 == 0.  dtype = storage type of `in8` and `out`. */
int fd_conv_in(const void* in8, const float* w, const float* bias, void* out, float* stats, int B, int H, int W, int Cout, int dtype,
               void* stream);

/* GroupNorm statistics (nn.GroupNorm(min(C//4,32), C, eps=1e-6), layerspp.py:229,241), split in two so that one
 * statistics pass can be shared by consumers that group the channels differently:
 *  partial sums  : part[b][tile][stride][2] = per-channel (sum x, sum x^2) of one spatial tile, float32.  Produced
 *                  either by fd_channel_sums (stand-alone pass; tiles = fd_channel_sums_tiles(H, W), stride = C) or by
 *                  fd_conv2d for its OUTPUT (tiles = fd_conv_stats_tiles(H, W), stride = fd_conv_cout_pad(Cout)).
 *  fd_gn_finalize: reduce the partials of one or two tensors (virtual channel concat [C0 | C1], ncsnpp.py:337) in
 *                  float64 and emit per-(b,c) affine pairs a = rstd*gamma[c], d = beta[c] - mean*rstd*gamma[c]. */
int fd_channel_sums_tiles(int H, int W);
int fd_channel_sums(const void* x, float* part, int B, int H, int W, int C, int dtype, void* stream);
int fd_gn_finalize(const float* part0, int tiles0, int stride0, int C0, const float* part1, int tiles1, int stride1, int C1,
                   const float* gamma, const float* beta, float* affine, int B, int groups, long long hw, float eps,
                   void* stream);

/* Packs PyTorch conv weights [Cout][Cin][k][k] float32 (device) into the MFMA layout [step][CoutPad][64 B]
 * (bf16: 32 channels, f32: 16 channels per row, the four 16-byte columns XOR-swizzled by (cout >> 2) & 3;
 * step = (concat segment, channel chunk, tap)).  Input channels
 * are split at C0 into two chunk-padded segments (virtual concat).  `w_sc` (optional, [Cout][S0+S1][1][1]) is the
 * 1x1 shortcut conv of a ResnetBlock (Conv_2, layerspp.py:244-245) whose K steps are appended so that one launch
 * computes Conv_1(h) + Conv_2(x). */
long long fd_conv_packed_bytes(int Cout, int C0, int C1, int ksize, int S0, int S1, int wdtype);
int fd_conv_pack_weights(const float* w, const float* w_sc, void* packed, int Cout, int C0, int C1, int ksize, int S0, int S1,
                         int wdtype, void* stream);
int fd_conv_cout_pad(int Cout);          /* row count of a packed slab / channel stride of the stats partials */
int fd_conv_stats_tiles(int H, int W);   /* 16x16 tiles per image */

/* Implicit-GEMM convolution, stride 1, 'same' zero padding, ksize 3 or 1 (ddpm_conv3x3 / ddpm_conv1x1,
 * layers.py:110-134) on MFMA:
 *   out = scale * ( conv_k( act([in0 | in1]) ) + conv_1x1([sc0 | sc1]) + bias[b] + skip )
 * act(x) = silu(a*x+d) per (b,c) if `affine` != NULL (GroupNorm+SiLU folded into the operand load), identity otherwise;
 * [in0|in1] / [sc0|sc1] are virtual channel concats (second tensors optional); bias: [bias_rows][Cout] float32 with
 * bias_rows in {1, B} (conv bias + Dense_0(act(temb)), layerspp.py:272-273); skip: optional NHWC tensor of Cout
 * channels ((x+h)/sqrt(2), layerspp.py:281-284); stats: optional partial sums of the output (see above).
 * dtype selects storage AND arithmetic: FD_BF16 = bf16 operands / f32 accumulate (v_mfma_f32_32x32x16_bf16),
 * FD_F32 = exact f32 (v_mfma_f32_32x32x2_f32).  Input channel counts must be multiples of 8, Cout 4 or a multiple of 8. */
int fd_conv2d(const void* in0, int C0, const void* in1, int C1, const float* affine, const void* sc0, int S0, const void* sc1,
              int S1, const void* packed_w, const float* bias, int bias_rows, const void* skip, float scale, void* out,
              int Cout, float* stats, int B, int H, int W, int ksize, int dtype, void* stream);

/* Which kernel fd_conv2d launched: one process-wide cumulative counter per kernel family, incremented (relaxed atomics) when a call
 * has passed its argument checks and enqueued its launch.  DIRECT = conv_mfma.hip in bf16 or f32 storage (every FD_TILE_* width),
 * DIRECT_MIXED / DIRECT_SPLIT = the same kernel with FD_BF16_OPERANDS / FD_BF16X3_OPERANDS, WINO = F(2,3), WINO4 = F(4,3) bf16,
 * WINO4F = F(4,3) f32, WINO44F = F(4x4, 3x3) f32, HEAD / HEADF = the Cout = 4 pyramid-head kernels (conv_head.hip / conv_headf.hip).
 * The counters count HOST dispatches: a launch recorded into a captured graph is counted once, at capture; replays of the graph are
 * not counted.  The model's planning walks (workspace sizing) never call fd_conv2d and count nothing.  There is no reset: read the
 * counters before and after and take the difference.  Writes min(n, FD_CONV_KERNEL_COUNT) counters to `counts` (host memory) and
 * returns FD_CONV_KERNEL_COUNT. */
enum { FD_CONV_KERNEL_DIRECT, FD_CONV_KERNEL_DIRECT_MIXED, FD_CONV_KERNEL_DIRECT_SPLIT, FD_CONV_KERNEL_WINO,
       FD_CONV_KERNEL_WINO4, FD_CONV_KERNEL_WINO4F, FD_CONV_KERNEL_WINO44F, FD_CONV_KERNEL_HEAD,
       FD_CONV_KERNEL_HEADF, FD_CONV_KERNEL_COUNT };
int fd_conv_kernel_counts(long long* counts, int n);

/* Time embedding: GaussianFourierProjection -> Linear -> SiLU -> Linear (ncsnpp.py:263-274,
 * layerspp.py:42-51); t [nt] float32 -> temb [nt][4*nf].  gfp_w [nf], w1 [4nf][2nf], w2 [4nf][4nf] row-major.  FD_EINVAL (nothing
 * launched) for a null pointer, nt < 1, nf odd or < 2 (weight rows are read as 4-float vectors), 6 nf floats above the 64 KiB of shared
 * memory the launch may ask for, and w1 / w2 not 16-byte aligned. */
int fd_time_embedding(const float* t, int nt, const float* gfp_w, int nf, const float* w1, const float* b1,
                      const float* w2, const float* b2, float* temb, void* stream);
/* out[r][o] = conv_bias[o] + dense_b[o] + sum_k dense_w[o][k] * silu(temb[r][k])  (layerspp.py:272-273); conv_bias NULL = no conv
 * bias.  FD_EINVAL (nothing launched) for a null pointer, nt < 1, Cout < 1, temb_dim < 4 or not a multiple of 4, temb_dim floats above
 * 64 KiB of shared memory, and dense_w not 16-byte aligned. */
int fd_temb_bias(const float* temb, int nt, int temb_dim, const float* dense_w, const float* dense_b,
                 const float* conv_bias, int Cout, float* out, void* stream);

/* silu(a*x + d) with per-(b,c) affine pairs = act(GroupNorm(x)) as a stand-alone pass (layerspp.py:253,274); on the hot
 * path this is fused into the consumer's operand load, the entry point exists for operator-level parity. */
int fd_gn_silu_apply(const void* x, const float* affine, void* out, int B, long long hw, int C, int dtype, void* stream);

/* One ResnetBlockBigGANpp.forward (layerspp.py:252-284): GroupNorm_0 + SiLU [+ FIR up/down of h and x] -> Conv_0 + time
 * bias -> GroupNorm_1 + SiLU -> Conv_1 [+ Conv_2(x) folded in] (+ x) -> / sqrt(2), as the launches the model uses
 * (2 convs, 2 finalize, optional FIR).  x0 / x1 = NHWC input (virtual concat), out = NHWC [B][H'][W'][cout].
 *   w0    = fd_conv_pack_weights(Conv_0.weight, NULL, cout, cin0, cin1, 3, 0, 0)  (up/down blocks: cin1 = 0)
 *   w1    = fd_conv_pack_weights(Conv_1.weight, Conv_2.weight or NULL, cout, cout, 0, 3, S0, S1) with (S0, S1) = the input
 *           split (cin0, cin1) when has_conv2 -- the shortcut conv runs as extra K steps on x (resampled for up/down)
 *   bias0 = [bias0_rows][cout] from fd_temb_bias (Conv_0.bias + Dense_0(silu(temb))),  bias1 = Conv_1.bias (+ Conv_2.bias) */
typedef struct fd_resblock_desc {
  int cin0, cin1, cout, up, down, has_conv2;
  const float *gn0_gamma, *gn0_beta, *gn1_gamma, *gn1_beta;
  const void* w0; const float* bias0; int bias0_rows;
  const void* w1; const float* bias1;
} fd_resblock_desc;
size_t fd_resblock_workspace_bytes(const fd_resblock_desc* d, int B, int H, int W, int dtype);
int fd_resblock(const fd_resblock_desc* d, const void* x0, const void* x1, void* out, int B, int H, int W, int dtype, void* ws,
                size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Operator-level: solver and edge kernels
 * ----------------------------------------------------------------------------------------------
 * The kernels between the network and the ODE / SDE solvers, one entry point each, for operator-level parity.  Every fd_op_* function
 * checks its arguments (FD_EINVAL with a message, nothing launched) and then calls the launcher the model and the solvers themselves
 * call: the same kernel, grid and block.  "complex" = complex64 as interleaved float pairs; all pointers are DEVICE memory unless marked
 * HOST; dtype (FD_BF16 / FD_F32) = storage type of the NHWC tensors; float32 arithmetic throughout; one element per thread, grid-stride
 * beyond 8192 blocks x 256 threads.  Formulas give the operations per component; a product-sum may be one fused multiply-add. */

/* cat(x.re, x.im, y.re, y.im) -> out8 [B][H][W][8] (8-CHANNEL STRIDE: channels 0..3 = the values, rounded to dtype; 4..7 = 0, the
 * padding the matrix-core convs need).  x, y: complex [B][H][W]. */
int fd_op_pack_input(const float* x, const float* y, void* out8, int B, int H, int W, int dtype, void* stream);
/* Combine 'sum' (layerspp.py:54-69): out[b][p][c] = ((((bias[c] + w[c][0] p4[0]) + w[c][1] p4[1]) + w[c][2] p4[2]) + w[c][3] p4[3]) +
 * h[b][p][c], each product-sum one fma, stored as dtype.  p4 = [B][H][W][8] (the 4-channel pyramid in the 8-channel stride of
 * fd_op_pack_input; channels 4..7 are not read), w = [Cout][4] float32, bias = [Cout] float32, h and out = [B][H][W][Cout].
 * stats = [B][tiles][Cout][2] float32 with tiles = ceil(H W / 256): per-channel (sum, sum of squares) over the 256 consecutive pixels
 * [256 tile, 256 tile + 256) of the image, taken from the values AS STORED (after rounding to dtype), the format fd_gn_finalize reads.
 * Cout: a power of two in [8, 256]; 1 <= B <= 65535. */
int fd_op_combine(const void* p4, const float* w, const float* bias, const void* h, void* out, float* stats, int B, int H, int W, int Cout,
                  int dtype, void* stream);
/* The output layer fused with a fixed-step solver's state update.  v = conv(pyr) as complex (channel 0 = re, 1 = im), no bias:
 *   ks = 1: w = [2][4];        v[o] = fma(w[o][3], p[3], fma(w[o][2], p[2], fma(w[o][1], p[1], w[o][0] p[0])))
 *   ks = 3: w = [2][4][3][3];  zero padding 'same' within each of the B images; taps ascending (dy, dx), input channels ascending per tap,
 *           one fma each, from 0.
 *   ksave = v (if non-NULL);  dst = base + coef * (v + kold)   (kold, base: NULL = that term is absent).
 * pyr = [B][H][W][4] in dtype (4-CHANNEL STRIDE: the pyramid head's output); base, kold, dst, ksave: complex [B][H][W]. */
int fd_op_output_update(const void* pyr, const float* w, const float* base, const float* kold, float coef, float* dst, float* ksave, int B,
                        int H, int W, int ks, int dtype, void* stream);
/* The output layer fused with a predictor / corrector update of the score sampler:
 *   dst = fma(cz, z, fma(cy, Y, fma(cn, v, cb * base)))     (v, pyr, w, ks as above)
 * The Y term is skipped when cy == 0 (Y is not read and may be NULL), the z term when cz == 0 (no noise is read or generated; z and seeds
 * may both be NULL).  Otherwise exactly one of z (complex [B][H][W]) and seeds (uint64 [B]: z = the plane (seeds[b], draw) of "Seeded
 * noise" below with F = H, T = W, generated in registers) must be given. */
int fd_op_score_update(const void* pyr, const float* w, const float* base, float cb, const float* Y, float cy, float cn, const float* z,
                       const unsigned long long* seeds, int draw, float cz, float* dst, int B, int H, int W, int ks, int dtype, void* stream);
/* fd_op_score_update with the seeded plane at absolute frames: column t of image b is frame frame0[b] + t (frame0 = DEVICE int32 [B], or
 * NULL = zeros: fd_op_score_update, bit for bit; frame0 needs seeds).  With cz == 0 neither seeds nor frame0 is read. */
int fd_score_update_at(const void* pyr, const float* w, const float* base, float cb, const float* Y, float cy, float cn, const float* z,
                          const unsigned long long* seeds, const int* frame0, int draw, float cz, float* dst, int B, int H, int W, int ks,
                          int dtype, void* stream);
/* fd_op_score_update with one time per clip and no noise term (the right-hand side of fd_score_ode_solve under per-clip step control):
 *   dst[b] = fma(cy_b, Y[b], fma(cn_b, v[b], cb_b * base[b])),  (cb_b, cy_b, cn_b) = ctab[b][0..2]   (ctab: DEVICE float [B][3])
 * The Y term of a clip is skipped when its cy_b == 0; cy lives on the device, so Y is always required.  Image b equals
 * fd_op_score_update(cb_b, cy_b, cn_b, cz = 0) on that image alone, bit for bit.  B <= 65535. */
int fd_score_update_clips(const void* pyr, const float* w, const float* base, const float* Y, const float* ctab, float* dst, int B, int H,
                             int W, int ks, int dtype, void* stream);
/* x0 = Y + sigma_fac * nx,  nx = (float)(sigma[f] * (double)z)   (sigma = float64 [sigma_n], sigma_n = 1: one value for every f, or F).
 * Y, x0: complex [B][F][T].  Exactly one of noise (complex [B][F][T]) and seeds (uint64 [B]; z = plane (seeds[b], draw) at the absolute
 * frames frame0[b] + t, frame0 = int32 [B] or NULL = zeros; frame0 needs seeds). */
int fd_op_init_state(const float* Y, const float* noise, const unsigned long long* seeds, const int* frame0, int draw, const double* sigma,
                     int sigma_n, float sigma_fac, float* x0, int B, int F, int T, void* stream);
/* dst = fma(cq, q, a): a, dst complex [B][F][T]; exactly one of q (complex [B][F][T]) and seeds (uint64 [B], plane (seeds[b], draw)). */
int fd_op_caxpy(const float* a, const float* q, const unsigned long long* seeds, int draw, float cq, float* dst, int B, int F, int T,
                void* stream);
/* fd_op_caxpy with the seeded plane at the absolute frames frame0[b] + t (frame0 = DEVICE int32 [B], or NULL = zeros: fd_op_caxpy, bit for
 * bit; frame0 needs seeds). */
int fd_caxpy_at(const float* a, const float* q, const unsigned long long* seeds, const int* frame0, int draw, float cq, float* dst, int B,
                   int F, int T, void* stream);
/* Adaptive solvers.  n = complex elements of the state (fd_op_ode_lincomb, fd_op_ode_scaled_sq) or of ONE clip of a [B][n] state (the
 * *_clips forms, 1 <= B <= 65535: one grid row per clip).
 * dst = fma(cx, x, dt * s),  s = fma(c[m-1], k[m-1], ... fma(c[0], k[0], 0))  over the m terms kept: k, c = HOST arrays of nk <= 7 device
 * pointers / coefficients, a term with k[j] == NULL or c[j] == 0 is dropped before the launch (its buffer is never read); with cx == 0,
 * x is not read (may be NULL).  *_clips: clip b uses dt[b] (DEVICE float [B]) and equals fd_op_ode_lincomb on clip b alone, bit for bit. */
int fd_op_ode_lincomb(const float* x, float cx, float dt, const float* const* k, const float* c, int nk, float* dst, long long n, void* stream);
int fd_op_ode_lincomb_clips(const float* x, float cx, const float* dt, const float* const* k, const float* c, int nk, float* dst, int B,
                            long long n, void* stream);
/* Block partials of the Hairer error norm: partial[nblocks] (float64), their sum = sum_i |p_i - q_i|^2 / (atol + rtol max(|r_i|, |s_i|))^2
 * (complex moduli; q may be NULL = 0).  Every term is formed in float32 and accumulated in float64; block j owns the elements i = j 256 +
 * thread (mod nblocks 256); a block that owns no element writes 0.  *_clips: partial[B][nblocks], row b = the partials of
 * fd_op_ode_scaled_sq on clip b alone, bit for bit.  nblocks >= 1 (the solvers use 512). */
int fd_op_ode_scaled_sq(const float* p, const float* q, const float* r, const float* s, float atol, float rtol, double* partial, int nblocks,
                        long long n, void* stream);
int fd_op_ode_scaled_sq_clips(const float* p, const float* q, const float* r, const float* s, float atol, float rtol, double* partial,
                              int nblocks, int B, long long n, void* stream);
/* Masked commit of an attempted step: for every clip b with accept[b] != 0 (int32 [B]): x[b] = x_new[b], k0[b] = k6[b], and, where
 * ckpt[b] > 0 (int32 [B]) and traj != NULL, traj[ckpt[b]][b] = x_new[b]   (traj = complex [ckpt][B][n]).  Nothing else is written. */
int fd_op_ode_commit_clips(const int* accept, const int* ckpt, const float* x_new, const float* k6, float* x, float* k0, float* traj, int B,
                           long long n, void* stream);

/* Time conditioning (csrc/net_edges.hip: time_embedding_kernel, temb_bias_kernel), through the launchers fd_ncsnpp_forward calls.
 * fd_op_time_embedding = fd_time_embedding with the scalar-time path of the fixed-step solvers: t == NULL takes the time of every row
 * from t_imm (passed by value, no device read); with t != NULL, t_imm is ignored.  Row r:
 *   xp = ((t[r] * gfp_w[j]) * 2) * pi_f32 (three float32 roundings), emb = (sinf(xp) [nf], cosf(xp) [nf]),
 *   hid[o] = silu(fma chain over k ascending of w1[o][k] emb[k], from b1[o]),  temb[r][o] = the same chain of w2[o][k] hid[k] from b2[o].
 * Refusals as fd_time_embedding (t may be NULL). */
int fd_op_time_embedding(const float* t, float t_imm, int nt, const float* gfp_w, int nf, const float* w1, const float* b1, const float* w2,
                         const float* b2, float* temb, void* stream);
/* The batched table of every ResBlock's time bias in one launch (grid = jobs x rows), as the model runs it: for job j, row r
 *   out[j][r][o] = (fma chain over k ascending of dense_w[j][o][k] * silu(temb[r][k]), from dense_b[j][o]) + conv_b[j][o],  o < cout[j],
 * bit-identical to fd_temb_bias on job j alone.  dense_w, dense_b, conv_b, out, cout: HOST arrays of njobs device pointers / channel counts;
 * out[j] = [nt][cout[j]].  The entry builds the device job table, launches and SYNCHRONISES the stream before it releases the table: a
 * synchronous entry point for tests (the model keeps its table for its lifetime).  Refusals as fd_temb_bias per job, and: njobs < 1 or
 * above 2^24 - 1 (grid x of 256-thread blocks), nt > 65535 (grid y), a NULL conv_b[j] (this kernel reads it unconditionally; only
 * fd_temb_bias takes NULL as "no conv bias"). */
int fd_op_temb_bias_jobs(const float* temb, int nt, int temb_dim, const float* const* dense_w, const float* const* dense_b,
                         const float* const* conv_b, float* const* out, const int* cout, int njobs, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Front / back end
 * ---------------------------------------------------------------------------------------------- */

/* normalize_noisy('noisy') + torch.stft(n_fft, hop, sym-Hann, center/reflect, onesided) + amplitude
 * compression beta*|X|^alpha*e^{j angle X} + zero pad of the frame axis to T_pad
 * (util/other.py:55-82, feature_extractors.py:86-96,118-128, util/other.py:25-52).
 * y [B][L] f32 -> Y [B][1][n_fft/2+1][T_pad] complex64, normfac [B] f32.
 * ws: fd_stft_workspace_bytes(B, L, n_fft, hop) bytes of scratch. */
/* The DFT matrices / window envelope of one (n_fft, hop) live in a plan the CALLER owns (2 x 9.4 MB on the current device for
 * n_fft = 1534): fd_stft_plan_create allocates and uploads (synchronous, init time), the transforms themselves allocate
 * nothing and keep no state. */
typedef struct fd_stft_plan fd_stft_plan;
int fd_stft_plan_create(int n_fft, int hop, fd_stft_plan** out);
void fd_stft_plan_destroy(fd_stft_plan* plan);
size_t fd_stft_workspace_bytes(int B, int L, int n_fft, int hop);
/* normalize != 0: per-clip max-abs normalisation (normalize_mode 'noisy'); 0: normfac = 1 (normalize_mode 'none', util/other.py:70) */
int fd_stft_compress(const fd_stft_plan* plan, const float* y, int B, int L, float alpha, float beta, int normalize,
                     float* normfac, float* Y, int T_pad, void* ws, size_t ws_bytes, void* stream);
/* Inverse: slice [:T] -> X/beta -> |.|^(1/alpha) -> torch.istft(length=L) -> * normfac
 * (model.py:165-190, feature_extractors.py:98-109,130-139).  normfac may be NULL. */
int fd_decompress_istft(const fd_stft_plan* plan, const float* X, int B, int T, int T_pad, float alpha, float beta,
                        const float* normfac, float* y, int L, void* ws, size_t ws_bytes, void* stream);
/* Ragged batches (round 6).  The reference's driver enhances a directory FILE BY FILE, every file its own length (enhance.py:96-137,
 * model.py:129-163,476-528).  These variants take the files whose spectrograms pad to the same T_pad (util/other.py:25-52) as ONE
 * batch: y / the output are [B][L] rows with L = the longest clip, `lengths` (DEVICE int32 [B], n_fft/2 < lengths[b] <= L) the clips'
 * own sample counts.  Clip b gets exactly the arithmetic of a call with that clip alone: reflect padding at ITS end, its own
 * 1 + lengths[b]/hop frames (the rest zero, as pad_spec would leave them), torch.istft(length = lengths[b]) with its own overlap-add
 * envelope -- the result is bit-identical to the one-clip call; samples [lengths[b], L) of an output row are zero.  The caller
 * guarantees fd_padded_frames(fd_num_frames(lengths[b], hop)) == T_pad for every b; the kernels clamp a length into (n_fft/2, L]. */
int fd_stft_compress_ragged(const fd_stft_plan* plan, const float* y, const int* lengths, int B, int L, float alpha, float beta,
                            int normalize, float* normfac, float* Y, int T_pad, void* ws, size_t ws_bytes, void* stream);
/* T = 1 + L / hop (the frame count of the row length). */
int fd_decompress_istft_ragged(const fd_stft_plan* plan, const float* X, const int* lengths, int B, int T, int T_pad, float alpha,
                               float beta, const float* normfac, float* y, int L, void* ws, size_t ws_bytes, void* stream);
/* CompressAmplitudesAndScale.forward (inverse = 0: beta |x|^alpha e^{j angle x}) / .invert (inverse = 1) on n complex64
 * values (feature_extractors.py:118-139) as a stand-alone pass; X == Y allowed. */
int fd_compress_spec(const float* X, float* Y, long long n, float alpha, float beta, int inverse, void* stream);
/* The pieces of the transforms on their own, for tests.
 *   fd_stft_tables (host memory): the plan's tables for (n_fft, hop), validated as fd_stft_plan_create does.  Returns kpad (the GEMM
 *     width: 2 (n_fft/2 + 1) rounded up to a multiple of 128) or FD_EINVAL; with Dt, E and w2 all NULL it only returns kpad.
 *     Dt [kpad][kpad]: row k, columns 2f / 2f+1 = w[k] cos / -w[k] sin (2 pi k f / n_fft); E [kpad][kpad]: rows 2f / 2f+1, column n =
 *     c_f w[n] cos / -c_f w[n] sin (2 pi n f / n_fft) / n_fft, c_f = 1 at DC and Nyquist, else 2; zero beyond n_fft / the 2 (n_fft/2 + 1)
 *     spectrum columns.  w2 [n_fft] = w^2, w the float32 symmetric Hann window.
 *   fd_stft_gemm_variant (host only): the tile width BN (128 or 32) fd_stft_gemm_f32 would launch for M x N x K, FD_EINVAL if it refuses.
 *   fd_stft_gemm_f32: the transforms' DFT GEMM, device C[M][N] = A[M][K] B[K][N] (row-major float32; M >= 1, N a multiple of 128, K of
 *     16, A / B / C 16-byte aligned -- anything else is refused on the host).
 *   fd_istft_envelope_ok (host only): 1 if fd_decompress_istft takes (n_fft, hop, T, L), 0 if it refuses because the overlap-add window
 *     envelope falls below 1e-11 on a kept sample (exactly where torch.istft(center=True, length=L) raises); FD_EINVAL for bad
 *     arguments.  Always 1 for FlowModel.enhance's own T = 1 + L / hop with hop <= n_fft / 2.  The ragged form cannot see its lengths
 *     on the host and refuses hop > n_fft / 2 (and n_fft < 4) altogether. */
int fd_stft_tables(int n_fft, int hop, float* Dt, float* E, float* w2);
int fd_stft_gemm_variant(int M, int N, int K);
int fd_stft_gemm_f32(const float* A, const float* B, float* C, int M, int N, int K, void* stream);
int fd_istft_envelope_ok(int n_fft, int hop, int T, int L);
int fd_num_frames(int L, int hop);     /* 1 + L / hop */
/* One AttnBlockpp.forward with skip_rescale (layerspp.py:72-101; the bottleneck block of the SGMSE-style backbone):
 * out = (x + NIN_3(softmax(q k^T C^-0.5) v)) / sqrt(2), q | k | v = NIN_0..2(GroupNorm_0(x)), GroupNorm_0 = min(C/4, 32) groups,
 * eps 1e-6, affine, no SiLU; the softmax runs over all H*W positions of an image.  x / out = NHWC [B][H][W][C] in `dtype`
 * (FD_BF16 or FD_F32); every product, sum and exponential is float32 in both.  C = 16, 32, 64, 128 or 256.
 *   w_qkv = [C][3C]: NIN_0.W | NIN_1.W | NIN_2.W side by side (NIN.W is [in][out]),  b_qkv = [3C] likewise
 *   w_out = NIN_3.W [C][C],  b_out = NIN_3.b [C]
 * stats (optional, may be NULL): the GroupNorm partial sums of out, [B][ceil(H*W / 16)][C][2] (sum, sum of squares). */
typedef struct fd_attn_desc {
  int C;
  const float *gn_gamma, *gn_beta;
  const float *w_qkv, *b_qkv;
  const float *w_out, *b_out;
} fd_attn_desc;
size_t fd_attn_block_workspace_bytes(const fd_attn_desc* d, int B, int H, int W, int dtype);
int fd_attn_block(const fd_attn_desc* d, const void* x, void* out, float* stats, int B, int H, int W, int dtype, void* ws, size_t ws_bytes,
                  void* stream);

int fd_padded_frames(int T);           /* next multiple of 64 */

/* ------------------------------------------------------------------------------------------------
 * Whole-model entry points
 * ---------------------------------------------------------------------------------------------- */
typedef struct fd_model fd_model;

typedef struct fd_model_config {
  int nf;                /* 64 */
  int ch_mult[8];        /* {4,4,4,2} */
  int num_levels;        /* 4 */
  int num_res_blocks;    /* 1 */
  int n_fft;             /* 1534 */
  int hop;               /* 384 */
  float alpha, beta;     /* 0.3, 0.33 */
  int act_dtype;         /* FD_BF16 (bf16 storage + bf16 MFMA) [| FD_WINOGRAD | FD_WINOGRAD_LOWRES | FD_WINOGRAD_AUTO | FD_LOW_LATENCY], FD_F32 (f32 storage + exact f32 MFMA) [| FD_WINOGRAD_AUTO], FD_F32 | FD_BF16_OPERANDS or FD_F32 | FD_BF16X3_OPERANDS */
} fd_model_config;

int fd_model_create(const fd_model_config* cfg, fd_model** out);
/* Architecture switches beyond the shipped backbone (fd_model_create = fd_model_create_ex with {0, 1}):
 *   bottleneck_attn  1 = an AttnBlockpp between the two middle ResBlocks (ncsnpp.py:196-199, 325-330; one more all_modules slot)
 *   output_ksize     1 = output_layer 1x1 [2][4][1][1]; 3 = 3x3 with zero padding 'same' [2][4][3][3]; never a bias
 * The SGMSE-style backbone (config/model/backbone/ncsnpp_default_ycond.yaml) is {1, 3} with nf = 128. */
typedef struct fd_model_arch {
  int bottleneck_attn;
  int output_ksize;
} fd_model_arch;
int fd_model_create_ex(const fd_model_config* cfg, const fd_model_arch* arch, fd_model** out);
void fd_model_destroy(fd_model* m);
/* Number of parameter tensors the model expects, and the i-th name / shape (reference state_dict
 * layout `backbone.all_modules.<i>.<...>`). */
int fd_model_num_params(const fd_model* m);
int fd_model_param_info(const fd_model* m, int i, const char** name, int* ndim, int shape[4]);
/* Copy one parameter (float32, HOST pointer, contiguous, reference shape) into the model. */
int fd_model_set_param(fd_model* m, const char* name, const float* host_data, long long numel);
/* sigma_y: per-frequency curve [n_freq] (float64 host) or a scalar (n = 1) (model.py:399-419). */
int fd_model_set_sigma_y(fd_model* m, const double* host_sigma, int n);
/* Pack weights for MFMA and upload; must be called after all fd_model_set_param and before forward. */
int fd_model_finalize(fd_model* m, void* stream);

size_t fd_model_workspace_bytes(const fd_model* m, int B, int T_pad);
/* v = NCSNpp(x, y, t): x, y, v complex64 [B][1][F][T_pad]; t float32 [nt] with nt in {1, B}
 * (FlowModel.forward, model.py:470-474; ncsnpp.py:254-399). */
int fd_ncsnpp_forward(fd_model* m, const float* x, const float* y, const float* t, int nt, float* v, int B, int T_pad,
                      void* ws, size_t ws_bytes, void* stream);
/* x0 = Y + sigma_fac * (sigma_y * noise) (model.py:512,530-536), then the fixed-step solve over
 * t_span = linspace(0,1,N+1) (:513-514) -- torchdyn fixed-step semantics restated (oracle/flowdec_oracle.py
 * odeint_fixed).  X (in: Y; out: final state) complex64 [B][1][F][T_pad]; noise complex64 same shape
 * (standard complex normal, supplied by the caller so results are reproducible); traj (optional)
 * receives all N+1 states.  use_graph != 0 captures the whole solve into a hipGraph cached per
 * (B, T_pad, N, solver) and replays it. */
int fd_ode_solve(fd_model* m, const float* Y, const float* noise, float sigma_fac, int N, int solver, float* X_out,
                 float* traj, int B, int T_pad, void* ws, size_t ws_bytes, int use_graph, void* stream);
/* Adaptive Dormand-Prince 5(4) over t_span = linspace(0, 1, N+1) (solver='dopri5' of the reference's torchdyn NeuralODE,
 * model.py:487-514; controller semantics restated, see oracle/).  Host-driven: the error ratio of every attempted step is
 * read back, so the call synchronises `stream` and cannot be graph-captured.  traj (optional) receives the N+1 states at
 * the t_span checkpoints, *nfe_out the number of vector-field evaluations. */
size_t fd_ode_adaptive_workspace_bytes(const fd_model* m, int B, int T_pad);
int fd_ode_solve_adaptive(fd_model* m, const float* Y, const float* noise, float sigma_fac, int N, float atol, float rtol,
                          float* X_out, float* traj, int* nfe_out, int B, int T_pad, void* ws, size_t ws_bytes, void* stream);
/* Same driver with the embedded pair chosen by id: Dormand-Prince 5(4) ('dopri5') or Tsitouras 5(4) ('tsit5', the default solver of
 * torchdyn's NeuralODE); both 7 stages with FSAL, the same controller. */
#define FD_ADAPTIVE_DOPRI5 0
#define FD_ADAPTIVE_TSIT5 1
int fd_ode_solve_adaptive_method(fd_model* m, const float* Y, const float* noise, float sigma_fac, int N, int method, float atol, float rtol,
                                 float* X_out, float* traj, int* nfe_out, int B, int T_pad, void* ws, size_t ws_bytes, void* stream);
/* The same solvers with PER-CLIP step control.  The two calls above accept or reject a step on one error ratio taken over the whole
 * [B][F][T_pad] state (torchdyn's behaviour for a batched call), so a clip's result depends on its batch companions.  Here every clip
 * carries its own t, dt, checkpoint index and accept / reject decisions: clip b's final state, trajectory planes and nfe_out[b] are
 * BIT-IDENTICAL to the B = 1 call above on that clip, whatever else is in the batch and however the batch is sharded.
 *   noise / seeds   exactly one is given: noise = complex64 [B][1][F][T_pad] as above, or seeds = DEVICE uint64 [B] (the library's own
 *                   noise, draw 0, as in fd_ode_solve_seeded; equals the buffer form on fd_noise_fill's planes).
 *   B               at most 256 clips (the per-sample time table of the network); more is refused.
 *   nfe_out         HOST int [B]: the evaluations made while clip b was still integrating = the nfe of its one-clip call.
 *   rejected_out    HOST int [B] or NULL: clip b's rejected attempts.
 *   evals_out       HOST int or NULL: the network evaluations (each over the whole batch) the call ran, 2 + 6 x attempts.  A clip that has
 *                   reached t = 1 rides along with dt = 0, untouched, until the slowest clip is done; B x *evals_out against the sum of
 *                   nfe_out is that waste.
 *   traj            optional [N+1][B][1][F][T_pad]: clip b's plane of checkpoint i is written when clip b lands on it.
 * Host-driven like the calls above: one synchronisation of `stream` per attempted step (one small host-to-device table -- step sizes,
 * stage times, the previous attempt's commit flags -- and one read-back of B x 512 partial sums), no graph capture.  The workspace is
 * fd_ode_adaptive_clips_workspace_bytes (0 for a bad shape or B > 256). */
size_t fd_ode_adaptive_clips_workspace_bytes(const fd_model* m, int B, int T_pad);
int fd_ode_solve_adaptive_clips(fd_model* m, const float* Y, const float* noise, const unsigned long long* seeds, float sigma_fac, int N, int method,
                                float atol, float rtol, float* X_out, float* traj, int* nfe_out, int* rejected_out, int* evals_out, int B, int T_pad,
                                void* ws, size_t ws_bytes, void* stream);
size_t fd_enhance_workspace_bytes(const fd_model* m, int B, int L);
/* Byte offset, inside the workspace of fd_enhance / fd_score_enhance / fd_regression_enhance, of the B float32 normalisation
 * factors the front end computed (EnhancementModel._preprocess' `normfac`, model.py:156-162); valid after the call. */
size_t fd_enhance_normfac_offset(const fd_model* m, int B, int L);
/* FlowModel.enhance (model.py:476-528) end to end on device buffers: y [B][L] f32 -> x_hat [B][L] f32. */
int fd_enhance(fd_model* m, const float* y, const float* noise, float sigma_fac, int N, int solver, float* x_hat, int B,
               int L, void* ws, size_t ws_bytes, int use_graph, void* stream);
/* FlowModel.enhance on a ragged batch (see "Ragged batches" above): workspace as for fd_enhance(B, L); noise [B][1][F][T_pad];
 * clip b bit-identical to fd_enhance on that clip alone with the same noise.  A captured graph is keyed on the POINTER `lengths`
 * (its contents may change between replays). */
int fd_enhance_ragged(fd_model* m, const float* y, const int* lengths, const float* noise, float sigma_fac, int N, int solver,
                      float* x_hat, int B, int L, void* ws, size_t ws_bytes, int use_graph, void* stream);
/* ---- Seeded noise: the library draws the sampler's Gaussian noise itself, from one 64-bit seed per clip ----------------------
 * The reference draws from the global device RNG (model.py:512,530-536; correctors.py:61); the entry points above take the noise
 * as a buffer.  The *_seeded forms take `seeds` (DEVICE uint64 [B]) instead and generate every value in registers, in the kernel
 * that consumes it -- no noise buffer exists.  The value at (clip seed s, draw index d >= 0, frequency row f, frame t) is a pure
 * function (NORMATIVE):
 *   - Philox4x32-10 (Random123: multipliers 0xD2511F53, 0xCD9E8D57; Weyl constants 0x9E3779B9, 0xBB67AE85) with key
 *     (s & 0xffffffff, s >> 32) and counter (t >> 1, f, d, 0) gives r0..r3.  Counter word 3 is reserved: the noise uses value 0 only.
 *     Value 1 is the clip's validation-loss time ("Validation loss" below): counter (0, 0, 0, 1), u = (r0 >> 8) * 2^-24 in [0, 1).
 *     Every other value of word 3 stays unused.
 *   - t is the ABSOLUTE frame: frame0[b] + the local frame (column) of row b, where frame0 (DEVICE int32 [B], fd_noise_fill_at /
 *     fd_enhance_chunks / fd_score_enhance_chunks, every draw of the sampler / fd_op_init_state / fd_caxpy_at / fd_score_update_at)
 *     says where in a longer recording the row starts; 0 <= frame0[b] and frame0[b] + T_pad < 2^31.  Every other entry point, and a NULL
 *     frame0, has frame0 = 0: t is the local frame.
 *   - an even t uses (ra, rb) = (r0, r1), an odd t (r2, r3).
 *   - u1 = ((ra >> 9) + 0.5) * 2^-23 in (0, 1), u2 = (rb >> 8) * 2^-24 in [0, 1): both exact in float32.
 *   - z = sqrt(-ln u1) * (cos 2 pi u2 + i sin 2 pi u2) in float32 (logf, sqrtf, sincospif(2 u2)): complex normal with
 *     E|z|^2 = 1 (variance 1/2 per component, like torch.randn(complex64)); |z| <= sqrt(24 ln 2) ~ 4.08.
 *   - draw index: 0 for the flow models' initial state; for the score sampler the k-th randn_like of the reference's order,
 *     i.e. the index of the plane fd_score_enhance reads (a plane whose coefficient is zero still takes its index).
 * So a clip's noise does not depend on B, its position in the batch, T_pad, the rank, or how many draws precede it, and a
 * seeded call equals, bit for bit, the buffer call on fd_noise_fill's output.  A captured graph is keyed on the POINTER `seeds`
 * (like `lengths`): its contents may change between replays.  Workspaces: the unseeded calls' fd_*_workspace_bytes. */
#define FD_NOISE_GAUSSIAN 0 /* out = complex64 [n_draws][B][F][T_pad]: the layout fd_score_enhance consumes; n_draws = 1: fd_enhance's */
#define FD_NOISE_BITS 1     /* out = uint32 [n_draws][B][F][T_pad][2]: the raw words (ra, rb) of every element (for tests) */
/* The planes draw0 .. draw0 + n_draws - 1 written to `out` (16-byte aligned device memory). */
int fd_noise_fill(void* out, const unsigned long long* seeds, int B, int F, int T_pad, int draw0, int n_draws, int mode, void* stream);
/* The same planes at absolute frames: column t of row b holds frame frame0[b] + t, i.e. the columns [frame0[b], frame0[b] + T_pad) of an
 * fd_noise_fill plane with a larger T_pad.  frame0 = NULL is fd_noise_fill, bit for bit. */
int fd_noise_fill_at(void* out, const unsigned long long* seeds, const int* frame0, int B, int F, int T_pad, int draw0, int n_draws, int mode,
                     void* stream);
/* fd_ode_solve with x0 = Y + sigma_fac * (sigma_y * z(seeds[b], 0, f, t)). */
int fd_ode_solve_seeded(fd_model* m, const float* Y, const unsigned long long* seeds, float sigma_fac, int N, int solver, float* X_out,
                        float* traj, int B, int T_pad, void* ws, size_t ws_bytes, int use_graph, void* stream);
/* fd_enhance (lengths == NULL: every clip is L samples long) or fd_enhance_ragged (lengths = DEVICE int32 [B]) on seeded noise. */
int fd_enhance_seeded(fd_model* m, const float* y, const int* lengths, const unsigned long long* seeds, float sigma_fac, int N, int solver,
                      float* x_hat, int B, int L, void* ws, size_t ws_bytes, int use_graph, void* stream);
/* ---- Long-form: a recording of any length as overlapping rows of one (B, T_pad) bucket (planner: flowdec_amd/longform.py) ------------
 * No counterpart in the reference, whose driver skips files over 30 s (enhance.py:115, :139).  Row r of a recording holds its samples
 * [start_r, start_r + lengths[r]), start_r a multiple of hop, so that the row's frame grid is the recording's and frame0 = start_r / hop.
 * fd_enhance_chunks = fd_enhance_seeded on ragged rows plus two optional DEVICE arrays:
 *   frame0     int32 [B]: the initial state uses the recording's noise z(seeds[b], 0, f, frame0[b] + t) ("Seeded noise" above) -- rows that
 *              overlap start from bit-identical noise in their overlap.
 *   normfac_in float [B]: the recording's normalisation factor (fd_normfac).  The per-row maximum is not taken: the front end divides
 *              by normfac_in[b], the back end multiplies by it; the workspace's normfac slot (fd_enhance_normfac_offset) is not written.
 * Both NULL: fd_enhance_seeded, bit for bit.  Workspace: fd_enhance_workspace_bytes(m, B, L).  A captured graph is keyed on the POINTERS
 * lengths, seeds, frame0 and normfac_in (their contents may change between replays: one graph serves every group of rows of a file).
 * The ScoreDec and regression baselines run the same rows through fd_score_enhance_chunks / fd_regression_enhance_chunks (declared with the
 * baselines below): the same two arrays with the same meaning, frame0 applied to every draw of the score sampler; the regression model
 * draws no noise and takes normfac_in only.  fd_normfac and fd_stitch_chunks serve the three classes alike. */
int fd_enhance_chunks(fd_model* m, const float* y, const int* lengths, const unsigned long long* seeds, const int* frame0, const float* normfac_in,
                      float sigma_fac, int N, int solver, float* x_hat, int B, int L, void* ws, size_t ws_bytes, int use_graph, void* stream);
/* The front end's normalisation rule on its own: normfac_out[b] = max |y[b][0 .. len_b)|, 1 where that is <= 1e-8 (torch.isclose(., 0));
 * y [B][L], lengths DEVICE int32 [B] or NULL (len_b = L); rows of ANY length 1 <= len_b <= L <= 2^31 - 1025.  One workgroup per row. */
int fd_normfac(const float* y, const int* lengths, int B, int L, float* normfac_out, void* stream);
/* out [n] (n < 2^31) = a recording's output from its rows' outputs.  rows [n_rows][row_stride] float32: row r holds the recording's samples
 * from starts[r] on; bounds[r - 1] (r = 1 .. n_rows - 1, ascending) = the boundary between the rows r - 1 and r (starts, bounds: DEVICE
 * int32; bounds may be NULL for one row).  Sample i is copied from the row whose [bounds[r - 1], bounds[r]) holds it, except in the
 * cross-fades: for i in [bounds[r - 1] - xfade / 2, bounds[r - 1] + xfade / 2), with a / b = the earlier / later row's sample,
 *   out[i] = a + w * (b - a),  w = weights[i - (bounds[r - 1] - xfade / 2)]
 * -- subtraction, product and sum each rounded to float32 on its own (no fused multiply-add).  weights: DEVICE float32 [xfade], by
 * convention w_k = 0.5 - 0.5 cos(pi (k + 0.5) / xfade) evaluated in float64 and rounded once (flowdec_amd.longform.stitch_weights); xfade
 * even, 0 = no cross-fade.  The caller keeps the cross-fades inside both rows and apart from each other (plan_rows does); an index outside
 * a row is clamped into it. */
int fd_stitch_chunks(const float* rows, long long row_stride, const int* starts, const int* bounds, int n_rows, const float* weights, int xfade,
                     float* out, long long n, void* stream);
/* ---- Streaming: the same rows, run as the input arrives (session layer: flowdec_amd/stream.py; planner: longform.StreamPlanner) -------
 * A stream's output is, bit for bit, enhance_long's on the concatenated input, however the input was cut into pushes and whichever other
 * streams shared its native calls.  With h = hop, rf = row_frames, halo = halo_frames, X = xfade (even), half = X / 2:
 *   W = rf * h - 1 (row samples), S = (rf - 2 * halo - 1) * h (stride), Bo = (rf - halo - 1) * h (boundary after a row's start).
 * Regular row j = [j * S, j * S + W) can run as soon as MORE than j * S + W samples have arrived (it is then known not to be the last
 * row); the end of the stream (n samples) adds the last row exactly as plan_rows places it.  After regular row j the samples
 * [lo_j - half, hi_j - half) are final (lo_j = (j - 1) * S + Bo, hi_j = j * S + Bo; lo_0 - half reads 0), after the last row everything
 * up to n.  Worst-case algorithmic delay: a sample leaves once (rf - halo) * h + half FURTHER samples have arrived (plus one row's compute time).
 * A session keeps its input from the start of the previous regular row on: the last row starts at most S - h before the next regular start.
 * Normalisation that needs no whole file: a fixed factor, or CAUSAL -- row j is scaled by fd_normfac of everything up to the row's end
 * (a running maximum: exact, and independent of how the input was pushed).  Overlapping rows then differ slightly in scale; the
 * cross-fade absorbs it.
 * One step of a pool of sessions = one table upload and three launches whatever the number of sessions:
 *   fd_stream_gather (rings -> y [B][L], lengths' zero tails, causal factors) -> fd_enhance_chunks -> fd_stream_emit (x_hat -> outputs, tails).
 * gather and emit know nothing of the model: with fd_score_enhance_chunks or fd_regression_enhance_chunks in the middle the same step
 * serves a ScoreDec or a regression model (all rows of a call share one fd_score_config).
 * Both read ONE DEVICE table, an entry per row of the call (at most one row of a session per call): */
typedef struct fd_stream_row {
  const float* ring;     /* gather: the session's input ring, ring_cap floats; absolute sample i lives at ring[i % ring_cap] */
  long long start;       /* gather: absolute index of the row's first sample (>= 0) */
  int ring_cap;          /* gather: >= length */
  int length;            /* gather: samples of the row, 1 .. L */
  int peak_slot;         /* gather: the session's slot in peak[] (causal normalisation) */
  int emit_lo;           /* emit: row-local index of the first finished sample (boundary with the previous row - half; 0 for a first row) */
  int emit_count;        /* emit: finished samples, written to out[0 .. emit_count) */
  int tail_lo;           /* emit: row-local index of (boundary with the next row - half): the new tail is x_hat[b][tail_lo .. tail_lo + X) */
  const float* tail_in;  /* emit: the previous row's tail [X], or NULL for a session's first row */
  float* tail_out;       /* emit: where this row's tail [X] goes, or NULL for a session's last row.  NOT tail_in: the old tail is read and
                          *       the new one written in the same launch -- keep two buffers per session and alternate by row parity */
  float* out;            /* emit: destination of the finished samples */
} fd_stream_row;
/* y [B][L] float32: y[b][0 .. length_b) = the ring's samples [start_b, start_b + length_b), y[b][length_b .. L) = 0.  peak / normfac_out
 * (both or neither; DEVICE float32 [slots] / [B]): peak[peak_slot_b] = max(peak[peak_slot_b], max |row b|), normfac_out[b] = that peak,
 * 1 where it is <= 1e-8 (fd_normfac's rule).  Zero a session's slot when it opens.  One workgroup per row. */
int fd_stream_gather(const fd_stream_row* table, int B, float* y, int L, float* peak, float* normfac_out, void* stream);
/* x_hat [B][L] float32 (fd_enhance_chunks' output).  out_b[i] = x_hat[b][emit_lo_b + i], i < emit_count_b, except where a previous row
 * exists (tail_in_b != NULL) and i < xfade: out_b[i] = a + w * (x - a) with a = tail_in_b[i], w = weights[i], x = x_hat[b][emit_lo_b + i]
 * -- fd_stitch_chunks' arithmetic and weights table (three roundings, no fused multiply-add).  Then tail_out_b[k] = x_hat[b][tail_lo_b + k],
 * k < xfade, unless tail_out_b is NULL.  Row-local indices are clamped into [0, L). */
int fd_stream_emit(const fd_stream_row* table, int B, const float* x_hat, int L, const float* weights, int xfade, void* stream);
/* normalize_mode of the model's front end: 1 = 'noisy' (default), 0 = 'none' (model.py:52, util/other.py:70). */
int fd_model_set_normalize(fd_model* m, int normalize);

/* ---- ScoreDec / regression baselines on the same backbone -------------------------------
 * ScoreModel.enhance (model.py:630-657) with the predictor-corrector sampler of sampling/__init__.py:32-72 on the OUVE
 * SDE (sdes.py:132-206): predictors reverse_diffusion / euler_maruyama / none (sampling/predictors.py:48-83), correctors
 * ald / none (sampling/correctors.py:42-80); the score is -backbone(x, y, t) / std(t) (model.py:613-628).
 * Three forms of the sampler: fd_score_enhance (noise planes, clips of one length), fd_score_enhance_seeded (per-clip seeds, one length)
 * and fd_score_enhance_ragged (either noise source, clips of different lengths in one T_pad bucket); fd_regression_enhance has the
 * ragged form fd_regression_enhance_ragged.  A clip's result is the same, bit for bit, through every form that can express it. */
#define FD_PREDICTOR_REVERSE_DIFFUSION 0
#define FD_PREDICTOR_EULER_MARUYAMA 1
#define FD_PREDICTOR_NONE 2
#define FD_CORRECTOR_ALD 0
#define FD_CORRECTOR_NONE 1
typedef struct fd_score_config {
  float theta, sigma_min, sigma_max; /* OUVESDE(theta, sigma_min, sigma_max), config/model/sde/ouve_final.yaml */
  float t_eps;                       /* ScoreModel.t_eps: timesteps = linspace(1, t_eps, N) */
  float snr;                         /* corrector target SNR */
  int N;                             /* reverse steps */
  int predictor, corrector, corrector_steps;
  int denoise;                       /* != 0: return the noise-free mean of the last predictor step */
} fd_score_config;
/* Number of Gaussian draws the sampler consumes: 1 (prior) + N * (corrector_steps [ald] + 1 [predictor != none]). */
int fd_score_num_draws(const fd_score_config* cfg);
/* y [B][L] f32 -> x_hat [B][L] f32.  noise = [fd_score_num_draws][B][n_freq][T_pad] complex64 standard normal, consumed in
 * the order of the reference's randn_like calls.  Workspace: fd_enhance_workspace_bytes(m, B, L). */
int fd_score_enhance(fd_model* m, const float* y, const float* noise, const fd_score_config* cfg, float* x_hat, int B, int L,
                     void* ws, size_t ws_bytes, int use_graph, void* stream);
/* The same sampler on seeded noise ("Seeded noise" above): no [fd_score_num_draws][B][n_freq][T_pad] buffer is needed. */
int fd_score_enhance_seeded(fd_model* m, const float* y, const unsigned long long* seeds, const fd_score_config* cfg, float* x_hat, int B,
                            int L, void* ws, size_t ws_bytes, int use_graph, void* stream);
/* ScoreModel.enhance on a ragged batch: the contract of fd_enhance_ragged ("Ragged batches" above), restated.  y / x_hat are [B][L]
 * rows; lengths (DEVICE int32 [B], required) the clips' own sample counts -- the CALLER guarantees that every clip pads to the T_pad of
 * L (the kernels clamp a length into (n_fft/2, L]).  Exactly one of noise ([fd_score_num_draws][B][n_freq][T_pad] complex64) and seeds
 * (DEVICE uint64 [B], "Seeded noise" above) is non-NULL; both or neither is FD_EINVAL.  Clip b is bit-identical to fd_score_enhance /
 * fd_score_enhance_seeded on that clip alone with its noise planes / its seed; samples [lengths[b], L) of a row of x_hat are zero.
 * Workspace: fd_enhance_workspace_bytes(m, B, L).  A captured graph is keyed on the POINTERS lengths, noise and seeds (their contents
 * may change between replays) and on the values of *cfg. */
int fd_score_enhance_ragged(fd_model* m, const float* y, const int* lengths, const float* noise, const unsigned long long* seeds,
                            const fd_score_config* cfg, float* x_hat, int B, int L, void* ws, size_t ws_bytes, int use_graph, void* stream);
/* Long-form ("Long-form" above): fd_score_enhance_ragged on seeds (required, as lengths) plus the two optional DEVICE arrays of
 * fd_enhance_chunks.  frame0 (int32 [B]): EVERY one of the fd_score_num_draws(cfg) planes -- the prior and each predictor / corrector
 * draw -- is the recording's, z(seeds[b], draw, f, frame0[b] + t), so two overlapping rows see bit-identical noise where they overlap at
 * every step of the sampler.  normfac_in (float [B]) replaces the per-row maximum in the front and the back end.  Both NULL:
 * fd_score_enhance_ragged(seeds), bit for bit.  An invalid argument is FD_EINVAL before any launch.  Workspace:
 * fd_enhance_workspace_bytes(m, B, L).  A captured graph is keyed on the POINTERS lengths, seeds, frame0 and normfac_in (their contents
 * may change between replays) and on the values of *cfg. */
int fd_score_enhance_chunks(fd_model* m, const float* y, const int* lengths, const unsigned long long* seeds, const int* frame0,
                            const float* normfac_in, const fd_score_config* cfg, float* x_hat, int B, int L, void* ws, size_t ws_bytes,
                            int use_graph, void* stream);
/* One score-network evaluation in the form the black-box ODE sampler needs (sampling/__init__.py:75-146, which drives
 * scipy.integrate.solve_ivp on the host): x, Y, out = complex64 [B][1][n_freq][T_pad]; workspace fd_model_workspace_bytes.
 *   FD_SCORE_DRIFT_PF : out = theta (Y - x) - 0.5 g(t)^2 score(x, Y, t)     (probability-flow drift, sdes.py:93-109)
 *   FD_SCORE_DRIFT    : out = theta (Y - x) -     g(t)^2 score(x, Y, t)     (reverse-SDE drift)
 *   FD_SCORE_DENOISE  : out = mean of one reverse-diffusion predictor step at t (predictors.py:61-71), dt = 1 / cfg->N */
#define FD_SCORE_DRIFT_PF 0
#define FD_SCORE_DRIFT 1
#define FD_SCORE_DENOISE 2
int fd_score_eval(fd_model* m, const float* x, const float* Y, float t, const fd_score_config* cfg, int mode, float* out, int B,
                  int T_pad, void* ws, size_t ws_bytes, void* stream);
/* The ODE sampler itself on the device (ScoreModel.enhance(sampler_type="ode"), sampling/__init__.py:75-146): the probability-flow ODE
 * integrated from t = 1 down to cfg->t_eps by Dormand-Prince 5(4) under the step-size rule of scipy.integrate.RK45 -- its
 * select_initial_step, its strict acceptance err < 1, its growth and shrink factors, its clamp to the end of the span --, restated in
 * double precision (Rk45Ctl, csrc/step_ctl.h); the network is given (float)t like the host-driven sampler gives it.  The state and the
 * stages are float32 planes on the device (scipy carries complex128), the error norm is a float64 sum; one synchronisation per attempted
 * step, no hipGraph.  Of *cfg only theta, sigma_min, sigma_max, t_eps, N and denoise are read; with denoise one FD_SCORE_DENOISE
 * evaluation at t_eps (dt = 1 / N) follows the solve.
 *   step_control = FD_STEP_CONTROL_BATCH: ONE controller on the norms over the whole batch -- what solve_ivp sees, and the reference's
 *     meaning of a batch; nfe_out / rejected_out have one entry.
 *   step_control = FD_STEP_CONTROL_CLIP: one controller per clip (B <= 256): clip b takes the steps, and gives the bits, of the B = 1 call
 *     on it; a clip that has reached t_eps rides along with dt = 0 until the slowest is done.  nfe_out / rejected_out have B entries.
 * Exactly one of noise (complex64 [B][n_freq][T_pad]: the prior sample is Y + std(1) noise) and seeds (DEVICE uint64 [B]: draw 0 of "Seeded
 * noise") is non-NULL.  nfe_out (required): 2 + 6 per attempt, the count scipy reports (the denoising evaluation is not counted);
 * rejected_out, evals_out (optional): rejected attempts, and the network evaluations of the whole batch that ran.
 * FD_EINVAL before any launch for null pointers, bad OUVE parameters, t_eps outside (0, 1), atol <= 0, rtol < 0, an unknown step_control
 * and B > 256 with FD_STEP_CONTROL_CLIP; FD_ENOMEM for a short workspace.  FD_ERUNTIME "step size too small" when a step falls below ten
 * spacings of t (a NaN input ends there after some twenty attempts): scipy's solver stops with a failure status at that point and the
 * reference carries on with the last state without a word -- this library reports it. */
#define FD_STEP_CONTROL_BATCH 0
#define FD_STEP_CONTROL_CLIP 1
size_t fd_score_ode_workspace_bytes(const fd_model* m, int B, int T_pad, int step_control);
int fd_score_ode_solve(fd_model* m, const float* Y, const float* noise, const unsigned long long* seeds, const fd_score_config* cfg, float rtol,
                       float atol, int step_control, float* X_out, int* nfe_out, int* rejected_out, int* evals_out, int B, int T_pad, void* ws,
                       size_t ws_bytes, void* stream);
/* The same from waveform to waveform, with the front end and the back end of fd_score_enhance_ragged: y / x_hat are [B][L] rows, lengths
 * (DEVICE int32 [B]) the clips' own sample counts of ONE T_pad bucket, or NULL when every clip is L samples long.  With
 * FD_STEP_CONTROL_CLIP clip b is bit-identical to the B = 1 call on that clip alone with its noise plane or its seed.  Synchronous. */
size_t fd_score_ode_enhance_workspace_bytes(const fd_model* m, int B, int L, int step_control);
int fd_score_ode_enhance(fd_model* m, const float* y, const int* lengths, const float* noise, const unsigned long long* seeds,
                         const fd_score_config* cfg, float rtol, float atol, int step_control, float* x_hat, int* nfe_out, int* rejected_out,
                         int* evals_out, int B, int L, void* ws, size_t ws_bytes, void* stream);
/* RegressionModel.enhance (model.py:566-578): x_hat = iSTFT(backbone(Y, Y, t = 0)). */
int fd_regression_enhance(fd_model* m, const float* y, float* x_hat, int B, int L, void* ws, size_t ws_bytes, int use_graph,
                          void* stream);
/* RegressionModel.enhance on a ragged batch: the same contract as fd_score_enhance_ragged without noise -- [B][L] rows, lengths (DEVICE
 * int32 [B], required) of ONE T_pad bucket, clip b bit-identical to fd_regression_enhance on that clip alone, samples [lengths[b], L)
 * of a row of x_hat zero, workspace fd_enhance_workspace_bytes(m, B, L), a captured graph keyed on the POINTER lengths. */
int fd_regression_enhance_ragged(fd_model* m, const float* y, const int* lengths, float* x_hat, int B, int L, void* ws, size_t ws_bytes,
                                 int use_graph, void* stream);
/* Long-form ("Long-form" above): fd_regression_enhance_ragged plus normfac_in (DEVICE float [B] or NULL) in place of the per-row maximum,
 * as in fd_enhance_chunks; the model draws no noise, so there is no frame0.  NULL: fd_regression_enhance_ragged, bit for bit.  A captured
 * graph is keyed on the POINTERS lengths and normfac_in. */
int fd_regression_enhance_chunks(fd_model* m, const float* y, const int* lengths, const float* normfac_in, float* x_hat, int B, int L, void* ws,
                                 size_t ws_bytes, int use_graph, void* stream);

/* Per-launch timing of the dominant kernel (conv MFMA) measured with HIP events on the launch stream;
 * used by bench.py for the roofline object.  enable != 0 starts recording (forces eager launches). */
int fd_profile_enable(fd_model* m, int enable);
int fd_profile_read(fd_model* m, double* conv_ms_total, long long* conv_launches, double* conv_flops_total,
                    double* conv_bytes_total /* algorithmic HBM bytes: operands read once + output written once */);
/* The multiply-add FLOPs the convolution launches actually EXECUTED since fd_profile_enable / the last call of this function (reads and
 * resets its own counter; call it before or after fd_profile_read): a Winograd F(4,3) launch executes half, an F(2,3) launch two thirds
 * of the direct count of its 3x3 part.  conv_flops_total of fd_profile_read stays the DIRECT convolution's count. */
int fd_profile_read_executed(fd_model* m, double* conv_flops_executed);
/* Same for the HBM-bound FIR resampling launches (fd_fir_resample inside the model): total time, launches and algorithmic
 * bytes (input read once + every output written once) since fd_profile_enable. */
int fd_profile_read_fir(fd_model* m, double* ms_total, long long* launches, double* bytes_total);
/* Front / back end (ComplexSTFT + compression, feature_extractors.py:86-139): per-kernel time of the LAST forward and the last
 * inverse transform recorded while profiling was on, ms6 = {absmax + framing, forward DFT GEMM, compression, decompression,
 * inverse DFT GEMM, overlap-add}; calls2 = number of forward / inverse calls seen.  The plan-level pair does the same for a
 * caller-owned plan (fd_stft_compress / fd_decompress_istft); fd_profile_enable switches it on for the model's own plan. */
int fd_profile_read_stft(fd_model* m, double* ms6, int* calls2);
int fd_stft_plan_profile(fd_stft_plan* plan, int enable);
int fd_stft_plan_profile_read(fd_stft_plan* plan, double* ms6, int* calls2);

/* ------------------------------------------------------------------------------------------------
 * NDAC codec: the Descript-Audio-Codec architecture whose output FlowDec post-filters.  Reference call
 * sites: demo.ipynb cell 2 (`DAC.load(.../weights.pth)`), cell 3 (`preprocess`, `encode(x, n_quantizers=nq)`,
 * `quantizer.from_codes(codes)`, `decode(zq)`); arithmetic = descript-audio-codec==1.0.0 (requirements.txt:4), a third-party
 * package that is not under /root/reference: restated from the published algorithm, PARITY UNPINNED (oracle/ndac_oracle.py).
 * Layout [B][C][T] float32 like nn.Conv1d.  Weights are passed EFFECTIVE (weight norm g * v / ||v|| folded by the caller:
 * flowdec_amd/ndac.py), under their state_dict names with `.weight` in place of `.weight_g` / `.weight_v`.
 * ---------------------------------------------------------------------------------------------- */
/* Operator level (stateless, re-entrant): nn.Conv1d / nn.ConvTranspose1d with the DAC surroundings fused in.
 *   alpha_in [Ci] or NULL : Snake activation x + sin^2(alpha x) / (alpha + 1e-9) applied to the INPUT (zero padding after it)
 *   residual [B][Co][To] or NULL : added to the result (ResidualUnit: x + block(x));  tanh_out != 0 : tanh of the result
 * w: [Co][Ci][K] (conv) / [Ci][Co][K] (transposed); To = (T + 2 p - d (K - 1) - 1) / s + 1  resp.  (T - 1) s - 2 p + K. */
int fd_conv1d(const float* x, const float* w, const float* bias, const float* alpha_in, const float* residual, float* out, int B, int Ci,
              int T, int Co, int K, int stride, int padding, int dilation, int tanh_out, void* stream);
int fd_conv_transpose1d(const float* x, const float* w, const float* bias, const float* alpha_in, float* out, int B, int Ci, int T, int Co,
                        int K, int stride, int padding, void* stream);
/* The matrix-core convolution of FD_NDAC_MFMA_DECODER / _ENCODER (split-bf16 operands, f32 accumulation) on its own, for tests.
 * Shapes it supports: Co a multiple of 64 or 96; stride 1 (any dilation) or transposed (K % stride == 0, dilation 1) with Ci % 32 == 0;
 * strided (stride 2 / 4 / 5 / 8 / 10, K % stride == 0, dilation 1) with any Ci; the staged tile (256 + span) x 160 B within 64 KiB.
 *   fd_ndac_mfma_packed_bytes / _pack_weights (host memory): PyTorch weights w ([Co][Ci][K] conv, [Ci][Co][K] transposed) -> the
 *     kernel's pre-split A-operand layout (hi and lo bf16 terms); bytes 0 / FD_EINVAL for an unsupported shape.
 *   fd_ndac_mfma_variant (host only): the launch fd_ndac_mfma_conv1d would make, variant[5] = {MT (32-channel tiles per workgroup:
 *     2 or 3), S (0: stride 1 or transposed; else the polyphase stride), NT (32-position tiles per wave: 1 or 2), grid.x, grid.y}.
 *   fd_ndac_mfma_conv1d: device x [B][Ci][T] (already activated), packed weights, bias [Co]; outputs [B][Co][To]: out = conv + bias
 *     (+ residual), out_act = Snake of it with alpha_out [Co] (hardware sine).  Any of out / out_act may be NULL but not both; a
 *     residual needs out_act. */
size_t fd_ndac_mfma_packed_bytes(int Ci, int Co, int K, int stride, int transposed);
int fd_ndac_mfma_pack_weights(const float* w, int Ci, int Co, int K, int stride, int transposed, void* packed);
int fd_ndac_mfma_variant(int B, int Ci, int T, int Co, int K, int stride, int pad, int dil, int transposed, int* variant);
int fd_ndac_mfma_conv1d(const float* x, const void* packed, const float* bias, const float* residual, float* out, float* out_act,
                        const float* alpha_out, int B, int Ci, int T, int Co, int K, int stride, int pad, int dil, int transposed, void* stream);

typedef struct fd_ndac fd_ndac;
typedef struct fd_ndac_config {   /* dac.DAC.__init__ keyword arguments (the `metadata["kwargs"]` of a weights.pth) */
  int encoder_dim;                /* 64 */
  int encoder_rates[8];           /* e.g. {2,4,8,8}; hop length = their product */
  int n_encoder_rates;
  int latent_dim;                 /* encoder_dim * 2^n_encoder_rates unless the checkpoint says otherwise */
  int decoder_dim;                /* 1536 */
  int decoder_rates[8];           /* e.g. {8,8,4,2} */
  int n_decoder_rates;
  int n_codebooks, codebook_size, codebook_dim;   /* 9, 1024, 8 (codebook_dim <= 8) */
} fd_ndac_config;
int fd_ndac_create(const fd_ndac_config* cfg, fd_ndac** out);
void fd_ndac_destroy(fd_ndac* m);
int fd_ndac_hop_length(const fd_ndac* m);
int fd_ndac_num_params(const fd_ndac* m);
int fd_ndac_param_info(const fd_ndac* m, int i, const char** name, int* ndim, int shape[3]);
int fd_ndac_set_param(fd_ndac* m, const char* name, const float* host_data, long long numel);   /* float32 HOST pointer */
int fd_ndac_finalize(fd_ndac* m, void* stream);   /* uploads; normalises the codebooks (synchronous, init time) */
/* Arithmetic (bit flags).  FD_NDAC_EXACT: float32 on the vector ALUs in a defined operation order; the encoder's code indices are
 * bit-identical to oracle/ndac_oracle.py.  FD_NDAC_MFMA_DECODER (the default): the decoder's wide convolutions run on the matrix
 * cores with both operands split into two bf16 terms (three products, f32 accumulation: ~1e-6 relative per layer) and the hardware
 * sine in Snake; decode agrees with the exact path to ~1e-5 of the waveform peak.  FD_NDAC_MFMA_ENCODER (opt-in): the same for
 * the encoder; the latent agrees to ~1e-5, so a code index can differ from the exact path where two codebook entries are within
 * that distance of a tie (tests/test_hip_ndac.py bounds the fraction). */
#define FD_NDAC_EXACT 0
#define FD_NDAC_MFMA_DECODER 1
#define FD_NDAC_MFMA_ENCODER 2
int fd_ndac_set_precision(fd_ndac* m, int flags);
int fd_ndac_get_precision(const fd_ndac* m);
int fd_ndac_latent_frames(const fd_ndac* m, int L);    /* frames for L samples (L % hop == 0: L / hop) */
int fd_ndac_decoded_length(const fd_ndac* m, int T);   /* samples the decoder produces for T frames */
size_t fd_ndac_workspace_bytes(const fd_ndac* m, int B, int L);   /* covers encode of [B][L] and decode of its frames */
/* dac.DAC.encode (eval): x [B][L] (L % hop == 0: DAC.preprocess pads) -> z_q [B][latent][T] f32, codes [B][nq][T] int32,
 * latents [B][nq * codebook_dim][T] or NULL.  n_quantizers <= 0 or > n_codebooks: all of them. */
int fd_ndac_encode(fd_ndac* m, const float* x, int B, int L, int n_quantizers, float* z_q, int* codes, float* latents, void* ws,
                   size_t ws_bytes, void* stream);
/* ResidualVectorQuantize.forward on a given latent z [B][latent][T] (ws: B * latent * T floats) / .from_codes */
int fd_rvq_encode(fd_ndac* m, const float* z, int B, int T, int n_quantizers, float* z_q, int* codes, float* latents, void* ws,
                  size_t ws_bytes, void* stream);
int fd_rvq_from_codes(fd_ndac* m, const int* codes, int B, int n_quantizers, int T, float* z_q, void* stream);
/* fd_rvq_encode as ONE launch (rvq_chain_kernel: the residual tile stays in LDS across the quantisers, z_q accumulates in registers): z is
 * read-only and no workspace is needed.  codes, z_q and latents are BIT-IDENTICAL to fd_rvq_encode on the same z.  frames: DEVICE int32
 * [B] or NULL; under a table clip b is the first frames[b] frames of its row, 1 <= frames[b] <= T (checked on the host as
 * fd_ndac_decode_ragged does: FD_EINVAL leaves the outputs untouched); frames at and behind frames[b] are never read, and get code 0,
 * z_q 0 and latents 0.  fd_rvq_chain_supported(latent_dim, codebook_dim) (host only) says whether the kernel takes the shape: the
 * [latent_dim][8] float32 tile within LDS and latent_dim / 32 <= 32 accumulators per thread, i.e. latent_dim <= 1024; FD_EINVAL otherwise. */
int fd_rvq_chain_supported(int latent_dim, int codebook_dim);
int fd_rvq_encode_chain(fd_ndac* m, const float* z, const int* frames, int B, int T, int n_quantizers, float* z_q, int* codes,
                        float* latents, void* stream);
/* Encode of a RAGGED batch: x [B][L] (L % hop == 0), frames = DEVICE int32 [B], clip b = the first frames[b] * hop samples of its row,
 * 1 <= frames[b] <= L / hop (checked on the host before anything is launched: one B-int copy and a stream synchronisation; FD_EINVAL
 * leaves every output untouched).  Columns t < frames[b] of row b of z_q / codes / latents are BIT-IDENTICAL to fd_ndac_encode of that clip
 * alone (B = 1, L = frames[b] * hop) in the same precision mode; the columns behind are 0.  Every kernel bounds its input reads by the
 * clip's own length at that layer (frames[b] * hop / the strides so far), so what lies behind a clip -- in x or in the workspace -- is
 * never read as data.  The quantiser runs as one launch (fd_rvq_encode_chain; the per-quantiser kernels under the same table where
 * fd_rvq_chain_supported says no).  Workspace: fd_ndac_workspace_bytes(m, B, L), as fd_ndac_encode. */
int fd_ndac_encode_ragged(fd_ndac* m, const float* x, const int* frames, int B, int L, int n_quantizers, float* z_q, int* codes,
                          float* latents, void* ws, size_t ws_bytes, void* stream);
/* Latent frames before (left) and after (right) a frame whose samples can reach that frame -- the receptive field of the encoder in
 * frames, from the configuration alone (host only): rates (2,4,8,10) give (7, 7), (2,4,8,8) give (8, 8).  A window of whole hops with
 * this much real context on both sides (or a true edge of the signal) encodes its interior frames to the bits of the one-shot encode
 * (flowdec_amd/ndac_stream.py); odd rates are fine here (a shift by whole frames keeps every layer's phase).  FD_EINVAL when the rates
 * do not give n frames for n hops of samples (a rate of 1). */
int fd_ndac_encode_halo(const fd_ndac* m, int* left, int* right);
/* dac.DAC.decode: z [B][latent][T] -> audio [B][fd_ndac_decoded_length(T)] in (-1, 1) */
int fd_ndac_decode(fd_ndac* m, const float* z, int B, int T, float* audio, void* ws, size_t ws_bytes, void* stream);
/* Decode of a RAGGED batch: z [B][latent][T], frames = DEVICE int32 [B] (like the lengths of fd_enhance_ragged), clip b = the first
 * frames[b] frames of its row, 1 <= frames[b] <= T (checked on the host before anything is launched: one B-int copy and a stream
 * synchronisation; FD_EINVAL leaves audio untouched).  audio [B][fd_ndac_decoded_length(T)]: samples [0, fd_ndac_decoded_length(
 * frames[b])) of row b are BIT-IDENTICAL to fd_ndac_decode of that clip alone (B = 1, T = frames[b]) in the same precision mode, the
 * rest of the row is 0.  Every kernel bounds its input reads by the clip's own length at that layer (an affine function of
 * frames[b], odd rates included), so what lies behind a clip in the workspace is never read as data.  Workspace: as fd_ndac_decode. */
int fd_ndac_decode_ragged(fd_ndac* m, const float* z, const int* frames, int B, int T, float* audio, void* ws, size_t ws_bytes,
                          void* stream);
/* Latent frames before (left) and after (right) a frame that can influence that frame's hop output samples -- the receptive field
 * of the decoder in frames, from the configuration alone (host only).  A window of frames with this much real context on both sides
 * (or a true edge of the signal) decodes its interior to the bits of the one-shot decode (flowdec_amd/ndac_stream.py).
 * FD_EINVAL, naming the rate, when a decoder rate is odd: the decoded length is then not frames * hop. */
int fd_ndac_decode_halo(const fd_ndac* m, int* left, int* right);
/* ---- Codec pools: many streaming sessions through one native call per step (session layer: flowdec_amd/ndac_pool.py) -----------------
 * A session's output is, bit for bit, the one-shot decode / encode of everything it was given, however that was cut into pushes and
 * whichever other sessions shared its native calls (the windows are ndac_stream.DecodePlanner's; a ragged row is its one-clip result).
 * One step = one table upload and ONE call, whose launch count does not depend on the number of rows:
 *   decode: gather (code rings -> z_q, from_codes fused in, per-row nq; the device frame table) -> the decoder layers of
 *           fd_ndac_decode_ragged under that table -> emit (the final samples of every row -> out)
 *   encode: gather (sample rings -> x; the frame table) -> the encoder layers and the quantiser of fd_ndac_encode_ragged with the call's
 *           n_quantizers -> emit (the first nq code rows of the final frames -> out)
 * Both read ONE DEVICE table, an entry per row of the call; a session may have several rows in a call (rows are independent).  The call
 * checks the caller's HOST copy of the same table -- every rule below, before anything is launched: FD_EINVAL leaves every output
 * untouched -- so there is no copy back to the host and no stream synchronisation; no atomics.  What lies outside a row's window, in a
 * ring or in the workspace, is never read as data. */
typedef struct fd_ndac_pool_row {
  const void* ring;     /* decode: int32 codes [n_codebooks][ring_cap], frame i of code row q at ring[q * ring_cap + i % ring_cap]
                         * encode: float32 samples [ring_cap], absolute sample i at ring[i % ring_cap] */
  long long start;      /* absolute first frame (decode) / first sample (encode) of the window, >= 0; the window may wrap the ring */
  int ring_cap;         /* >= frames (decode) / frames * hop (encode) */
  int frames;           /* window length in frames, 1 .. T */
  int nq;               /* code rows of this session, 1 .. n_codebooks (decode: summed as fd_rvq_from_codes sums them) / 1 .. n_quantizers
                         * (encode: rows emitted; quantiser i does not depend on the later ones, so these are the session's own encode) */
  int emit_lo, emit_count;   /* window-local frames that are final: emit_lo >= 0, emit_count >= 0, emit_lo + emit_count <= frames */
  void* out;            /* decode: float32 [emit_count * samples per frame]; encode: int32 [nq][emit_count] */
} fd_ndac_pool_row;
/* Bytes of a step of B rows of at most T frames, either direction (0 for a bad B or T). */
size_t fd_ndac_pool_workspace_bytes(const fd_ndac* m, int B, int T);
/* use_graph != 0: the step is one linear chain, so after one eager call with the same (B, T, n_quantizers, precision, table_dev, ws) it is
 * captured once as a hipGraph and replayed -- the table's content is read at run time and is not part of the graph, so upload it before
 * the call; the same bits either way.  Capture is illegal on the legacy default stream.  fd_ndac_pool_decode refuses odd decoder rates
 * (fd_ndac_decode_halo's message), fd_ndac_pool_encode an encoder rate of 1 (fd_ndac_encode_halo's).  The precision mode is the codec's
 * (fd_ndac_set_precision). */
int fd_ndac_pool_decode(fd_ndac* m, const fd_ndac_pool_row* table_dev, const fd_ndac_pool_row* table_host, int B, int T, void* ws,
                        size_t ws_bytes, int use_graph, void* stream);
int fd_ndac_pool_encode(fd_ndac* m, const fd_ndac_pool_row* table_dev, const fd_ndac_pool_row* table_host, int B, int T, int n_quantizers,
                        void* ws, size_t ws_bytes, int use_graph, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Evaluation metrics: the two metrics of the reference's evaluation (flowdec/eval/metrics.py) that need no outside model, over ragged
 * batches -- what scores a `triples_list.txt` (flowdec_amd/eval_cli.py).  Rows [B][L] float32 on the device; lengths: DEVICE int32 [B],
 * clip b is the first lengths[b] samples of its row (samples behind it are never read).  All three calls are asynchronous on `stream`,
 * allocate nothing and launch nothing when they refuse.  A clip's result has the SAME BITS alone, in a batch, at any batch position and
 * next to clips of any other lengths: every partition and order of summation depends on the clip's own length only; no atomics.
 * ws: fd_metrics_workspace_bytes(B, L, n_fft, hop) bytes (covers all three; n_fft <= 0: fd_metrics_sisxr only; 0 for a bad B or L).
 * A NULL pointer, a bad shape and a workspace that is too small are all FD_EINVAL here, with a message.
 *
 * fd_metrics_sisxr: SI-SDR / SI-SIR / SI-SAR (eval/metrics.py:256-270, :554-563) of estimate x_hat against reference x with degraded
 *   input y, in float64, two passes.  The noise is n = y - x, or y + x when that has less power (the reference's phase-flip guard;
 *   decided as x.y < 0); alpha_s = x_hat.x / x.x, alpha_n = x_hat.n / n.n; per sample s_target = alpha_s x, e_noise = alpha_n n,
 *   e_art = x_hat - s_target - e_noise.  sums_out: DEVICE double [B][8] =
 *     [0] x.x  [1] x_hat.x  [2] x_hat.n  [3] n.n  [4] |s_target|^2  [5] |e_noise|^2  [6] |e_art|^2  [7] |e_noise + e_art|^2
 *   and the caller forms  si_sdr = 10 log10([4] / [7]),  si_sir = 10 log10([4] / [5]),  si_sar = 10 log10([4] / [6])  in float64.
 *   A length is clamped into [0, L]; an empty clip gives zero sums.
 * fd_metrics_logspec_mse: LogSpecMSE (eval/metrics.py:333-372): mean over all bins and frames of (10 log10 max(|X_hat|^2, eps) -
 *   10 log10 max(|X|^2, eps))^2 of the one-sided power spectrograms of the plan's transform -- the reference's is
 *   fd_stft_plan_create(1536, 384) at 48 kHz: symmetric Hann, center = True with reflect padding, T_b = 1 + lengths[b] / hop frames --,
 *   |X|^2 in float32, everything after it in float64.  mse_out: DEVICE double [B].  L <= n_fft / 2 (torch.stft raises: the clip cannot be
 *   reflect-padded) is FD_EINVAL; a DEVICE length outside (n_fft / 2, L] cannot be seen by the host and gives NaN for that clip (no
 *   out-of-bounds access).
 * fd_metrics_power_spec (operator level, for tests): P_out DEVICE float [B][1 + L / hop][n_fft / 2 + 1] = re^2 + im^2 exactly as the
 *   call above forms it, zero in the frames t >= T_b.
 * ---------------------------------------------------------------------------------------------- */
size_t fd_metrics_workspace_bytes(int B, int L, int n_fft, int hop);
int fd_metrics_sisxr(const float* x_hat, const float* x, const float* y, const int* lengths, int B, int L, double* sums_out, void* ws,
                     size_t ws_bytes, void* stream);
int fd_metrics_logspec_mse(const fd_stft_plan* plan, const float* x_hat, const float* x, const int* lengths, int B, int L, double eps,
                           double* mse_out, void* ws, size_t ws_bytes, void* stream);
int fd_metrics_power_spec(const fd_stft_plan* plan, const float* x, const int* lengths, int B, int L, float* P_out, void* ws, size_t ws_bytes,
                          void* stream);

/* Alignment in time (still "Evaluation metrics": what eval_cli --align runs before it scores; csrc/xcorr.hip, host yardstick and the
 * definition in flowdec_amd/align.py).  The bounded-lag cross-correlation of every pair of a ragged batch and the lag of its peak:
 *     c[b][l + M] = sum_n a_b[n] b_b[n + l],   l in [-M, M],   n over max(0, -l) <= n < min(la, lb - l),   M = max_lag
 * with la, lb the clip's own lengths; an empty range gives exactly 0.0; a peak at l > 0 means b is a delayed by l samples.  a DEVICE
 * float [B][La], b DEVICE float [B][Lb] (the two signals of a pair may differ in length); lens_a, lens_b DEVICE int32 [B], each clamped
 * into its row.  Samples outside [0, len) of a clip are zeros by definition and are never loaded, neither from the row's tail nor from
 * the next row.  The samples are finite float32, so every product is exact in float64; the sums are float64.  The same contract as
 * above: a clip's c and lag have the SAME BITS alone, in a batch, at any batch position and next to clips of any other lengths -- every
 * partition and order of addition is a function of (lens_a[b], lens_b[b], max_lag) only (per lag the products of a slice of 32768
 * samples of a in ascending order, four per v_mfma_f64_16x16x4_f64; the slice of lag l starts (l + max_lag) % 16 samples before a
 * multiple of 32768; the slices added in index order); no atomics.
 * lags DEVICE int32 [B]: the l with the largest c, NaN counting as -inf; among equal maxima the smallest |l|, and of -l and +l it is
 *   +l (so two silent signals give 0), picked on the device from the finished float64 values.  c DEVICE double [B][2 M + 1] or NULL.
 * fd_xcorr_workspace_bytes: 0 for a bad argument.  fd_xcorr_lags is asynchronous on `stream`, allocates nothing and launches nothing
 *   when it refuses: FD_EINVAL with a message for a NULL pointer (c alone may be NULL), B outside [1, 65535], max_lag outside
 *   [1, 1 << 20] and a row length outside [1, 0x7fffffff - 1024]; FD_ENOMEM for a workspace that is too small. */
size_t fd_xcorr_workspace_bytes(int B, int La, int Lb, int max_lag);
int fd_xcorr_lags(const float* a, const float* b, const int* lens_a, const int* lens_b, int B, int La, int Lb, int max_lag, double* c, int* lags,
                  void* ws, size_t ws_bytes, void* stream);

/* The same peak on a grid of 1 / Q samples, with polarity (align.py refine_lag; eval_cli --align-frac / --align-polarity and the --align
 * of estimate_cli and loss_cli).  bank DEVICE double [Q][2 W]: the host's table of Hann-windowed sinc interpolators (align.frac_bank: row
 * j, column t is the tap k = t - W + 1 of the delay j / Q; row 0 the unit impulse) -- the device only reads it and evaluates no
 * transcendental.  c is fd_xcorr_lags' c, bit for bit (the same slice kernel and the same order of the slice sums).  l0 is picked by the
 * rule above on |c| when polarity != 0, else on c; sign = -1 when polarity != 0 and c[l0] < 0, else +1.  Then one workgroup per clip
 * evaluates, for q in [-(Q - 1), Q - 1] with |l0 Q + q| <= max_lag Q,
 *     r(q) = sum_{k = -W + 1 .. W} (sign c[l0 + floor(q / Q) + k]) bank[q mod Q][k + W - 1]
 * k ascending, every product and sum rounded to float64 on its own (no fused multiply-add), indices outside [-M, M] left out, a NaN r
 * counting as -inf, and picks the largest r; ties go to the smallest |q|, then to +q (all -inf: q = 0).
 * lag_q DEVICE int64 [B] = l0 Q + q (the lag is lag_q / Q samples); sign DEVICE int32 [B]; c DEVICE double [B][2 M + 1] or NULL.
 * The promises of fd_xcorr_lags hold: asynchronous on `stream`, no allocation, no atomics, a clip's c, lag_q and sign have the same bits
 * alone and in any batch, nothing launched on a refusal: FD_EINVAL with a message for a NULL pointer (c alone may be NULL; a NULL bank
 * is named), B, max_lag and the row lengths as above, Q outside [2, 1024], W outside [1, 256]; FD_ENOMEM for a workspace smaller than
 * fd_xcorr_frac_workspace_bytes (0 for a bad argument). */
size_t fd_xcorr_frac_workspace_bytes(int B, int La, int Lb, int max_lag);
int fd_xcorr_lags_frac(const float* a, const float* b, const int* lens_a, const int* lens_b, int B, int La, int Lb, int max_lag, const double* bank,
                       int Q, int W, int polarity, double* c, long long* lag_q, int* sign, void* ws, size_t ws_bytes, void* stream);

/* fd_frac_shift (csrc/fracshift.hip; align.py frac_shift): a ragged batch of signals moved by base + j / Q samples and multiplied by sign.
 * s DEVICE float [B][Ls], lens DEVICE int32 [B] (clamped into the row); per clip base DEVICE int32 [B], its tap row taps DEVICE double
 * [B][2 W] (bank[j]), sign DEVICE int32 [B] (negative: -1, else +1) and the output window n0, n1 DEVICE int32 [B]:
 *     out[b][i] = f32(sign_b * sum_{k = -W + 1 .. W} f64(s_b[n0_b + i + base_b + k]) * taps_b[k + W - 1]),   0 <= i < n1_b - n0_b
 * k ascending, products and sums separately rounded float64, one rounding to float32; samples outside [0, len) are zeros and are never
 * loaded; out DEVICE float [B][Lo], zeros behind the window (a window longer than Lo is cut to it).  Every index is clamped: a wrong
 * table gives wrong samples, never an access outside a row.  Asynchronous, no allocation, no workspace, no atomics; a clip's samples
 * have the same bits alone and in any batch.  FD_EINVAL with a message (nothing launched) for a NULL pointer, B outside [1, 65535], a
 * row length outside [1, 0x7fffffff - 1024] and W outside [1, 256]. */
int fd_frac_shift(const float* s, const int* lens, int B, int Ls, const int* base, const double* taps, int W, const int* sign, const int* n0,
                  const int* n1, float* out, int Lo, void* stream);

/* Loudness (still "Evaluation metrics": eval_cli --loudness / --match-loudness and loudness.LoudnessMeter; csrc/loudness.hip, host
 * yardstick and the definition in flowdec_amd/loudness.py).  The integrated loudness of ITU-R BS.1770-4 / EBU R 128 of every clip of a
 * ragged batch of MONO signals at 48 kHz: the K-weighting (the standard's two biquads at 48 kHz, a recursive filter in float64), the
 * energies E[j] of the filtered signal over the sub-blocks [4800 j, 4800 (j + 1)), gating blocks of four sub-blocks
 * (ms_j = (((E[j] + E[j+1]) + E[j+2]) + E[j+3]) / 19200) and the two gates, both taken on the mean squares (no logarithm decides a
 * comparison): ms_j > 10^((-70 + 0.691) / 10), then ms_j > 0.1 * the mean of the blocks above the first gate.  LUFS = -0.691 +
 * 10 log10(ms_gated) is formed by the caller.  Only whole sub-blocks are read: the last len mod 4800 samples of a clip, the row behind
 * it and the next row are never loaded.  The filter runs parallel in time (chunks of 75 samples, 64 to a sub-block, one lane each; the
 * chunk and sub-block states joined through the tabulated zero-input transitions) in an order of operations that csrc/loudness.hip and
 * loudness.py state and that depends on the clip's own length only: a clip's E, ms and counts have the SAME BITS alone, in a batch, at
 * any batch position, and cut at any multiple of 4800 samples into calls that hand the state on.  No atomics, no fused multiply-add.
 *   x DEVICE float [B][L]; lengths DEVICE int32 [B], clamped to [0, L]; Jmax = L / 4800 (0 is allowed: nothing is filtered).
 *   fd_loudness_energies: E_out DEVICE double [B][Jmax] (E_out[b][j] = 0.0 for j >= nsub_b; NULL only when Jmax = 0); nsub_out DEVICE
 *     int32 [B] = len_b / 4800; state DEVICE double [B][4] in/out: the filter state at the clip's sample 0 on entry and after its last
 *     whole sub-block on return (what a stream hands to its next call), or NULL = the zero state, nothing written back.
 *   fd_loudness_gate: E DEVICE double [B][Jmax], nsub DEVICE int32 [B] (clamped to [0, Jmax]) -> ms_out DEVICE double [B] (ms_gated) and
 *     counts_out DEVICE int32 [B][3] = blocks, blocks above the absolute gate, blocks above both.  Fewer than four sub-blocks: NaN and
 *     0 0 0.  A block that is NaN or Inf (a NaN or Inf sample in a sub-block that was read): NaN and (blocks, 0, 0).  No block above the
 *     absolute gate: 0.0 (-inf LUFS) and (blocks, 0, 0).
 *   fd_loudness: the two in one call, E and nsub in the workspace.
 *   fd_loudness_workspace_bytes(B, L): what both calls need (never 0 for a good shape); 0 for a bad argument.
 *   fd_loudness_tables: HOST double [16] + [16] + [1]: the two transition matrices (75 and 4800 samples, row-major) and the absolute gate
 *     as the library holds them (tests compare them with loudness.py's, bit for bit); no device is touched.
 * All calls are asynchronous on `stream`, allocate nothing and launch nothing when they refuse: FD_EINVAL with a message for a NULL
 * pointer, B outside [1, 65535], L outside [1, 0x7fffffff - 1024] (Jmax outside [0, (0x7fffffff - 1024) / 4800]) and a workspace that is
 * not 8-byte aligned; FD_ENOMEM for a workspace that is too small. */
int fd_loudness_tables(double* chunk16, double* sub16, double* abs_gate);
size_t fd_loudness_workspace_bytes(int B, int L);
int fd_loudness_energies(const float* x, const int* lengths, int B, int L, double* state, double* E_out, int* nsub_out, void* ws, size_t ws_bytes,
                         void* stream);
int fd_loudness_gate(const double* E, const int* nsub, int B, int Jmax, double* ms_out, int* counts_out, void* stream);
int fd_loudness(const float* x, const int* lengths, int B, int L, double* ms_out, int* counts_out, void* ws, size_t ws_bytes, void* stream);

/* True peak (ITU-R BS.1770-4 Annex 2) and loudness range (EBU Tech 3342): csrc/loudness_range.hip; the host yardsticks and the definitions
 * are loudness.py true_peak_lin and range_of.  eval_cli --true-peak / --loudness-range, loudness.loudness_report_batch and
 * loudness.LoudnessMeter run on them.  Both calls are asynchronous on `stream`, allocate nothing, use no floating-point atomics and no
 * fused multiply-add; a clip's results have the SAME BITS alone, in a batch and at any batch position; nothing is launched on a refusal:
 * FD_EINVAL with a message for a NULL pointer, B outside [1, 65535], L outside [1, 0x7fffffff - 1024], Jmax outside [0, (0x7fffffff -
 * 1024) / 4800] and W outside [1, 256]; FD_ENOMEM for a workspace smaller than the *_workspace_bytes function gives (0 for a bad argument).
 *
 * fd_true_peak: x DEVICE float [B][L] at 48 kHz, lengths DEVICE int32 [B] (clamped to [0, L]); lo, hi DEVICE int32 [B]: the positions
 *   [lo_b, hi_b) of clip b (clamped into [0, len_b]), or both NULL: every position; taps DEVICE double [4][2 W]: the host's table of a 4x
 *   oversampling interpolator (align.frac_bank(4, W): row j, column t is the tap k = t - W + 1 of the delay j / 4; row 0 the unit
 *   impulse, so the sample peak is included) -- the device only reads it and evaluates no transcendental.
 *       p_out[b] = max over n in [lo_b, hi_b), j in 0..3 of | sum_{t = 0 .. 2W-1} f64(x_b[n + t - W + 1]) * taps[j][t] |
 *   p_out DEVICE double [B]; t ascending, every product and sum rounded to float64 on its own; samples outside [0, len_b) are zeros and
 *   are never loaded, every index is clamped: a wrong table or window gives a wrong number, never an access outside a row.  A sum that
 *   is not finite (a NaN or Inf sample among those the window reads): NaN.  An empty clip: NaN.  An empty window of a clip that is not
 *   empty: 0.0.  dBTP = 20 log10(p) is formed by the caller.  fd_true_peak_tile(): the positions one workgroup owns (tests put lengths
 *   and windows around its multiples).
 * fd_loudness_range: E DEVICE double [B][Jmax] and nsub DEVICE int32 [B] (clamped to [0, Jmax]) as fd_loudness_gate takes them.  Short-
 *   term windows st_j = (((E[j] + E[j+1]) + ...) + E[j+29]) / 144000 for j = 0 .. nsub - 30 (kept in the workspace); the absolute gate
 *   st_j > 10^((-70 + 0.691) / 10); the relative gate st_j > 0.01 * the mean of the windows above the first (the sum in fd_loudness_gate's
 *   order: 64 lane sums, added in ascending lane order); with m windows above both and s their ascending order,
 *       st_out[b] = (s[((m - 1) * 10 + 50) / 100], s[((m - 1) * 95 + 50) / 100])     (DEVICE double [B][2], exact order statistics by a
 *   radix select on the 64-bit patterns, linear in the number of windows); counts_out DEVICE int32 [B][3] = windows, windows above the
 *   absolute gate, windows above both.  LRA = 10 log10(st_hi) - 10 log10(st_lo) is formed by the caller.  Fewer than 30 sub-blocks: NaN
 *   NaN and 0 0 0.  A window that is NaN or Inf: NaN NaN and (windows, 0, 0).  No window above the absolute gate: 0.0 0.0 (0 LU by
 *   definition) and (windows, 0, 0). */
int fd_true_peak_tile(void);
size_t fd_true_peak_workspace_bytes(int B, int L);
int fd_true_peak(const float* x, const int* lengths, int B, int L, const int* lo, const int* hi, const double* taps, int W, double* p_out,
                 void* ws, size_t ws_bytes, void* stream);
size_t fd_loudness_range_workspace_bytes(int B, int Jmax);
int fd_loudness_range(const double* E, const int* nsub, int B, int Jmax, double* st_out, int* counts_out, void* ws, size_t ws_bytes, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Parameter estimation: the statistics behind a FlowDec model's beta and sigma_y (the reference's scripts/estimate_flowdec_params.py;
 * flowdec_amd/estimate.py, flowdec_amd/estimate_cli.py).  Both calls are asynchronous on `stream`, allocate nothing, keep no state and
 * launch nothing when they refuse; a NULL pointer, a bad shape and a workspace that is too small are FD_EINVAL with a message.
 *
 * fd_estimate_pair_stats: x (clean) and y (coded) are DEVICE float [B][L], every pair already cropped or padded to the one length L (not
 *   ragged).  Per pair: normfac = max|y| + 1e-5 in float32 (the script's normalize_noisy: NO zero guard, unlike enhance's rule); x and y
 *   divided by it sample by sample in float32; the plan's transform (symmetric Hann, reflect-centred, T = 1 + L / hop frames) of both;
 *   amplitude compression |.|^alpha e^{j angle} with beta = 1 of both (fd_stft_compress's arithmetic, bit for bit).
 *     normfac_out  DEVICE float [B]
 *     absx_out     DEVICE float [B][F][T], F = n_fft / 2 + 1: |X_c| of the compressed CLEAN spectrum, formed from its float32 parts as
 *                  (float) sqrt((double) re^2 + (double) im^2) (both roundings IEEE).  May be NULL.
 *     band_sq_out  DEVICE double [B][F]: sum over t of |Y_c - X_c|^2, the difference per component in float32 (complex64 subtraction),
 *                  squared and summed in float64 in a fixed order that depends on T only; no floating-point atomics.
 *   A pair's three outputs have the SAME BITS alone, in a batch and at any batch position.
 *   ws: fd_estimate_workspace_bytes(B, L, n_fft, hop) bytes (0 for a bad argument).
 * fd_select_f32: exact order statistics of n non-negative DEVICE float values: out[r] (DEVICE float [R]) is bit for bit the value at
 *   position ranks[r] of the sorted array.  ranks: HOST long long [R], 1 <= R <= 8, each in [0, n); 1 <= n <= 2^40, every count 64-bit.
 *   A most-significant-digit radix select on the bit pattern (monotone for non-negative floats, denormals and +inf included), four
 *   passes of 8 bits, integer atomics only, no host synchronisation between the passes; `values` is only read.  -0.0 counts as +0.0 (and
 *   comes out as +0.0).  Every other value with the sign bit set and every NaN is counted in bad_out (DEVICE int64, written by every
 *   call); the caller treats a non-zero count as an error, `out` is then meaningless.
 *   ws: fd_select_workspace_bytes(R) bytes (0 for a bad R).
 * ---------------------------------------------------------------------------------------------- */
size_t fd_estimate_workspace_bytes(int B, int L, int n_fft, int hop);
int fd_estimate_pair_stats(const fd_stft_plan* plan, const float* x, const float* y, int B, int L, float alpha, float* normfac_out,
                           float* absx_out, double* band_sq_out, void* ws, size_t ws_bytes, void* stream);
size_t fd_select_workspace_bytes(int R);
int fd_select_f32(const float* values, long long n, const long long* ranks, int R, float* out, long long* bad_out, void* ws, size_t ws_bytes,
                  void* stream);

/* ----------------------------------------------------------------------------------------------
 * Validation loss: the quantity the reference's validation_step logs as `valid_loss` (flowdec/model.py:221-223; `_loss` of FlowModel
 * :421-468, ScoreModel :590-611, RegressionModel :552-559) for (clean, coded) pairs -- one front end on the pair, the random draws, ONE
 * network evaluation at a random time and per-clip sums of squared errors.  No gradient, no optimiser.  flowdec_amd/loss.py drives these
 * calls; csrc/loss.hip holds the kernels.  Every call is asynchronous on `stream`, allocates nothing and launches nothing when it
 * refuses; a NULL pointer, a bad shape and a workspace that is too small are FD_EINVAL with a message that names the argument.
 *
 * fd_loss_config: kind = FD_LOSS_FLOW / FD_LOSS_SCORE / FD_LOSS_REGRESSION; sigma_x (flow: the scalar sigma_x of the model, >= 0);
 *   theta, sigma_min, sigma_max, t_eps (score: OUVESDE and ScoreModel.t_eps).  fd_loss_num_draws: the Gaussian planes a kind consumes:
 *   flow 1, or 2 with sigma_x != 0; score 1; regression 0 (-1 for a NULL cfg or an unknown kind).
 *
 * fd_loss_times: t_out[b] (DEVICE float [B]) = lo + u[b] * (hi - lo) in float32 (product and sum rounded separately, as
 *   torch.rand(B) * (T - t_eps) + t_eps), u[b] = (r0 >> 8) * 2^-24 with r0 from Philox4x32-10, key = seeds[b] (DEVICE uint64 [B]), counter
 *   (0, 0, 0, 1) -- value 1 of the reserved counter word of "Seeded noise" (NORMATIVE).  (lo, hi) = (0, 1) for flow, (t_eps, 1) for score;
 *   0 <= lo < hi <= 1.  Every value lies in [lo, hi] and below hi unless the float32 sum rounds up to it.
 *
 * fd_loss_state: Y, X = complex64 [B][1][F][T_pad] (the compressed spectrograms, zero tail as fd_stft_compress_ragged leaves it), t =
 *   DEVICE float [B] -> xt_out (the network input) and target_out, both complex64 [B][1][F][T_pad], in one pass.  Exactly one of noise
 *   (complex64 [fd_loss_num_draws][B][F][T_pad]) and seeds (DEVICE uint64 [B]: draw k is draw index k of "Seeded noise") is given; the
 *   seeded form equals the buffer form on fd_noise_fill's planes bit for bit.  Every product and sum below is rounded to float32 on its
 *   own (no fused multiply-add), per component:
 *     flow        Ys = Y + (float)(sigma_y[f] * (double)z0) -- fd_ode_solve's x0 with sigma_fac = 1, bit for bit, padded frames included
 *                 (randn_like(Ymu) covers them);  Xs = X + sigma_x * z1, or X itself when sigma_x == 0 (no draw is consumed);
 *                 xt = t * Xs + (1 - t) * Ys with 1 - t rounded once;  target = Ut = Xs - Ys.  (ConditionalFlowMatcher with sigma = 0.)
 *                 sigma_y = DEVICE double [sigma_n], sigma_n = 1 or F.  ys_out (optional) receives Ys.
 *     score       e = expf(-theta t), mean = e * X + (1 - e) * Y, std = the OUVE closed form fd_score_* uses (sdes.py:183-196) evaluated
 *                 in float32 on the device at the clip's t;  xt = mean + z0 * std;  target = z0;  std_out (optional, DEVICE float [B]).
 *     regression  xt = Y, target = X (t, noise, seeds are not read; the network runs at t = 0).
 * fd_loss_sqerr: V (the network output), target: complex64 [B][1][F][T_pad]; std DEVICE float [B] (score only).  err per component in
 *   float32 as the reference forms it -- flow V - Ut; score std * ((-V / std) - (-z0 / std)); regression V - X -- then
 *   sums_out[b] (DEVICE double) = sum over the clip of (double)re^2 + (double)im^2, and bad_out[b] (DEVICE int64) = its number of elements
 *   with a non-finite component.  Two stages in a fixed order that depends on F * T_pad only; no floating-point atomics; a clip's sum
 *   has the SAME BITS alone, in a batch and at any batch position.  ws: fd_loss_sqerr_workspace_bytes(B, F, T_pad) (0 for a bad shape).
 *
 * fd_valid_loss: x (clean), y (coded) = DEVICE float [B][L] rows; lengths = DEVICE int32 [B] of ONE T_pad bucket (the contract of
 *   fd_enhance_ragged) or NULL: every pair is L samples long.  The front end is EnhancementModel._preprocess(y, x=x): normfac from y
 *   with enhance's zero guard (fd_normfac's rule; NOT fd_estimate_pair_stats' + 1e-5), x divided by the same factor, both transformed,
 *   compressed and zero-padded to T_pad.  Then fd_loss_state, fd_ncsnpp_forward at the per-clip times (regression: t = 0, input Y) and
 *   fd_loss_sqerr.
 *     noise / seeds  exactly one for flow and score (noise = complex64 [fd_loss_num_draws][B][F][T_pad]); regression reads neither.
 *     t              DEVICE float [B], or NULL: drawn from `seeds` as fd_loss_times does, over [0, 1) (flow) / [t_eps, 1) (score);
 *                    NULL without seeds is FD_EINVAL.  Regression ignores it.
 *     sums_out       DEVICE double [B]: sum |err|^2 of clip b over its F * T_pad bins.  The HOST turns the sums into the loss: flow
 *                    mean_b(sums[b] / (F T_pad)) with NaN clips dropped; score 0.5 mean_b sums[b]; regression sum_b sums[b] / (B F T_pad).
 *     bad_out        DEVICE int64 [B];  normfac_out DEVICE float [B].
 *     B              at most 256 clips (the per-sample time table of the network).
 *   Clip b's three outputs have the SAME BITS alone, in a batch and at any batch position.
 *   ws: fd_valid_loss_workspace_bytes(m, B, L) bytes (0 for a bad shape).
 * ---------------------------------------------------------------------------------------------- */
#define FD_LOSS_FLOW 0
#define FD_LOSS_SCORE 1
#define FD_LOSS_REGRESSION 2
typedef struct fd_loss_config {
  int kind;
  float sigma_x;
  float theta, sigma_min, sigma_max, t_eps;
} fd_loss_config;
int fd_loss_num_draws(const fd_loss_config* cfg);
int fd_loss_times(const unsigned long long* seeds, int B, float lo, float hi, float* t_out, void* stream);
int fd_loss_state(const fd_loss_config* cfg, const float* Y, const float* X, const float* t, const float* noise, const unsigned long long* seeds,
                  const double* sigma_y, int sigma_n, float* xt_out, float* target_out, float* std_out, float* ys_out, int B, int F, int T_pad,
                  void* stream);
size_t fd_loss_sqerr_workspace_bytes(int B, int F, int T_pad);
int fd_loss_sqerr(int kind, const float* V, const float* target, const float* std, double* sums_out, long long* bad_out, int B, int F, int T_pad,
                  void* ws, size_t ws_bytes, void* stream);
size_t fd_valid_loss_workspace_bytes(const fd_model* m, int B, int L);
int fd_valid_loss(fd_model* m, const fd_loss_config* cfg, const float* x, const float* y, const int* lengths, const float* noise,
                  const unsigned long long* seeds, const float* t, double* sums_out, long long* bad_out, float* normfac_out, int B, int L, void* ws,
                  size_t ws_bytes, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Resampling: torchaudio.functional.resample (sinc_interp_hann) as a polyphase FIR on the device, with an order of summation that is
 * part of the contract (flowdec_amd/resample.py; csrc/resample.hip).  With o = orig / gcd, n = new / gcd, f = min(o, n) * rolloff,
 * width = ceil(lowpass_filter_width * o / f) and K = 2 width + o, the bank is h[n][K] float32,
 *     t = clamp((k' / o - i / n) f, -lpw, lpw),  h[i][k' + width] = sinc(t) cos^2(pi t / (2 lpw)) f / o,   k' in [-width, width + o)
 * computed in float64 and rounded once.  The CALLER supplies it (flowdec_amd.enhance_cli.sinc_resample_kernel): the library has no
 * generator, so the bits are those of the pinned host restatement.  An input of L samples has M = ceil(n L / o) outputs; output
 * m = q n + i (0 <= i < n) is
 *     acc = 0.0 (double);  for k = 0 .. K-1 ascending:  j = q o + k - width;  if 0 <= j < L: acc += (double)h[i][k] * (double)x[j]
 *     y[m] = (float)acc                                   one rounding, to nearest even
 * The product of two float32 values is exact in float64, so the float64 add is the loop's only rounding and a fused multiply-add
 * gives the same bits; a tap outside [0, L) may equally be multiplied by a zero (acc starts at +0.0).  One thread owns an output's
 * whole sum -- no matrix instruction, no atomics, no split K -- so an output has the SAME BITS alone, in a batch, at any batch
 * position and in any span of a stream, and a plain float64 loop on the host reproduces it.  Inputs are finite float32.
 *
 * fd_resample_plan_create: bank_host is HOST float [n][K]; it is uploaded synchronously here (in a layout of the kernel's choosing)
 *   and nothing on the call path allocates.  Checked before any HIP call, FD_EINVAL otherwise: o, n >= 1, width >= 0, bank_host and out
 *   non-NULL, n K <= 2^24 (a pair like 47999 -> 48000 would ask for a 9 GB bank).
 * fd_resample_out_length: ceil(n L / o) in 64 bits, host only (-1 for L < 0 or o, n < 1).
 * fd_resample: the ragged batch.  x DEVICE float [B][L]; lengths DEVICE int32 [B] (row b is its first lengths[b] samples, clamped
 *   into [0, L]) or NULL: every row has L samples; y DEVICE float [B][L_out]: row b's ceil(n len_b / o) outputs followed by zeros.
 *   L_out < ceil(n L / o) is FD_EINVAL (checked from L: device lengths cannot be seen); 1 <= B <= 65535.
 * fd_resample_span: the streaming building block.  x DEVICE float [nx] holds the samples [x0, x0 + nx) of a recording of `total`
 *   samples (-1: not known yet, L = +infinity in the formula); the call writes the outputs [m0, m0 + count) of the recording's resampled
 *   signal to y[0 .. count).  x0, total, m0, count are absolute 64-bit indices (each at most 2^46).  FD_EINVAL, from the integers alone:
 *   a span that reads a sample outside [x0, x0 + nx) that is neither below 0 nor at or beyond a known total; m0 + count beyond
 *   ceil(n total / o) of a known total.  count = 0 is a no-op.
 * Both calls are asynchronous on `stream` and launch nothing when they refuse.
 * ---------------------------------------------------------------------------------------------- */
typedef struct fd_resample_plan fd_resample_plan;
int fd_resample_plan_create(const float* bank_host, int o, int n, int width, fd_resample_plan** out);
void fd_resample_plan_destroy(fd_resample_plan* plan);
long long fd_resample_out_length(long long L, int o, int n);
int fd_resample(const fd_resample_plan* plan, const float* x, const int* lengths, int B, int L, float* y, long long L_out, void* stream);
int fd_resample_span(const fd_resample_plan* plan, const float* x, long long x0, long long nx, long long total, long long m0, long long count,
                     float* y, void* stream);

/* ----------------------------------------------------------------------------------------------
 * ESTOI: the extended short-time objective intelligibility measure (Jensen & Taal 2016) of estimate x_hat against clean x, the metric
 * the reference computes as pystoi.stoi(x, x_hat, sr, extended=True) (flowdec/eval/metrics.py:273-283), over ragged batches
 * (csrc/stoi.hip; host yardstick and the algorithm in full: flowdec_amd/metrics.py estoi).  Rows [B][L] float32 on the device; lengths:
 * DEVICE int32 [B], clamped into [0, L]; samples behind a clip's end are never read.  The calls are asynchronous on `stream`, allocate
 * nothing and launch nothing when they refuse: a NULL pointer, a bad shape (1 <= B <= 65535, L >= 1, the resampled row at most 2^30
 * samples) and a workspace that is too small are FD_EINVAL with a message.  A clip's results have the SAME BITS alone, in a batch, at
 * any batch position and next to clips of any other lengths: every partition and order of summation depends on the clip's own length
 * only; no atomics.  Parity with the pystoi package itself is UNPINNED (the package is not available to the tests; scripts/pin_estoi.py
 * prints the comparison where it is); what is pinned is the host function, and this against it.
 *
 *   1. both signals to 10 kHz with the caller's resample plan (the pystoi bank: flowdec_amd.metrics.estoi_bank), fd_resample's
 *      arithmetic, rounded to float32; resample = NULL: the rows are at 10 kHz already
 *   2. frames of 256 samples at hop 128 starting below len - 256, window w = hanning(258)[1:-1]; frame t of x is kept iff
 *      (||w x_t|| + eps) > (max_t ||w x_t|| + eps) 10^-2 (40 dB), norms in float64, eps = 2^-52; the kept windowed frames of either signal
 *      are overlap-added at hop 128 in order (never stored: a gather), k kept frames give k - 1 spectral frames
 *   3. each spectral frame windowed again (formed in float64, rounded once to float32), the 512-point DFT bins 7..218 as an exact-float32
 *      fma chain in ascending sample order on the matrix cores, re^2 + im^2 in float32; 15 third-octave bands (edges 7 9 11 14 17 22 27
 *      34 43 55 69 87 109 138 174 219) summed in float64 in ascending bin order, square root, rounded to float32
 *   4. fewer than 30 spectral frames: 1e-5 (pystoi's value).  Else every block of 30 consecutive frames x 15 bands of either signal is
 *      normalised by row (mean over the frames removed, divided by the 2-norm) and then by column, in float64; a row or column whose sum
 *      of squares is exactly 0 becomes zeros (pystoi adds eps-sized noise instead: the one deliberate deviation);
 *      estoi = sum(x_n y_n) / 30 / segments.
 *
 * fd_estoi_plan_create: the window and the DFT table, uploaded synchronously; nothing on the call path allocates.
 * fd_metrics_estoi_workspace_bytes(B, L, o, n): o, n = the resample plan's rates over their gcd (orig, 10000), o = n = 1 without a
 *   resample plan; 0 for a bad argument.  fd_metrics_estoi_max_frames(L, o, n): T_max = max(1, frames of a clip of L samples).
 * fd_metrics_estoi: estoi_out DEVICE double [B]; frames_out DEVICE int32 [B][3] = frames, kept frames, spectral frames.
 * fd_metrics_estoi_bands (stage call, for tests): steps 1-3.  kept_out DEVICE int32 [B][T_max] = the source frame of every kept frame
 *   in order, -1 behind the clip's own count; tob_out DEVICE float [B][2][T_max][15] = the band magnitudes of x ([b][0]) and x_hat
 *   ([b][1]), zero behind the clip's own spectral frames.
 * ---------------------------------------------------------------------------------------------- */
typedef struct fd_estoi_plan fd_estoi_plan;
int fd_estoi_plan_create(fd_estoi_plan** out);
void fd_estoi_plan_destroy(fd_estoi_plan* plan);
size_t fd_metrics_estoi_workspace_bytes(int B, int L, int o, int n);
int fd_metrics_estoi_max_frames(int L, int o, int n);
int fd_metrics_estoi(const fd_estoi_plan* plan, const fd_resample_plan* resample, const float* x_hat, const float* x, const int* lengths, int B,
                     int L, double* estoi_out, int* frames_out, void* ws, size_t ws_bytes, void* stream);
int fd_metrics_estoi_bands(const fd_estoi_plan* plan, const fd_resample_plan* resample, const float* x_hat, const float* x, const int* lengths,
                           int B, int L, int* frames_out, int* kept_out, float* tob_out, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Spectral distances: the multi-scale STFT distance and the multi-scale mel distance between an estimate x_hat and a reference x (the
 * arithmetic of the reference's MultiScaleSTFTLoss and MelSpectrogramLoss, flowdec/losses.py, at their default parameters, as metrics
 * without gradients), over ragged batches (csrc/specdist.hip; host yardsticks and the definitions in full: flowdec_amd/specdist.py).
 * Rows [B][L] float32 on the device; lengths: DEVICE int32 [B]; samples behind a clip's end are never read.  A clip's results have the
 * SAME BITS alone, in a batch, at any batch position and next to clips of any other lengths: every partition and order of summation
 * depends on the clip's own length only; no atomics.  Parity of the mel filter bank with torchaudio's melscale_fbanks is UNPINNED (the
 * package is not available to the tests; scripts/pin_mel.py prints the comparison where it is).
 *
 * Per scale N (a power of two in [128, 4096]): one-sided STFT, center = True with reflect padding by N / 2, hop N / 4, periodic Hann
 * window w[k] = 0.5 - 0.5 cos(2 pi k / N), not normalised, T_b = 1 + lengths[b] / hop frames, F = N / 2 + 1 bins.  One workgroup
 * transforms the frames of both signals at once as z = w x_hat + i w x (each product rounded once) with an N-point complex FFT in LDS
 * (radix-2 decimation-in-time butterflies, two stages per LDS pass, float32, twiddles from the plan's table), separates A = |STFT(x_hat)|
 * and R = |STFT(x)| in float32, and forms in float64, with c = 1e-5:
 *     stft log   |2 log10(max(A, c) / max(R, c))|        stft mag   |A - R|        (scales with stft_term)
 *     mel log    |2 log10(max(M_hat, c) / max(M, c))|,   M = (float) sum_f fb[f][j] A_f^2 over the filter's own bins in ascending order,
 *                the products and the sum in float64                                                   (scales with n_mels > 0)
 * Per-frame sums in a fixed order, a clip's frames added in an order that depends on T_b only, divided by F T_b or n_mels T_b.
 * x_hat == x gives exactly 0 in every term (the transform's arithmetic is symmetric under the exchange of the two signals).
 *
 * fd_specdist_tables (HOST memory, no GPU needed): the tables of one (sr, N, n_mels), computed in double with exact integer phase
 *   reduction and rounded once: window [N]; twiddle [N / 2][2] = cos(2 pi m / N), -sin(2 pi m / N); the mel bank fb [F][n_mels]
 *   (melscale_fbanks(F, 0, sr / 2, n_mels, sr, norm = "slaney", mel_scale = "htk") in float64) as bands: first[j], count[j] = the bins
 *   with a non-zero weight (contiguous), weights = their values filter after filter.  Returns the number of weights (sum of count), or a
 *   negative FD_* code.  Every pointer NULL: the count only.  n_mels = 0: no bank (first, count, weights are not touched).
 * fd_specdist_plan_create: n_scales in [1, 16]; window_lengths[i] a power of two in [128, 4096]; n_mels[i] = 0: no mel term at scale i,
 *   else 1 <= n_mels[i] <= N / 2 and no filter may be empty; stft_term[i] != 0: the STFT terms at scale i.  Uploads the tables
 *   synchronously; nothing on the call path allocates.  The reference's two metrics in one plan: N = 128 .. 4096, n_mels = 10 .. 320,
 *   stft_term = 0 0 1 1 1 1.
 * fd_metrics_specdist_workspace_bytes(plan, B, L): 0 for a bad plan, B or L (1 <= B <= 65535, L > max(N) / 2).
 * fd_metrics_specdist: out DEVICE double [B][2] = msstft (sum over the scales of stft log mean + stft mag mean), mel (sum of the mel log
 *   means); terms DEVICE double [B][n_scales][3] = stft log, stft mag, mel log means (0 for a term the scale does not have), may be
 *   NULL.  A DEVICE length outside (max(N) / 2, L] gives NaN in everything of that clip and no out-of-bounds access.
 * fd_metrics_specdist_spectra (operator level, for tests): mag_hat, mag_x DEVICE float [B][T][F] with T = 1 + L / hop: A and R of scale
 *   `scale` exactly as the call above forms them; mel_hat, mel_x DEVICE float [B][T][n_mels]: M_hat and M (may be NULL; must be NULL at a
 *   scale without a mel term).  Zero in the frames t >= T_b.
 * The calls are asynchronous on `stream`, allocate nothing and launch nothing when they refuse: a NULL pointer, a bad B or L,
 * L <= max(N) / 2 and a workspace that is too small are FD_EINVAL with a message.
 * ---------------------------------------------------------------------------------------------- */
typedef struct fd_specdist_plan fd_specdist_plan;
int fd_specdist_tables(int sr, int N, int n_mels, float* window, float* twiddle, int* first, int* count, float* weights);
int fd_specdist_plan_create(int sr, int n_scales, const int* window_lengths, const int* n_mels, const int* stft_term, fd_specdist_plan** out);
void fd_specdist_plan_destroy(fd_specdist_plan* plan);
size_t fd_metrics_specdist_workspace_bytes(const fd_specdist_plan* plan, int B, int L);
int fd_metrics_specdist(const fd_specdist_plan* plan, const float* x_hat, const float* x, const int* lengths, int B, int L, double* out,
                        double* terms, void* ws, size_t ws_bytes, void* stream);
int fd_metrics_specdist_spectra(const fd_specdist_plan* plan, int scale, const float* x_hat, const float* x, const int* lengths, int B, int L,
                                float* mag_hat, float* mag_x, float* mel_hat, float* mel_x, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Segmental SNRs: the segmental SNR (`SSNR`) and the frequency-weighted segmental SNR (`fwSSNR`) of an estimate x_hat against a reference
 * x -- Hu & Loizou's comp_snr.m / comp_fwseg.m as the pysepm package restates them, which the reference's default metric list calls with
 * frameLen 0.03 and overlap 0.75 -- over ragged batches (csrc/segsnr.hip; host yardstick and the definitions in full:
 * flowdec_amd/segsnr.py).  Rows [B][L] float32 on the device; lengths: DEVICE int32 [B]; samples behind a clip's end are never read.  A
 * clip's results have the SAME BITS alone, in a batch, at any batch position and next to clips of any other lengths: every partition and
 * order of summation depends on the clip's own length only; no atomics.  Parity with the pysepm package is UNPINNED (the package is not
 * available to the tests; scripts/pin_segsnr.py prints the comparison where it is).
 *
 * With win = round(0.03 sr), skip = floor(0.0075 sr), n_fft = 2^ceil(log2(2 win)), w[n] = 0.5 (1 - cos(2 pi (n + 1) / (win + 1))) and
 * eps = 2^-52, both metrics use the frames t = 0 .. T_b - 1, T_b = (lengths[b] - win) / skip, frame t = samples [t skip, t skip + win):
 *     SSNR_t    clip(10 log10(sum (w x)^2 / (sum (w x - w x_hat)^2 + eps) + eps), -10, 35), float64 throughout
 *     fwSSNR_t  |DFT_n_fft(w (x + eps))| over the bins 0 .. n_fft / 2 - 1, divided by its sum over those bins, likewise for x_hat; the 25
 *               critical bands (Gaussian filters, centres 50 Hz .. 3597.63 Hz) ce = bank . clean, pe = bank . processed;
 *               clip(sum ce^0.2 10 log10(ce^2 / max((ce - pe)^2, eps)) / sum ce^0.2, -10, 35).  The transform is a float32 FFT in LDS of
 *               both signals at once (fft_lds.h), each frame of each signal scaled beforehand by the power of two that brings its peak
 *               into [1, 2) (the division by the sum cancels it); magnitudes, sums, bands and the logarithms in float64.
 * out[b] = the means over the clip's frames.  x_hat == x scores exactly 35 in both wherever no frame of x is silent.
 *
 * fd_segsnr_tables (HOST memory, no GPU needed): the tables of one rate in double: dims [3] = win, skip, n_fft (may be NULL); window
 *   [win]; twiddle [n_fft / 2][2] float32 (fd_specdist_tables'); the bank as bands: first[25], count[25] = the bins with a non-zero weight
 *   (contiguous), weights = their values filter after filter.  Returns the number of weights, or a negative FD_* code.  window .. weights
 *   all NULL: the count (and dims) only.  FD_EINVAL for a rate whose n_fft falls outside [128, 4096] or at which a band has no bin.
 * fd_segsnr_plan_create: uploads the tables of one rate synchronously; nothing on the call path allocates.
 * fd_metrics_segsnr_workspace_bytes(plan, B, L): 0 for a bad plan, B or L (1 <= B <= 65535, L >= 1).
 * fd_metrics_segsnr: out DEVICE double [B][2] = fwSSNR, SSNR (the reference's order); frames DEVICE double [B][T][2] with
 *   T = (L - win) / skip (0 below win + skip), may be NULL: the per-frame values, NaN in the frames t >= T_b.  A DEVICE length outside
 *   [win + skip, L] gives NaN in everything of that clip and no out-of-bounds access.
 * The calls are asynchronous on `stream`, allocate nothing and launch nothing when they refuse: a NULL pointer, a bad B or L and a
 * workspace that is too small are FD_EINVAL with a message, the outputs untouched.
 * ---------------------------------------------------------------------------------------------- */
typedef struct fd_segsnr_plan fd_segsnr_plan;
int fd_segsnr_tables(int sr, int* dims, double* window, float* twiddle, int* first, int* count, double* weights);
int fd_segsnr_plan_create(int sr, fd_segsnr_plan** out);
void fd_segsnr_plan_destroy(fd_segsnr_plan* plan);
size_t fd_metrics_segsnr_workspace_bytes(const fd_segsnr_plan* plan, int B, int L);
int fd_metrics_segsnr(const fd_segsnr_plan* plan, const float* x_hat, const float* x, const int* lengths, int B, int L, double* out,
                      double* frames, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FLOWDEC_HIP_H */
