// conv_wino4.hip -- 3x3 convolution as Winograd F(4,3) along W (time frames) x direct along H on the gfx950 matrix cores.
//
// Same contract as conv_mfma.hip (ddpm_conv3x3, flowdec/backbones/ncsnpp_utils/layers.py:128-134, with the ResnetBlockBigGANpp
// surroundings of layerspp.py:252-284 fused in: GroupNorm+SiLU operand transform, time/conv bias, residual, 1/sqrt(2), statistics
// of the output for the next GroupNorm, virtual channel concat) -- with HALF the MFMAs of the direct kernel: for four outputs
// y0..y3 = pixels 4j..4j+3 of a row and the six inputs d0..d5 = pixels 4j-1..4j+4
//   V = B^T d,  U = G g (one kernel row g),  M_xi = U_xi V_xi (6 products instead of 12),  y = A^T M
//   B^T = [4 0 -5 0 1 0; 0 -4 -4 1 1 0; 0 4 -4 -1 1 0; 0 -2 -1 2 1 0; 0 2 -1 -2 1 0; 0 4 0 -5 0 1]
//   G   = [1/4 0 0; -1/6 -1/6 -1/6; -1/6 1/6 -1/6; 1/24 1/12 1/6; 1/24 -1/12 1/6; 0 0 1]
//   A^T = [1 1 1 1 1 0; 0 1 -1 2 -2 0; 0 1 1 4 4 0; 0 1 -1 8 -8 1]
// summed over the three kernel rows dy and all input channels in the accumulators of position xi = 0..5.
//
// Design (round 4; what the round-2 F(2,3) kernel conv_wino.hip got wrong: MEASUREMENTS.md, "conv_wino_kernel"):
//   * one workgroup = 16 x 16 output pixels (64 Winograd tiles of 1 x 4) x ALL 256 output channels: the input is activated once
//     per pixel tile, as in the direct kernel (the F(2,3) kernel's 128-channel workgroups activated everything twice);
//   * the input transform happens ONCE per workgroup and chunk, in ONE producer pass: raw bf16 halo --(direct-to-LDS DMA)--> RAW -->
//     registers: silu(a x + d) -> fp16 -> packed-fp16 B^T transform --> LDS (V planes, double-buffered).  A lane owns one channel
//     pair of one THIRD of one halo row: it reads six of the row's 18 halo columns from RAW (a layout in which the lanes of a row
//     never conflict: "halo loader and producer" below, wino4_layout.h), activates them with the (a, d) of its two channels (four
//     registers, read per chunk from the affine table the prologue stages in LDS) -- every column is activated once.  The outer
//     lanes of a group of three hold the six columns of tiles 0 and 3; the middle lane takes two activated words from each
//     neighbour by DPP and transforms tiles 1 and 2.  18 rows x 8 words x 3 thirds = 432 items = 54 lanes in each of the eight
//     waves: ONE balanced pass per chunk (the 4-tile mapping before it needed 576 items for 512 lanes: rows 16 and 17 were a second
//     pass on one wave, which every wave met at the chunk barrier -- MEASUREMENTS.md "One balanced producer pass").  No
//     activated-halo staging buffer: that cost one LDS store phase, one LDS read phase, an s_waitcnt lgkmcnt(0) and a barrier per
//     chunk inside every wave's MFMA stream (MEASUREMENTS.md "One-pass producer").  The K loop then reads plain fragments: no VALU
//     work per fragment (the F(2,3) kernel transformed at fragment-read time, in every wave, for every cout tile: 6.9 VALU per MFMA);
//   * 6 x 256 x 64 accumulators = 96 K registers = 192 per lane of the 8 waves: wave (cq, xt) owns positions xi = 0, 1, 2 (xt = 0) or 5, 3, 4
//     (xt = 1) for couts {ct * 128 + cq * 32 + 0..31, ct = 0, 1} and all 64 tiles: 3 x (2 x 2) MFMA tiles of 32 x 32
//     (v_mfma_f32_32x32x16_f16); fragments rotate through three 16-byte quads per operand, 4 MFMAs per 4 ds_read_b128;
//   * K walks 16-channel chunks; per chunk a wave runs the 9 steps (xi, dy), 4 MFMAs each.  A step needs a 2-KiB weight piece that
//     only THIS wave reads: every wave streams its own pieces through a private ring of 6 LDS slots by direct-to-LDS DMA -- no
//     barrier for the weights at all, counted s_waitcnt vmcnt for this wave's own traffic (every vector-memory operation of the
//     loop is inline asm and counted by hand);
//   * one barrier per chunk (V planes complete + raw halo landed) and one more per chunk PAIR (the pair's RAW bytes consumed: the
//     next pair may be requested), both in the middle of a step with the fragments pipelined across; the producer pass runs in
//     different steps in the two wave groups;
//   * epilogue: partial output transforms in registers (xt = 0: M0+M1+M2, M1-M2, M1+M2; xt = 1: M3+M4, 2(M3-M4), 4(M3+M4),
//     8(M3-M4)+M5), the two waves of a cout block swap two planes each through LDS, then the direct kernel's staged sweep
//     (bias / residual (prefetched by DMA) / scale / statistics / bf16 store with 16 bytes per lane); with a folded 1x1 shortcut
//     (Conv_2 of layerspp.py:276-284) a bf16 MFMA GEMM on the raw shortcut input runs between the two on the same accumulators' outputs.
// Operands are fp16 (3 more mantissa bits than bf16 and packed add / fma for the transform); storage stays bf16, accumulation f32.
// Error of a 256-channel convolution against f64: 1.7e-3 (direct bf16 kernel: 1.9e-3; both are the bf16 output rounding).
// Measurements (per launch x1.14-1.22 over conv_mfma.hip at full resolution, counters, ablations): MEASUREMENTS.md section R4.
#include <type_traits>

#include "conv_common.h"
#include "wino4_layout.h"

namespace {

using namespace fdconv;

typedef _Float16 f16;
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int cmax(int a, int b) { return a > b ? a : b; }

// ---- geometry -------------------------------------------------------------------------------------------------------------
using fdw4::NTH, fdw4::HH, fdw4::HW, fdw4::RROW, fdw4::RROW_BYTES, fdw4::RAW_PASSES, fdw4::RAW_BYTES, fdw4::NPIECE, fdw4::VXI;   // (wino4_layout.h)
constexpr int TH = 16, TW = 16, BN = 256;
static_assert(HH == TH + 2 && HW == TW + 2, "wino4_layout.h describes this tile");
constexpr int CK = 16;                              // channels per K chunk (one 32-byte LDS row: two 16-byte halves)
constexpr int SLAB = BN * 32;                       // 8 KiB: the weights of one (chunk, xi, dy) step, [256 couts][16 ch] fp16
constexpr int RSLOT = 2048, NRING = 6;              // per-wave ring: 6 slots of 64 couts x 32 B (18 % NRING == 0)
static_assert(18 % NRING == 0, "the two-chunk loop body turns the ring a whole number of times");
constexpr int RING_BYTES = 8 * NRING * RSLOT;       // 96 KiB
constexpr int V_BYTES = 6 * VXI;                    // 13824
constexpr int V_OFF = RING_BYTES;
constexpr int AFF_OFF = V_OFF + 2 * V_BYTES;        // GroupNorm affine (a, d) of ALL input channels of this image, f32 pairs in concat order
                                                    // (fd_wino4_supported: at most AFF_BYTES), staged once by DMA in the prologue
constexpr int RAW_OFF = AFF_OFF + AFF_BYTES;        // raw halo (bf16) of a chunk PAIR as the DMA delivers it: one 64-byte slot per pixel,
                                                    // 20 slots per halo row (fdw4::raw_slot), the four 16-byte pieces [chunk parity][half]
                                                    // of a pixel inside its slot (fdw4::raw_flip): 1440 pieces = 3 passes of 512 lanes (24576 B)
constexpr int MAIN_BYTES = RAW_OFF + RAW_BYTES;     // 154624
// epilogue: exchange buffer [wave][plane][4][64 lanes x 16 B] = the staging of one round (128 pixels x 128 couts f32, padded rows)
// in the same bytes (a barrier apart), two residual buffers (one round each: 4 passes x 512 threads x 16 B), bias, statistics
constexpr int X_BYTES = 8 * 8192;                   // exchange buffer (two of them: one barrier per round)
constexpr int S_PITCH = 128 * 4 + 16;
constexpr int S_BYTES = 128 * S_PITCH;              // 67584; two staging buffers unless the residual buffers are in use
constexpr int SK_OFF = S_BYTES, SK_BYTES = 4 * NTH * 16;
constexpr int SCK = 2, SCD = 3;                     // shortcut GEMM: MFMA K steps (16 channels) per stage, stages resident (SCD - 1 in flight)
constexpr int WS_BYTES = SCK * SLAB;                // shortcut weights of a stage: [K step][cq][ct][32 couts][32 B], shared by the workgroup
constexpr int XS_OFF = SCD * WS_BYTES, XS_BYTES = SCK * 8192;   // SCD weight stages below, SCD x stages here
constexpr int BIAS_OFF = 2 * S_BYTES;               // = 135168: [256] f32; above what E1 (2 X) and E3 (2 S, or S + 2 SK) use.  E2 (shortcut:
                                                    // buffers up to XS_OFF + SCD * XS_BYTES) overlaps it: the table is written after E2
static_assert(BIAS_OFF >= 2 * X_BYTES && BIAS_OFF >= SK_OFF + 2 * SK_BYTES && XS_OFF + SCD * XS_BYTES <= 160 * 1024, "epilogue LDS map");
constexpr int ISC_OFF = BIAS_OFF + 1024;            // [256] f32: inverse of the per-cout power-of-two weight scale (wino4_scale_kernel)
constexpr int STAT_OFF = ISC_OFF + 1024;            // [2][8 waves][16 octets][16] f32 = 16 KiB
constexpr int LDS_BYTES = cmax(MAIN_BYTES, STAT_OFF + 16384);
static_assert(LDS_BYTES <= 160 * 1024 && NPIECE <= RAW_PASSES * NTH && AFF_BYTES <= 4 * 1024 && RAW_OFF % 128 == 0, "LDS layout");
constexpr int U_EXP = 9;                            // packed weights: every cout's row of U = G g is scaled by a power of two so that its
                                                    // largest magnitude lies in [2^(U_EXP-1), 2^U_EXP) -- fp16 keeps 23 binades below that
constexpr float RAW_MAX = 6000.f;                   // raw (not activated) inputs saturate here: |V| <= 10 |z| stays finite in fp16

__device__ __forceinline__ unsigned pack_f16(float a, float b) {
  f16x2 r = {(f16)a, (f16)b};
  return __builtin_bit_cast(unsigned, r);
}
__device__ __forceinline__ f16x2 h2(unsigned u) { return __builtin_bit_cast(f16x2, u); }
__device__ __forceinline__ unsigned u2(f16x2 v) { return __builtin_bit_cast(unsigned, v); }

// LDS-DMA from inline asm: not counted by hipcc, every wait for it is an explicit counted s_waitcnt vmcnt(N) below.  Each lane's 16 bytes
// come from (wave-uniform base + per-lane 32-bit byte offset) and land at LDS byte (M0 + instruction offset + lane * 16).  M0 is written
// in the same statement that uses it (cdna_hip_programming.md 5.7) and NOT restored: nothing else in this file uses M0 (gfx9+ LDS
// instructions do not).  M0 cannot go on the clobber list: hipcc treats it as a reserved register ("clobbering them may lead to undefined
// behaviour", -Winline-asm), so the BUILD checks the ISA instead -- flowdec_amd/build.py: no M0 use outside these statements, no scratch.
__device__ __forceinline__ void glds16s(const void* sbase, unsigned voff, unsigned lds_dst) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(sbase), "s"(lds_dst) : "memory");
}
// two consecutive 1-KiB pieces (global and LDS both + 1024 for the second)
__device__ __forceinline__ void glds16s_x2(const void* sbase, unsigned voff, unsigned lds_dst) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1\n\tglobal_load_lds_dwordx4 %0, %1 offset:1024" ::"v"(voff), "s"(sbase), "s"(lds_dst)
               : "memory");
}

template <bool ACT, bool SKIP, bool SC>
__global__ __launch_bounds__(NTH, 2) void conv_wino4_kernel(ConvArgs p) {
  static_assert(!(SKIP && SC), "residual input and folded shortcut exclude each other in this kernel");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  FD_T2(const unsigned long long t2_entry = __builtin_amdgcn_s_memtime();)

  // ---- tile decode with XCD-aware remap (as conv_mfma.hip) ------------------------------------------------------------
  const int bid = blockIdx.x, nblk = gridDim.x;
  int lid;
  {
    const int xcd = bid & 7, qq = nblk >> 3, rr = nblk & 7;
    lid = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + (bid >> 3);
  }
  if (p.reversed) lid = nblk - 1 - lid;   // FD_TILE_REVERSED: start where the producing launch stopped (its last lines are still cached)
  int pt = lid;
  const int tw_i = pt % p.tiles_w; pt /= p.tiles_w;
  const int th_i = pt % p.tiles_h;
  const int b = pt / p.tiles_h;
  const int h0 = th_i * TH, w0 = tw_i * TW;
  const int H = p.H, W = p.W;

  const int t = threadIdx.x;
  const int lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int cq = wave & 3, xt = wave >> 2;

  // ---- halo loader and producer.  The halo of a chunk PAIR (32 channels) is requested at once: 324 pixels x 64 contiguous bytes, FOUR
  // adjacent lanes per pixel (one memory request per pixel and pair: the 32-byte gathers of a per-chunk request were a third of the vector
  // L1's time), three passes of 512 lanes, straight to LDS by DMA (RAW; pass i of wave w at (i * 8 + w) KiB in lane order).  The DMA fixes
  // the LDS byte of every lane, the SOURCE address is free: LDS slot S = (t + 512 i) >> 2 holds the pixel (row S / 20, the column c with
  // raw_slot(c) = S % 20; slots 6 and 13 of a row and those behind row 17 are padding), lane position q = t & 3 of the slot the pixel's
  // piece q ^ (2 raw_flip(c)) -- fdw4::raw_request (wino4_layout.h).  PRODUCER, once per chunk, ONE pass RAW -> registers -> V that covers
  // all 18 halo rows: an item is (halo row, channel pair = 32-bit word 0..7 of a chunk's 32 bytes, column third k = 0..2), 432 items, 54 in
  // every wave (fdw4::item).  Lane k of a (row, word) group reads the halo columns 6 k .. 6 k + 5 straight from RAW (one base address, six
  // immediates), applies silu(a x + d) -> fp16 (or the saturation) and the zero padding to the six words: every one of the 18 columns is
  // activated ONCE.  The four tiles of the row need columns 0-5 (lane 0's own), 4-9, 8-13 and 12-17 (lane 2's own): lane 1 takes the
  // activated columns 4, 5 from lane 0 and 12, 13 from lane 2 (four v_mov_b32 with a DPP row shift: the three lanes are adjacent and never
  // straddle a 16-lane row) and transforms twice (tiles 1 and 2); the second transform's stores are masked off in lanes 0 and 2.  The
  // (a, d) of a lane's two channels come from the affine table that the prologue stages in LDS (AFF: one ds_read_b128 per chunk, 8
  // distinct 16-byte addresses per wave: a broadcast).
  // Bank conflicts (ds_read_b32 / ds_write_b32: banks = (byte / 4) % 32, a 32-lane group at a time).  The 8 words of a (slot, chunk parity)
  // are a quarter of the 128-byte bank row, quarter number 2 (slot & 1) + (parity ^ flip); the three lanes of a group need three
  // different quarters for each read j: slots j, 7 + j, 14 + j (parities j, ~j, j) with flips 0, 0, 1.  A V store of a group goes to
  // three of the four 32-byte tile cells of a 128-byte row.  So the lanes of ONE halo row never conflict; lanes 32..63 of a wave hold
  // one row, lanes 0..31 one row and two groups of rows 16 / 17, whose six lanes are 2-way conflicts (wino4_layout.h; checked
  // exhaustively on the host: tests/wino4_layout_check.cpp).
  // The K loop is bound by vector-instruction issue as soon as the per-chunk work costs more than a few hundred instructions per wave
  // (SQ counters, profiles/r04_wino4_*): everything a lane needs per chunk is computed ONCE here and kept in (packed) registers. -----
  auto opaque = [&](int v) { asm volatile("" : "+v"(v)); return v; };
  const size_t img_elems = (size_t)H * W;
  // The halo is addressed from its BAND: the first halo row of this tile (row hb of image b, a 64-bit wave-uniform base), so the
  // per-lane 32-bit byte offsets stay below (TH + 2) x W x C x 2 bytes whatever the image size (fd_conv2d checks the band bytes).
  const int hb = h0 > 0 ? h0 - 1 : 0;
  const size_t band_pix = (size_t)b * img_elems + (size_t)hb * W;
  // the (at most two) concat segments in scalar registers: no kernel-argument loads inside the K loop
  const bf16* const sb0 = reinterpret_cast<const bf16*>(p.seg[0].src) + band_pix * p.seg[0].C;
  const bool two3 = p.nseg > 1 && p.seg[1].taps == 9;   // (segments with taps == 1 are the folded shortcut: epilogue phase E2)
  const bf16* const sb1 = two3 ? reinterpret_cast<const bf16*>(p.seg[1].src) + band_pix * p.seg[1].C : sb0;
  const int sC0 = p.seg[0].C, sC1 = two3 ? p.seg[1].C : 0;
  const int nch0 = sC0 / CK, n3 = nch0 + sC1 / CK;
  // per-lane halo constants.  Ordering between the request side (lane t fills piece t + 512 i) and the producer side (which reads pieces
  // written by other waves' requests): "request after the barrier of step 3 of an even chunk (every producer pass over the previous pair
  // is done), landed before the barrier of step 8 (every wave waits for its own requests first), read after it".  Pixels outside the
  // image and padding slots: the request reads pixel 0 of the band (inside the image; harmless), the producer masks the value.
  int hpix[RAW_PASSES];                    // (pixel offset inside the band) * 4 + source piece
#pragma unroll
  for (int i = 0; i < RAW_PASSES; ++i) {   // request side: four adjacent lanes share a pixel's 64 bytes
    const fdw4::Req rq = fdw4::raw_request(t + i * NTH);
    const int gh = h0 - 1 + rq.row, gw = w0 - 1 + rq.col;
    const bool ok = rq.col >= 0 && gh >= 0 && gh < H && gw >= 0 && gw < W;
    hpix[i] = ((ok ? (gh - hb) * W + gw : 0) << 2) | (ok ? rq.piece : t & 3);
  }
  // producer side: item (halo row, word, third k).  pA = RAW byte of column 6 k (chunk parity 0; columns 6 k + j are 64 bytes apart) |
  // V offset of the first transform's tile << 16.  vbits: 1 = column 6 k is inside the image, 4 = column 6 k + 5 is, 2 = the row is,
  // 8 = the lane has an item, 16 = it is the middle lane of its group.  Idle lanes (10 of 64) repeat the reads of a neighbour and store nothing.
  int pA, vbits, pword;
  {
    const fdw4::Item it = fdw4::item(t);
    pA = fdw4::raw_addr(it.row, 6 * it.k, 0, it.word) | (fdw4::v_addr(it.row, fdw4::first_tile(it.k), it.word) << 16);
    const int gh = h0 - 1 + it.row;
    vbits = (it.k != 0 || w0 > 0 ? 1 : 0) | (gh >= 0 && gh < H ? 2 : 0) | (it.k != 2 || w0 + TW < W ? 4 : 0) | (it.active ? 8 : 0) |
            (it.active && it.k == 1 ? 16 : 0);
    pword = it.word;
  }
  // state of the chunk whose halo is in flight / being converted (wave-uniform)
  const bf16* nbase = sb0;
  int nC2 = 0, ncb = 0;              // bytes per pixel, byte offset of the chunk's 16 channels inside a pixel
  int cnext = 0;                     // index of the next chunk to request
  auto next_chunk = [&]() {          // (past the last chunk the state stays: load_halo turns the request into a harmless re-read)
    if (cnext < n3) {
      const bool first = cnext < nch0;
      const int cch = first ? cnext : cnext - nch0;
      nbase = first ? sb0 : sb1;
      nC2 = (first ? sC0 : sC1) * 2;
      ncb = cch * CK * 2;
    }
    ++cnext;
  };
  // past the end of the K loop every lane re-reads element 0 of the last tensor (one cache line; the data is never used)
  const unsigned rawdst = (unsigned)(RAW_OFF + wave * 1024);
  auto load_halo = [&]() {                // the 32 channels of the chunk pair that starts at the chunk next_chunk has just set up
    const int on = cnext <= n3 ? 1 : 0;   // (next_chunk has already counted this request)
#pragma unroll
    for (int i = 0; i < RAW_PASSES; ++i) {
      const int hp = opaque(hpix[i]);
      glds16s(nbase, (unsigned)(((hp >> 2) * nC2 + ncb + (hp & 3) * 16) * on), rawdst + i * 8192);
    }
  };
  // affine table of image b = [C0 + C1] (a, d) pairs in concat order (fd_conv2d: aff_off = 0 / C0): chunk cc, word wd at cc * 128 + wd * 16
  int affa = AFF_OFF + pword * 16;
  auto load_affine = [&]() {
    if constexpr (ACT) {
      if (wave < AFF_BYTES / 1024) {       // 1 KiB per wave; lanes behind the table re-read its start
        const int o = opaque(t) * 16;
        glds16s(p.affine + (size_t)b * p.affC * 2, (unsigned)(o < n3 * CK * 8 ? o : 0), (unsigned)(AFF_OFF + wave * 1024));
      }
    }
  };

  // ---- the producer pass of one item: RAW (bf16) -> [silu(a x + d)] -> fp16, zero padding AFTER the activation (an AND: no branch) ->
  // exchange inside the group -> packed-fp16 B^T (twice) -> V planes.  e = parity of the chunk inside its pair, affo = byte offset of
  // its affine records behind affa (both compile-time).  Every wave runs it once per chunk: halo rows 2 w, 2 w + 1 and two (row 16 / 17,
  // word) groups in wave w.
  auto produce = [&](const int e, const int vbuf, const int affo) {
    // (opaque: hipcc otherwise hoists the unpacked addresses out of the K loop -- registers it does not have)
    const int pa = opaque(pA), vbt = opaque(vbits);
    const char* const rp = smem + RAW_OFF + ((pa & 0xffff) ^ (e << 5));
    char* const vb = smem + V_OFF + vbuf * V_BYTES + (int)((unsigned)pa >> 16);
    unsigned w_[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) w_[j] = *reinterpret_cast<const unsigned*>(rp + j * 64);   // halo column 6 k + j
    f32x4 af = {0.f, 0.f, 0.f, 0.f};
    if constexpr (ACT) af = *reinterpret_cast<const f32x4*>(smem + opaque(affa) + affo);
    const unsigned mrow = (unsigned)((int)((unsigned)vbt << 30) >> 31);
    const unsigned m0 = mrow & (unsigned)((int)((unsigned)vbt << 31) >> 31), m5 = mrow & (unsigned)((int)((unsigned)vbt << 29) >> 31);
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      const unsigned u = w_[j];
      const float x0 = __builtin_bit_cast(float, u << 16), x1 = __builtin_bit_cast(float, u & 0xffff0000u);
      unsigned r;
      if constexpr (ACT) {   // silu >= -0.28: only the upper side can leave the range the transform tolerates (one packed min per pair)
        const f16x2 zc = {(f16)RAW_MAX, (f16)RAW_MAX};
        r = u2(__builtin_elementwise_min(h2(pack_f16(fd_silu(fmaf(x0, af[0], af[1])), fd_silu(fmaf(x1, af[2], af[3])))), zc));
      } else   // raw input (activated / resampled upstream): saturate so that the transform cannot overflow to inf
        r = pack_f16(__builtin_amdgcn_fmed3f(x0, -RAW_MAX, RAW_MAX), __builtin_amdgcn_fmed3f(x1, -RAW_MAX, RAW_MAX));
      w_[j] = r & (j == 0 ? m0 : j == 5 ? m5 : mrow);
    }
    // the middle lane's neighbours: columns 4, 5 (words 4, 5 of the lane below: row_shr:1) and 12, 13 (words 0, 1 of the lane above:
    // row_shl:1).  Lanes 0 and 2 of a group receive words they do not use (or nothing, at the ends of a 16-lane row).
    const unsigned l4 = (unsigned)__builtin_amdgcn_update_dpp(0, (int)w_[4], 0x111, 0xf, 0xf, true);
    const unsigned l5 = (unsigned)__builtin_amdgcn_update_dpp(0, (int)w_[5], 0x111, 0xf, 0xf, true);
    const unsigned r0 = (unsigned)__builtin_amdgcn_update_dpp(0, (int)w_[0], 0x101, 0xf, 0xf, true);
    const unsigned r1 = (unsigned)__builtin_amdgcn_update_dpp(0, (int)w_[1], 0x101, 0xf, 0xf, true);
    const bool mid = (vbt & 16) != 0;
    const f16x2 c4 = {(f16)4.f, (f16)4.f}, cm4 = {(f16)-4.f, (f16)-4.f}, cm5 = {(f16)-5.f, (f16)-5.f}, c2 = {(f16)2.f, (f16)2.f},
                cm2 = {(f16)-2.f, (f16)-2.f};
    auto transform = [&](char* const v, const unsigned d0, const unsigned d1, const unsigned d2, const unsigned d3, const unsigned d4, const unsigned d5) {
      const f16x2 z0 = h2(d0), z1 = h2(d1), z2 = h2(d2), z3 = h2(d3), z4 = h2(d4), z5 = h2(d5);
      const f16x2 t1 = __builtin_elementwise_fma(z2, cm4, z4);   // z4 - 4 z2
      const f16x2 t2 = __builtin_elementwise_fma(z1, cm4, z3);   // z3 - 4 z1
      const f16x2 t3 = z4 - z2, t4 = z3 - z1;
      // plane slots in the order xi = 0 1 2 | 5 3 4 (see the epilogue)
      *reinterpret_cast<unsigned*>(v + 0 * VXI) = u2(__builtin_elementwise_fma(z0, c4, __builtin_elementwise_fma(z2, cm5, z4)));   // xi = 0
      *reinterpret_cast<unsigned*>(v + 1 * VXI) = u2(t1 + t2);                                                                    // xi = 1
      *reinterpret_cast<unsigned*>(v + 2 * VXI) = u2(t1 - t2);                                                                    // xi = 2
      *reinterpret_cast<unsigned*>(v + 4 * VXI) = u2(__builtin_elementwise_fma(t4, c2, t3));                                       // xi = 3
      *reinterpret_cast<unsigned*>(v + 5 * VXI) = u2(__builtin_elementwise_fma(t4, cm2, t3));                                      // xi = 4
      *reinterpret_cast<unsigned*>(v + 3 * VXI) = u2(__builtin_elementwise_fma(z1, c4, __builtin_elementwise_fma(z3, cm5, z5)));   // xi = 5
    };
    // tiles 0 and 3 = the own six columns of lanes 0 and 2; tile 1 = columns 4 .. 9 = (l4, l5, own 0 .. 3) of lane 1
    if (vbt & 8)
      transform(vb, mid ? l4 : w_[0], mid ? l5 : w_[1], mid ? w_[0] : w_[2], mid ? w_[1] : w_[3], mid ? w_[2] : w_[4], mid ? w_[3] : w_[5]);
    // tile 2 = columns 8 .. 13 = (own 2 .. 5, r0, r1) of lane 1, the next 32 bytes of the V row
    if (mid) transform(vb + 32, w_[2], w_[3], w_[4], w_[5], r0, r1);
  };

  // ---- weight stream: this wave's 2 KiB (cout blocks ct = 0, 1: two consecutive 1-KiB pieces) of its step f -> ring slot f % NRING.
  // packed layout: [chunk][xt][xi][dy][cq][ct][32 couts][32 B]; the wave's 9 steps of a chunk are 9 consecutive slabs.  The stream
  // runs up to a ring length past the wave's last step: fd_wino4_packed_bytes pads the buffer by one chunk (what lands is never read).
  const char* wp = reinterpret_cast<const char*>(p.w) + (size_t)xt * 9 * SLAB + cq * 2048;   // first step of the current chunk pair
  asm volatile("" : "+s"(wp));
  const unsigned lane16 = (unsigned)(lane * 16);
  const unsigned wring = (unsigned)(wave * NRING * RSLOT);
  auto dma_step = [&](int f, int slot) {   // f = step index relative to the current chunk pair (compile-time)
    glds16s_x2(wp + (f / 9) * 18 * SLAB + (f % 9) * SLAB, lane16, wring + slot * RSLOT);
  };

  // ---- per-lane fragment coordinates --------------------------------------------------------------------------------------
  const int l31 = lane & 31, lh = lane >> 5;
  const int wa_lane = (int)wring + l31 * 32 + ((lh ^ ((l31 >> 3) & 1)) * 16);   // A: row l31 of the slot, cout block ct at + 1024
  // B: tile l31 (+ 32 at + 1024), halo row shift dy: row idx = l31 + 4 dy at idx * 32, half lh ^ ((idx >> 3) & 1).  dy = 2 flips the half
  // of every lane (idx + 8), dy = 1 that of the lanes with l31 & 4 (the carry into bit 3)
  const int vb0 = V_OFF + xt * 3 * VXI /* plane slots 0 1 2 | 5 3 4 */ + l31 * 32 + ((lh ^ ((l31 >> 3) & 1)) * 16);
  const int vb1 = (vb0 ^ ((l31 & 4) << 2)) + 128;

  f32x16 acc[3][2][2];
#pragma unroll
  for (int x = 0; x < 3; ++x)
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[x][ct][nt][e] = 0.f;

  auto lds_wait = [&]() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); };
  auto barrier = [&]() {
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };

  // Fragments: three quads per operand.  Step k multiplies A0 = qa[2k % 3], A1 = qa[(2k + 1) % 3] with B0 = qb[2k % 3], B1 = qb[(2k + 1) % 3]
  // in the order (A0,B0) (A0,B1) (A1,B0) (A1,B1); the spare quads (2k + 2) % 3 receive A0 / B0 of step k + 1 at the start of step k,
  // A1 of step k + 1 goes into A0's quad after the second MFMA, B1 of step k + 1 into B0's quad after the third (so the roles turn as
  // (A0, A1, spare) -> (spare, A0, A1)): every fragment is requested two to four MFMAs before its first use with 24 registers.
  u32x4 qa[3], qb[3];
  auto mma = [&](int xl, int ct, int nt, const u32x4& a, const u32x4& bq) {
    acc[xl][ct][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, bq), acc[xl][ct][nt], 0, 0, 0);
  };
  auto rd = [&](int off) { return *reinterpret_cast<const u32x4*>(smem + off); };
  // LDS offsets of the fragments of step k18 (0..17 inside the chunk pair; 18 = step 0 of the next pair)
  auto a_off = [&](int k18, int ct) { return wa_lane + (k18 % NRING) * RSLOT + ct * 1024; };
  auto b_off = [&](int k18, int nt) {
    const int s = k18 % 9, half = (k18 / 9) & 1;
    const int dy = s % 3;
    return (dy == 0 ? vb0 : dy == 1 ? vb1 : (vb0 ^ 16) + 256) + half * V_BYTES + (s / 3) * VXI + nt * 1024;
  };

  // ---- prologue: first halo, the first ring of weight steps and the affine table in one memory round trip; chunk 0 -> V[0] -------
  next_chunk();
  load_halo();
  load_affine();
#pragma unroll
  for (int k = 0; k < NRING; ++k) dma_step(k, k);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  barrier();                // every lane's halo slots and the affine table have landed
  produce(0, 0, 0);
  next_chunk();             // (chunk 1: its halo arrived with chunk 0's)
  lds_wait();
  barrier();                // V[0] complete
  FD_T2(const unsigned long long t2_first = __builtin_amdgcn_s_memtime();)
  qa[0] = rd(a_off(0, 0)); qb[0] = rd(b_off(0, 0)); qb[1] = rd(b_off(0, 1)); qa[1] = rd(a_off(0, 1));

  // ---- K loop.  Chunk c multiplies V[c & 1]; meanwhile the halo of chunk c + 1 (in RAW) is activated and transformed into V[(c + 1) & 1]
  // by the producer pass, and (in the even chunks) the halo of the pair c + 2, c + 3 is requested.  LDS ordering, one barrier per chunk:
  //   V[(c + 1) & 1]: last read by the fragments of chunk c - 1, which every wave has before it passes the barrier of step 8 of chunk
  //                   c - 1 (lds_wait in front of it); written in steps 0 and 1 of chunk c; complete (lds_wait) at the barrier of step 8
  //                   of chunk c; read from step 8 of chunk c on (the fragments of step 0 of chunk c + 1).
  //   RAW (one buffer for a chunk PAIR): parity 1 is read in steps 0 and 1 of the even chunk, parity 0 in steps 0 and 1 of the odd chunk
  //                   before it.  The barrier of step 3 of the EVEN chunks says "every producer pass over this pair is done": the request
  //                   for the next pair follows it, lands before the barrier of step 8 of the same chunk (every wave waits for its own
  //                   pieces first), and is read from step 0 of the odd chunk on.  The odd chunks have no barrier at step 3.
  //   AFF:            written once in the prologue, read only.
  // The two waves of a SIMD (groups xt = 0 / 1) do the producer's vector work in DIFFERENT steps:
  //   group 0: its four passes (halo rows 0..7 and half of rows 16, 17) in step 0
  //   group 1: its four passes (halo rows 8..15 and the other half of rows 16, 17) in step 1
  //   both:    the halo of the next chunk PAIR is requested in step 3 of the even chunks
  // A step starts with a counted wait for the weights of the NEXT step (its first fragments are requested right away); in flight on
  // this wave's vector-memory counter at that wait, oldest first: the weight pieces of steps s + 1 .. s + 5 (2 each) and, in the four
  // steps after a halo request, its three pieces: vmcnt(8 / 11).  The weights of step s + 6 are requested after the third MFMA of step
  // s: by then both weight fragments of step s have arrived and its ring slot is free.
  // Two chunks per iteration: 18 steps = three turns of the ring = six turns of the fragment quads, and the V buffers swap back, so
  // that every LDS offset is an immediate and the loop has ONE set of MFMA sites (two bodies in one loop double the accumulators).
  constexpr int NW = 2 * (NRING - 2);   // weight pieces that may stay in flight at the wait
  for (int c = 0; c < n3; c += 2) {
    int xg = xt;                       // (opaque per iteration: hipcc otherwise unswitches the loop on the wave group -- two loop bodies,
    asm volatile("" : "+s"(xg));       //  two sets of MFMA sites, spilled accumulators)
#pragma clang loop unroll(full)
    for (int k = 0; k < 18; ++k) {
      const int s = k % 9, half = k / 9;
      const int vn = half ^ 1;
      const int xl = s / 3;
      u32x4 &A0 = qa[(2 * k) % 3], &A1 = qa[(2 * k + 1) % 3], &A2 = qa[(2 * k + 2) % 3];
      u32x4 &B0 = qb[(2 * k) % 3], &B1 = qb[(2 * k + 1) % 3], &B2 = qb[(2 * k + 2) % 3];
      // the halo request of step 3 (issued BEFORE that step's weight request) is younger than the awaited weights in steps 4 .. 7 and
      // older than those of step 8: that wait also covers it, and the barrier behind it publishes the RAW slots
      if (s >= 4 && s <= 7 && half == 0) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NW + RAW_PASSES) : "memory");
      else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NW) : "memory");
      // s == 8: V[vn] complete (and the raw halo of the next pair landed), every wave has its last V[vc] fragments;
      // s == 3 of the even chunks: every producer pass has read the pair's RAW bytes (the request below overwrites them)
      if (s == 8 || (s == 3 && half == 0)) { lds_wait(); barrier(); }
      A2 = rd(a_off(k + 1, 0));
      B2 = rd(b_off(k + 1, 0));
      __builtin_amdgcn_sched_barrier(0);
      mma(xl, 0, 0, A0, B0);
      mma(xl, 0, 1, A0, B1);
      __builtin_amdgcn_sched_barrier(0);
      A0 = rd(a_off(k + 1, 1));
      mma(xl, 1, 0, A1, B0);
      __builtin_amdgcn_sched_barrier(0);
      B0 = rd(b_off(k + 1, 1));
      if (s == 3) { next_chunk(); if (half == 0) load_halo(); }   // (after the barrier of this step: every conversion of the previous pair is done)
      dma_step(k + NRING, k % NRING);              // step s + 6 into the slot whose fragments have both arrived
      mma(xl, 1, 1, A1, B1);
      __builtin_amdgcn_sched_barrier(0);
      // the chunk's vector work, while the quads A1 / B1 are dead: the NEXT chunk (the other parity) -> V[vn]
      if (s == 0) { if (xg == 0) produce(half ^ 1, vn, 128 * (1 + half)); }
      if (s == 1) { if (xg == 1) produce(half ^ 1, vn, 128 * (1 + half)); }
      __builtin_amdgcn_sched_barrier(0);
    }
    wp += 36 * SLAB;
    asm volatile("" : "+s"(wp));
    affa += 2 * CK * 8;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();  // all fragment reads / DMA done before the epilogue reuses the LDS
  FD_T2(const unsigned long long t2_loop = __builtin_amdgcn_s_memtime();)

  // ---- epilogue -------------------------------------------------------------------------------------------------------
  // Lane (l31, lh) of wave (cq, xt) holds, for cout block ct and tile block nt, acc[x][ct][nt][e]: cout ct * 128 + cq * 32 + 8 (e >> 2)
  // + 4 lh + (e & 3) of tile nt * 32 + l31 (row nt * 8 + (l31 >> 2), pixels 4 (l31 & 3) .. + 3); x = 0, 1, 2 are the positions
  // 0, 1, 2 (xt = 0) or 5, 3, 4 (xt = 1).
  //   E1  output transform.  Per (ct, nt): both wave groups run the same code with wave-uniform coefficients (a branch costs spilled
  //       accumulator tiles):  s = m1 + m2, d = m1 - m2;  send0 = s, send1 = ke d;  ya = ka m0 + ks s + recv0,  yb = kb m0 + kd d + recv1
  //         xt = 0 (m = M0, M1, M2): sends a2 = s, a1 = d;   y0 = M0 + s + b0,  y1 = d + b1             (ka ks kb kd ke = 1 1 0 1 1)
  //         xt = 1 (m = M5, M3, M4): sends b0 = s, b1 = 2 d;  y2 = 4 s + a2,     y3 = M5 + 8 d + a1      (ka ks kb kd ke = 0 4 1 8 2)
  //       the two waves of a cout block swap two planes through LDS (double-buffered: one barrier per round); afterwards wave (cq, xt)
  //       holds the pixel planes j = 2 xt (in m0) and 2 xt + 1 (in m1) of its couts and all 64 tiles.
  //   E2  (SC) the folded 1x1 shortcut conv Conv_2 (layerspp.py:278-279) as a bf16 GEMM straight into those planes: y[cout][pixel] +=
  //       W[cout][k] x[k][pixel], v_mfma_f32_32x32x16_bf16 on the RAW residual stream (no fp16 conversion: the direct kernel's numerics).
  //   E3  per (ct, nt): stage the round's 128 pixels x 128 couts as [pixel plane j][tile][cout] f32, sweep with 8 couts (16 B of bf16)
  //       per lane: bias / residual / scale / statistics / store.
  // output and residual from the tile's first row (row h0 of image b): the per-lane offsets of out_off stay 32-bit
  const size_t row0_pix = (size_t)b * img_elems + (size_t)h0 * W;
  bf16* const out = reinterpret_cast<bf16*>(p.out) + row0_pix * p.Cout;
  const bf16* const skip = SKIP ? reinterpret_cast<const bf16*>(p.skip) + row0_pix * p.Cout : nullptr;
  float* const biast = reinterpret_cast<float*>(smem + BIAS_OFF);      // [256] f32 (zeros without a bias)
  float* const statt = reinterpret_cast<float*>(smem + STAT_OFF);      // [ct][wave][oct 16][16] f32 partial sums
  float* const isct = reinterpret_cast<float*>(smem + ISC_OFF);        // [256] f32: 1 / (the cout's weight scale)
  auto load_bias_table = [&]() {
    if (t < BN) {
      // out = scale (acc / wscale + skip + bias) = acc (scale / wscale) + skip scale + bias scale: both tables carry `scale`, so that the
      // sweep is one fma per output pair (two with a residual) instead of fma + multiply (round 5: -0.4 % per launch)
      biast[t] = p.bias ? p.bias[(size_t)(p.bias_rows > 1 ? b : 0) * p.Cout + t] * p.scale : 0.f;
      isct[t] = p.w_scale[t] * p.scale;
    }
  };
  if constexpr (!SC) load_bias_table();   // (published by the barriers of the first round; with a shortcut: after E2, whose buffers overlap it)
  // element offset of pass ps of round (ct, nt) for this thread: staged pixel pp + 32 ps = plane ps of tile pp, cout octet oct
  auto out_off = [&](int tt, int ct, int nt, int ps) {
    const int oct = tt & 15, pp = tt >> 4;
    const int rh = nt * 8 + (pp >> 2), gw = w0 + 4 * (pp & 3) + ps;   // (row relative to h0)
    return (rh * W + gw) * p.Cout + ct * 128 + oct * 8;
  };
  // residual of round r -> SK[r & 1] by DMA: thread t requests exactly the 16 bytes it adds in the sweep (pass ps at (ps * 512 + t) * 16),
  // so the only synchronisation is this wave's own counted vmcnt
  auto skip_dma = [&](int r) {
    if constexpr (SKIP) {
      const int tt = opaque(t);
#pragma unroll
      for (int ps = 0; ps < 4; ++ps)
        glds16s(skip, (unsigned)(out_off(tt, r >> 1, r & 1, ps) * 2), (unsigned)(SK_OFF + (r & 1) * SK_BYTES + ps * NTH * 16 + wave * 1024));
    }
  };
  skip_dma(0);
  skip_dma(1);
  FD_T2(
  unsigned long long t2_r[5] = {0, 0, 0, 0, 0};
  t2_r[0] = __builtin_amdgcn_s_memtime();
  )

  const float ka = xt ? 0.f : 1.f, ks = xt ? 4.f : 1.f, kb = xt ? 1.f : 0.f, kd = xt ? 8.f : 1.f, kq = xt ? 0.25f : 1.f;
  // E1 of one round: partial transform, send, barrier, receive + combine (ya -> m0, yb -> m1); xoff = byte offset of the exchange buffer
  auto e1_round = [&](int rd_, int xoff) {
    const int ct = rd_ >> 1, nt = rd_ & 1;
    f32x16 &m0 = acc[0][ct][nt], &m1 = acc[1][ct][nt], &m2 = acc[2][ct][nt];
    const f32x2 kd2 = {kd, kd}, kq2 = {kq, kq}, ka2 = {ka, ka}, ks2 = {ks, ks}, kb2 = {kb, kb};
    char* const xmine = smem + xoff + wave * 8192 + lane * 16;
    const char* const xpeer = smem + xoff + (wave ^ 4) * 8192 + lane * 16;
    // (two channels per instruction: v_pk_add_f32 / v_pk_mul_f32 / v_pk_fma_f32 on consecutive accumulator registers)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      f32x2 snd[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int e = 4 * g + 2 * h;
        const f32x2 a1 = {m1[e], m1[e + 1]}, a2 = {m2[e], m2[e + 1]};
        const f32x2 s_ = a1 + a2, d_ = (a1 - a2) * kd2;
        m2[e] = s_[0]; m2[e + 1] = s_[1];
        m1[e] = d_[0]; m1[e + 1] = d_[1];
        snd[h] = d_ * kq2;                                     // ke d = (ke / kd) kd d
      }
      *reinterpret_cast<f32x4*>(xmine + g * 1024) = f32x4{m2[4 * g], m2[4 * g + 1], m2[4 * g + 2], m2[4 * g + 3]};
      *reinterpret_cast<f32x4*>(xmine + 4096 + g * 1024) = f32x4{snd[0][0], snd[0][1], snd[1][0], snd[1][1]};
    }
    lds_wait();
    barrier();
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 r0 = *reinterpret_cast<const f32x4*>(xpeer + g * 1024), r1 = *reinterpret_cast<const f32x4*>(xpeer + 4096 + g * 1024);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int e = 4 * g + 2 * h;
        const f32x2 mm = {m0[e], m0[e + 1]}, ss = {m2[e], m2[e + 1]}, dd = {m1[e], m1[e + 1]};
        const f32x2 q0 = {r0[2 * h], r0[2 * h + 1]}, q1 = {r1[2 * h], r1[2 * h + 1]};
        const f32x2 ya = __builtin_elementwise_fma(ka2, mm, __builtin_elementwise_fma(ks2, ss, q0));
        const f32x2 yb = __builtin_elementwise_fma(kb2, mm, dd + q1);
        m0[e] = ya[0]; m0[e + 1] = ya[1];
        m1[e] = yb[0]; m1[e + 1] = yb[1];
      }
    }
  };
  // E3 of one round: stage into sbuf (byte offset soff), barrier, sweep
  float ssum[8], ssq[8];
  auto e3_round = [&](int rd_, int soff) {
    const int ct = rd_ >> 1, nt = rd_ & 1;
    f32x16 &m0 = acc[0][ct][nt], &m1 = acc[1][ct][nt];
    char* const sbuf = smem + soff;
    if (nt == 0) {
#pragma unroll
      for (int j = 0; j < 8; ++j) ssum[j] = ssq[j] = 0.f;
    }
    {
      char* const sbase = sbuf + ((2 * xt) * 32 + l31) * S_PITCH + (cq * 32 + 4 * lh) * 4;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        *reinterpret_cast<f32x4*>(sbase + g * 32) = f32x4{m0[4 * g], m0[4 * g + 1], m0[4 * g + 2], m0[4 * g + 3]};
        *reinterpret_cast<f32x4*>(sbase + 32 * S_PITCH + g * 32) = f32x4{m1[4 * g], m1[4 * g + 1], m1[4 * g + 2], m1[4 * g + 3]};
      }
    }
    lds_wait();
    barrier();
    __builtin_amdgcn_sched_barrier(0);
    // sweep in two batches of two passes: computed into registers first, stores back to back afterwards.  The residual of this round
    // is in SK[rd_ & 1]; younger than its DMA are the stores of the previous round and the DMA issued after them.
    if constexpr (SKIP) {
      if (rd_ == 0 || rd_ == 3) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    }
    {
      const int tt = opaque(t);
      const int oct = tt & 15, pp = tt >> 4;
      const f32x4 bA = *reinterpret_cast<const f32x4*>(biast + ct * 128 + oct * 8), bB = *reinterpret_cast<const f32x4*>(biast + ct * 128 + oct * 8 + 4);
      const float bv[8] = {bA[0], bA[1], bA[2], bA[3], bB[0], bB[1], bB[2], bB[3]};
      // the accumulators hold (power-of-two scale of the cout) x (convolution + shortcut): the table entry is scale / (that power of two),
      // applied inside the fma that adds the (pre-scaled) bias / residual
      const f32x4 iA = *reinterpret_cast<const f32x4*>(isct + ct * 128 + oct * 8), iB = *reinterpret_cast<const f32x4*>(isct + ct * 128 + oct * 8 + 4);
      const float iv[8] = {iA[0], iA[1], iA[2], iA[3], iB[0], iB[1], iB[2], iB[3]};
#pragma unroll
      for (int bt = 0; bt < 2; ++bt) {
        u32x4 packed[2];
        int ooff[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const int ps = 2 * bt + q;
          ooff[q] = out_off(tt, ct, nt, ps);
          const float* sp = reinterpret_cast<const float*>(sbuf + (pp + ps * 32) * S_PITCH) + oct * 8;
          const f32x4 v0 = *reinterpret_cast<const f32x4*>(sp), v1 = *reinterpret_cast<const f32x4*>(sp + 4);
          float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
          if constexpr (SKIP) {
            const u32x4 skr = *reinterpret_cast<const u32x4*>(smem + SK_OFF + (rd_ & 1) * SK_BYTES + (ps * NTH + tt) * 16);
            const bf16x8 sk = __builtin_bit_cast(bf16x8, skr);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const f32x2 s2_ = {(float)sk[2 * k], (float)sk[2 * k + 1]}, sc2 = {p.scale, p.scale}, b2 = {bv[2 * k], bv[2 * k + 1]};
              const f32x2 i2 = {iv[2 * k], iv[2 * k + 1]}, x_ = {v[2 * k], v[2 * k + 1]};
              const f32x2 r_ = __builtin_elementwise_fma(x_, i2, __builtin_elementwise_fma(s2_, sc2, b2));
              v[2 * k] = r_[0]; v[2 * k + 1] = r_[1];
            }
          }
#pragma unroll
          for (int k = 0; k < 4; ++k) {
#pragma clang fp contract(off)
            f32x2 x = {v[2 * k], v[2 * k + 1]};
            f32x2 s1 = {ssum[2 * k], ssum[2 * k + 1]}, s2 = {ssq[2 * k], ssq[2 * k + 1]};
            if constexpr (!SKIP) {
              const f32x2 b2 = {bv[2 * k], bv[2 * k + 1]}, i2 = {iv[2 * k], iv[2 * k + 1]};
              x = __builtin_elementwise_fma(x, i2, b2);
            }
            s1 += x;
            s2 = __builtin_elementwise_fma(x, x, s2);
            v[2 * k] = x[0]; v[2 * k + 1] = x[1];
            ssum[2 * k] = s1[0]; ssum[2 * k + 1] = s1[1];
            ssq[2 * k] = s2[0]; ssq[2 * k + 1] = s2[1];
          }
          bf16x8 tv;
#pragma unroll
          for (int j = 0; j < 8; ++j) tv[j] = (bf16)v[j];
          packed[q] = __builtin_bit_cast(u32x4, tv);
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) *reinterpret_cast<u32x4*>(out + ooff[q]) = packed[q];
      }
    }
    if (nt == 1 && p.stats) {
      // channel sums of this cout half over the tile: fold the four 16-lane rows of the wave (they share the octets), then one
      // record per (wave, octet): 16 floats {sum, sumsq} x 8 channels
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        ssum[j] += __shfl_xor(ssum[j], 16, 64); ssq[j] += __shfl_xor(ssq[j], 16, 64);
        ssum[j] += __shfl_xor(ssum[j], 32, 64); ssq[j] += __shfl_xor(ssq[j], 32, 64);
      }
      if (lane < 16) {
        float* rec = statt + ((ct * 8 + wave) * 16 + lane) * 16;
#pragma unroll
        for (int j = 0; j < 4; ++j) *reinterpret_cast<f32x4*>(rec + 4 * j) = f32x4{ssum[2 * j], ssq[2 * j], ssum[2 * j + 1], ssq[2 * j + 1]};
      }
    }
  };

  if constexpr (SC) {
    // ---- E1 for all rounds (exchange buffers alternate: one barrier per round; the buffer of round r is written again in round r + 2,
    // and every wave has read it before it passes the barrier of round r + 1)
#pragma unroll
    for (int rd_ = 0; rd_ < 4; ++rd_) {
      e1_round(rd_, (rd_ & 1) * X_BYTES);
      __builtin_amdgcn_sched_barrier(0);
    }
    lds_wait();
    barrier();   // all exchange reads done: the LDS below is reused
    FD_T2(t2_r[1] = __builtin_amdgcn_s_memtime();)
    // ---- E2: folded shortcut ----
    {
      // K = the S0 + S1 channels of the (at most two) shortcut segments, in stages of SCK MFMA K steps (16 channels each).  A stage of x
      // is [pixel plane j][tile][64 B] (row r = j * 64 + tile = one pixel's 32 channels), filled by DMA -- the pixel order is made by
      // the SOURCE addresses.  Weights [K step][cq][ct][32 couts][32 B] bf16: the two waves of a cout block (xt = 0, 1) multiply the SAME
      // rows, so a stage's 16 KiB are loaded once -- wave (cq, xt) brings K step xt of its cout block (2 KiB), everybody reads both K
      // steps after the stage's barrier (private buffers fetched every piece twice).  SCD stages are resident: while stage s is multiplied, stages s + 1 and s + 2 are in flight (one
      // stage in flight left the phase at a quarter of the matrix rate: a stage is ~600 cycles of MFMAs, a DMA round trip ~2000).  One
      // barrier per stage, behind a counted wait: only the requests of the NEXT stage (4 instructions) may still be in flight.
      const int nsc = p.nseg - (sC1 ? 2 : 1);   // shortcut segments follow the 3x3 segments
      const Seg q0 = p.seg[p.nseg - nsc], q1 = p.seg[p.nseg - 1];
      const int S0 = q0.C, Stot = S0 + (nsc > 1 ? q1.C : 0);
      const int nstage = Stot / (16 * SCK);
      const bf16* const xb0 = reinterpret_cast<const bf16*>(q0.src) + row0_pix * q0.C;   // (from the tile's first row, as the output)
      const bf16* const xb1 = reinterpret_cast<const bf16*>(q1.src) + row0_pix * q1.C;
      const char* const wsc = reinterpret_cast<const char*>(p.w) + (size_t)(n3 + 1) * 18 * SLAB + cq * 2048;
      // per-lane source of the stage DMA.  A stage row is one pixel's 64 bytes (SCK = 2 K steps x 2 channel halves): FOUR adjacent
      // lanes fetch one pixel's contiguous 64 B (one memory request), lane l of DMA instruction i of wave w fills the 16 bytes at
      // ((i * 8 + w) * 64 + l) * 16: row r = that >> 2, 16-byte position q = l & 3, which holds piece (kk * 2 + half) = q ^ ((r >> 2) & 3)
      // (the XOR keeps the 64-byte-stride fragment reads free of bank conflicts)
      static_assert(SCK == 2, "a stage row = 2 K steps x 2 halves x 16 B; K step kk of the weights is loaded by wave group xt = kk");
      int xsrc[2];   // per DMA instruction: (pixel index from row h0) << 8 | byte offset of the piece inside the pixel's 64 B
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int r = ((i * 8 + wave) * 64 + lane) >> 2;
        const int xtile = r & 63, xj = r >> 6;
        const int piece = (lane & 3) ^ ((r >> 2) & 3);
        xsrc[i] = (((xtile >> 2) * W + w0 + 4 * (xtile & 3) + xj) << 8) | (piece * 16);
      }
      const unsigned lane16e = (unsigned)(lane * 16);
      // x of stage st -> x buffer `slot`, weights of stage st -> this wave's buffer `slot`; past the last stage: a harmless re-read of
      // stage 0 (every stage issues the same number of requests: the waits below count them)
      auto stage_dma = [&](int st, int slot) {
        const int ste = st < nstage ? st : 0;
        const int c0 = ste * 16 * SCK;
        const bool first = c0 < S0;
        const bf16* const xb = first ? xb0 : xb1;
        const int Cs = first ? S0 : Stot - S0, cc = first ? c0 : c0 - S0;
#pragma unroll
        for (int i = 0; i < 2; ++i)
          glds16s(xb, (unsigned)(((xsrc[i] >> 8) * Cs + cc) * 2 + (xsrc[i] & 255)), (unsigned)(XS_OFF + slot * XS_BYTES + i * 8192 + wave * 1024));
        glds16s_x2(wsc + (size_t)(ste * SCK + xt) * SLAB, lane16e, (unsigned)(slot * WS_BYTES + xt * SLAB + cq * 2048));
      };
      const int wa_sc = cq * 2048 + l31 * 32 + ((lh ^ ((l31 >> 3) & 1)) * 16);
      // B fragment of (K step kk, plane pl, tile block nt): row r = (2 xt + pl) * 64 + nt * 32 + l31 at r * 64, piece kk * 2 + lh at
      // position (kk * 2 + lh) ^ ((r >> 2) & 3) = ((kk * 2 + lh) ^ ((l31 >> 2) & 3))   (the row offsets are multiples of 16 rows)
      const int xb_row = XS_OFF + ((2 * xt) * 64 + l31) * 64;
      const int xb_sw = (l31 >> 2) & 3;
#pragma unroll
      for (int d = 0; d < SCD - 1; ++d) stage_dma(d, d);
      int slot = 0;
      for (int st = 0; st < nstage; ++st) {
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * (SCD - 2)) : "memory");   // stage st has landed (this wave's part)
        lds_wait();
        barrier();                                                                  // ... everybody's; buffer (slot + SCD - 1) % SCD is free
        const int nslot = slot == 0 ? SCD - 1 : slot - 1;                           // = (slot + SCD - 1) % SCD
        stage_dma(st + SCD - 1, nslot);
        const int wo = slot * WS_BYTES, xo = slot * XS_BYTES;
        // all twelve fragments of the stage first (the third accumulator plane is dead here: 48 registers are free), the MFMAs behind
        // them with the waits the compiler counts: one exposed LDS round trip per stage instead of four (hipcc otherwise issues every
        // group of reads right in front of its MFMAs)
        u32x4 af[SCK][2], bq[SCK][2][2];   // [K step][ct] and [K step][plane][nt]
#pragma unroll
        for (int kk = 0; kk < SCK; ++kk) {
          af[kk][0] = rd(wa_sc + wo + kk * SLAB);
          af[kk][1] = rd(wa_sc + wo + kk * SLAB + 1024);
#pragma unroll
          for (int pl = 0; pl < 2; ++pl)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) bq[kk][pl][nt] = rd(xb_row + xo + (pl * 64 + nt * 32) * 64 + (((kk * 2 + lh) ^ xb_sw) * 16));
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int kk = 0; kk < SCK; ++kk)
#pragma unroll
          for (int pl = 0; pl < 2; ++pl)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
              acc[pl][0][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, af[kk][0]), __builtin_bit_cast(bf16x8, bq[kk][pl][nt]), acc[pl][0][nt], 0, 0, 0);
              acc[pl][1][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, af[kk][1]), __builtin_bit_cast(bf16x8, bq[kk][pl][nt]), acc[pl][1][nt], 0, 0, 0);
            }
        __builtin_amdgcn_sched_barrier(0);
        slot = slot + 1 == SCD ? 0 : slot + 1;
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the re-reads past the last stage
      lds_wait();
      barrier();   // all fragment reads done: the staging buffers overlap the weight buffers and the x stages
      load_bias_table();
    }
    FD_T2(t2_r[2] = __builtin_amdgcn_s_memtime();)
    // ---- E3 for all rounds (two staging buffers: one barrier per round)
#pragma unroll
    for (int rd_ = 0; rd_ < 4; ++rd_) {
      e3_round(rd_, (rd_ & 1) * S_BYTES);
      __builtin_amdgcn_sched_barrier(0);
    }
  } else {
    // ---- rounds of E1 + E3.  Without a residual input the exchange buffer [0, 64 KiB) and the staging buffer behind it are separate:
    // two barriers per round (the next round's exchange stores follow this round's staging barrier, its staging stores the next
    // exchange barrier, which every wave reaches only after its sweep).  With one, the two residual buffers take that room: exchange
    // and staging share the bytes, four barriers per round.
#pragma unroll
    for (int rd_ = 0; rd_ < 4; ++rd_) {
      e1_round(rd_, 0);
      if constexpr (SKIP) { lds_wait(); barrier(); }
      e3_round(rd_, SKIP ? 0 : X_BYTES);
      if constexpr (SKIP) {
        lds_wait();
        barrier();
        if (rd_ < 2) skip_dma(rd_ + 2);   // SK[rd_ & 1] is free again
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  FD_T2(t2_r[3] = __builtin_amdgcn_s_memtime();)
  if (p.stats) {
    lds_wait();
    barrier();
    // o = 2 * channel + which = t;  channel = ct * 128 + oct * 8 + j
    const int ch = t >> 1, which = t & 1;
    const int ct = ch >> 7, oc = (ch >> 3) & 15, j = ch & 7;
    const float* src = statt + (ct * 8 * 16 + oc) * 16 + 2 * j + which;
    float a = 0.f;
#pragma unroll
    for (int w_ = 0; w_ < 8; ++w_) a += src[w_ * 256];
    const int tile = th_i * p.tiles_w + tw_i;
    p.stats[((size_t)b * p.tiles_h * p.tiles_w + tile) * p.CoutPad * 2 + t] = a;
  }
  FD_T2(
  if (p.dbg && t == 0 && bid < 8192) {
    const unsigned long long t2_end = __builtin_amdgcn_s_memtime();
    unsigned long long* d = p.dbg + (size_t)bid * 8;
    d[0] = t2_first - t2_entry; d[1] = t2_loop - t2_first; d[2] = t2_end - t2_loop;
    d[3] = t2_r[1] - t2_r[0]; d[4] = t2_r[2] - t2_r[1]; d[5] = t2_r[3] - t2_r[2]; d[6] = t2_end - t2_r[3]; d[7] = t2_r[0] - t2_loop;
  }
  )
}

// ---- weight packing: [Cout][Cin][3][3] f32 -> [chunk][xt][xi][dy][256 couts][32 B] fp16 ------------------------------------
// U_xi = G(xi) . w[dy][0..2]; a row's two 16-byte halves (channels 0-7 / 8-15 of the chunk) are XOR-swizzled by (cout >> 3) & 1.
__device__ __forceinline__ float wino4_u(const float* g, int xi) {
  const float g0 = g[0], g1 = g[1], g2 = g[2];
  switch (xi) {
    case 0: return 0.25f * g0;
    case 1: return -(g0 + g1 + g2) / 6.f;
    case 2: return (-g0 + g1 - g2) / 6.f;
    case 3: return g0 / 24.f + g1 / 12.f + g2 / 6.f;
    case 4: return g0 / 24.f - g1 / 12.f + g2 / 6.f;
    default: return g2;
  }
}

// Per-cout power-of-two scale.  G shrinks a kernel row by up to 24 x and fp16 goes subnormal below 6.1e-5: the rows of U of a cout whose
// weights are small (the reference zero-initialises Conv_1 and the pyramid heads, layers.py:100 -- a trained checkpoint may hold tiny
// weights exactly there) would lose their mantissa.  One block per cout: m = max |U| over (cin, dy, xi); scale = 2^k with m 2^k in
// [2^(U_EXP-1), 2^U_EXP); tab[cout] = 2^-k (the kernel's epilogue multiplies by it, exactly), tab[256 + cout] = 2^k (the pack kernels).
// The folded shortcut's weights get the same factor (exact in bf16): both land in the same f32 accumulators -- so the factor is also
// bounded by THEIR magnitude (a cout whose 3x3 row is ~1e-30 next to O(1) shortcut weights must not push the shortcut products
// towards the edge of f32: scaled shortcut weights stay below 2^SC_EXP_MAX; the 3x3 row then flushes to zero in fp16, which is
// what it is next to the shortcut term).
constexpr int SC_EXP_MAX = 60;
__global__ void wino4_scale_kernel(const float* __restrict__ w, const float* __restrict__ w_sc, float* __restrict__ tab, int Cout, int Cin, int S) {
  __shared__ float red[256], red_sc[256];
  const int co = blockIdx.x, t = threadIdx.x;
  float m = 0.f, msc = 0.f;
  if (co < Cout) {
    for (int i = t; i < Cin * 3; i += 256) {
      const float* g = w + ((size_t)co * Cin * 3 + i) * 3;
#pragma unroll
      for (int xi = 0; xi < 6; ++xi) m = fmaxf(m, fabsf(wino4_u(g, xi)));
    }
    if (w_sc)
      for (int i = t; i < S; i += 256) msc = fmaxf(msc, fabsf(w_sc[(size_t)co * S + i]));
  }
  red[t] = m;
  red_sc[t] = msc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) { red[t] = fmaxf(red[t], red[t + o]); red_sc[t] = fmaxf(red_sc[t], red_sc[t + o]); }
    __syncthreads();
  }
  if (t == 0) {
    int k = 0;
    m = red[0];
    msc = red_sc[0];
    if (m > 0.f && m < 3.0e38f) {
      int e;
      frexpf(m, &e);             // m = f 2^e, f in [0.5, 1)
      k = U_EXP - e;
      k = k < -100 ? -100 : (k > 100 ? 100 : k);
      if (msc > 0.f && msc < 3.0e38f) {
        int es;
        frexpf(msc, &es);
        if (k > SC_EXP_MAX - es) k = SC_EXP_MAX - es;
      }
    }
    tab[co] = ldexpf(1.f, -k);
    tab[BN + co] = ldexpf(1.f, k);
  }
}

__global__ void wino4_pack_kernel(const float* __restrict__ w, f16* __restrict__ dst, const float* __restrict__ tab, int Cout, int C0, int C1) {
  const int Cin = C0 + C1, nchunks = Cin / CK;
  const long long total = (long long)nchunks * 18 * BN * CK;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int k = (int)(i % CK);
    long long r = i / CK;
    const int n = (int)(r % BN); r /= BN;
    const int dy = (int)(r % 3); r /= 3;
    const int slot = (int)(r % 6);                          // wave group xt = slot / 3 owns the slabs slot % 3 = 0..2
    const int xi = slot < 3 ? slot : (slot == 3 ? 5 : slot - 1);   // positions in the order 0 1 2 | 5 3 4 (see the epilogue)
    const int chunk = (int)(r / 6);
    const int c = chunk * CK + k;   // (concat segments are multiples of 16 channels: a chunk never straddles them)
    const int co = ((n >> 5) & 1) * 128 + (n >> 6) * 32 + (n & 31);   // slab row n = [cq][ct][32] holds cout ct * 128 + cq * 32 + m
    float v = 0.f;
    if (co < Cout) v = wino4_u(w + (((size_t)co * Cin + c) * 3 + dy) * 3, xi) * tab[BN + co];
    const int half = (k >> 3) ^ ((n >> 3) & 1);
    dst[(i - k) + half * 8 + (k & 7)] = (f16)v;
  }
}

// shortcut weights [Cout][S] f32 -> [K step of 16 channels][slab row n = [cq][ct][32]][32 B] bf16, halves swizzled by (n >> 3) & 1
__global__ void wino4_pack_sc_kernel(const float* __restrict__ w, bf16* __restrict__ dst, const float* __restrict__ tab, int Cout, int S) {
  const long long total = (long long)(S / CK) * BN * CK;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int k = (int)(i % CK);
    long long r = i / CK;
    const int n = (int)(r % BN);
    const int ks = (int)(r / BN);
    const int co = ((n >> 5) & 1) * 128 + (n >> 6) * 32 + (n & 31);
    const float v = co < Cout ? w[(size_t)co * S + ks * CK + k] * tab[BN + co] : 0.f;   // (a power of two: the bf16 rounding is that of the plain weight)
    const int half = (k >> 3) ^ ((n >> 3) & 1);
    dst[(i - k) + half * 8 + (k & 7)] = (bf16)v;
  }
}

}  // namespace

bool fd_wino4_supported(int Cout, int C0, int C1, int S0, int S1, int ksize) {
  return ksize == 3 && Cout == BN && C0 > 0 && C0 % 32 == 0 && C1 % 32 == 0 && S0 % 32 == 0 && S1 % 32 == 0 && (S1 == 0 || S0 > 0) &&
         (C0 + C1) * 8 <= AFF_BYTES;
}
bool fd_wino4_shape_ok(int H, int W) { return H % TH == 0 && W % TW == 0; }

namespace {
// The packed buffer starts with a fixed 4-KiB header: the scale table [2][256] f32 (inverse scales, scales).  Its position does
// not depend on the segment list of a launch (it used to sit behind the shortcut steps: a weight packed with a folded shortcut but
// launched without its shortcut segments read another table); the packed steps the kernel streams follow at W4_HDR.
constexpr long long W4_HDR = 4096;
}  // namespace

long long fd_wino4_packed_bytes(int Cout, int C0, int C1, int S0, int S1) {
  (void)Cout;
  // header, 3x3 part + one chunk (the weight stream runs a ring length past the last step), then the shortcut K steps (+ slack)
  return W4_HDR + (long long)((C0 + C1) / CK + 1) * 18 * SLAB + (long long)((S0 + S1) / CK) * SLAB + 16 * 1024;
}

int fd_wino4_pack_weights(const float* w, const float* w_sc, void* packed, int Cout, int C0, int C1, int S0, int S1, hipStream_t st) {
  const long long total = (long long)((C0 + C1) / CK) * 18 * BN * CK;
  const int blocks = (int)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
  float* const tab = reinterpret_cast<float*>(packed);
  char* const steps = reinterpret_cast<char*>(packed) + W4_HDR;
  hipLaunchKernelGGL(wino4_scale_kernel, dim3(BN), dim3(256), 0, st, w, w_sc, tab, Cout, C0 + C1, w_sc ? S0 + S1 : 0);
  hipLaunchKernelGGL(wino4_pack_kernel, dim3(blocks), dim3(256), 0, st, w, (f16*)steps, tab, Cout, C0, C1);
  if (w_sc) {
    const long long tsc = (long long)((S0 + S1) / CK) * BN * CK;
    const int bsc = (int)((tsc + 255) / 256 > 4096 ? 4096 : (tsc + 255) / 256);
    hipLaunchKernelGGL(wino4_pack_sc_kernel, dim3(bsc), dim3(256), 0, st, w_sc,
                       reinterpret_cast<bf16*>(steps + (size_t)((C0 + C1) / CK + 1) * 18 * SLAB), tab, Cout, S0 + S1);
  }
  FD_LAUNCH_CHECK();
  return FD_OK;
}

namespace {
template <bool ACT>
int set_attr4() {
  FD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(conv_wino4_kernel<ACT, false, false>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES));
  FD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(conv_wino4_kernel<ACT, true, false>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES));
  FD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(conv_wino4_kernel<ACT, false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES));
  return FD_OK;
}
template <bool ACT>
void launch4(const ConvArgs& a, bool sc, dim3 grid, dim3 block, hipStream_t st) {
  if (sc) hipLaunchKernelGGL((conv_wino4_kernel<ACT, false, true>), grid, block, LDS_BYTES, st, a);
  else if (a.skip) hipLaunchKernelGGL((conv_wino4_kernel<ACT, true, false>), grid, block, LDS_BYTES, st, a);
  else hipLaunchKernelGGL((conv_wino4_kernel<ACT, false, false>), grid, block, LDS_BYTES, st, a);
}
}  // namespace

int fd_wino4_init_attributes() {
  FD_TRY(set_attr4<false>());
  FD_TRY(set_attr4<true>());
  return FD_OK;
}

int fd_wino4_launch(ConvArgs a, hipStream_t st) {
  FD_REQUIRE(fd_wino4_shape_ok(a.H, a.W), "fd_conv2d: FD_WINOGRAD4 needs H %% 16 == 0 and W %% 16 == 0 (got %d x %d)", a.H, a.W);
  bool sc = false;
  for (int s = 0; s < a.nseg; ++s) sc = sc || a.seg[s].taps == 1;
  a.w_scale = reinterpret_cast<const float*>(a.w);                   // header of the packed buffer (launch-independent position)
  a.w = reinterpret_cast<const char*>(a.w) + W4_HDR;                 // the packed steps
  FD_REQUIRE(!(sc && a.skip), "fd_conv2d: FD_WINOGRAD4 takes a folded shortcut or a residual input, not both");
  a.tiles_h = a.H / TH;
  a.tiles_w = a.W / TW;
  a.tiles_n = 1;
  a.CoutPad = BN;
  const long long nblk = (long long)a.B * a.tiles_h * a.tiles_w;
  FD_REQUIRE(nblk > 0 && nblk < (1ll << 31), "conv grid out of range");
  const dim3 grid((unsigned)nblk), block(NTH);
  if (a.affine) launch4<true>(a, sc, grid, block, st);
  else launch4<false>(a, sc, grid, block, st);
  FD_LAUNCH_CHECK();
  return FD_OK;
}
