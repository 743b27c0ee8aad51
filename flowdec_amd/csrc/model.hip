// model.hip -- the network itself: NCSN++ structure (ncsnpp.py:102-251), parameter store + MFMA weight packing (fd_model_create ...
// fd_model_finalize), the kernel choice per convolution (pick_conv), and the forward pass (ncsnpp.py:254-399) walked by Fwd over the
// workspace planner of arena.h; fd_ncsnpp_forward, fd_resblock and the profiling readers.  The solvers are in solve.hip, the waveform
// entry points and the validation loss in enhance.hip; model_internal.h is what the three share.
#include <string>
#include <vector>

#include "arena.h"
#include "model_internal.h"

using namespace fdm;

namespace {

struct Tens {
  size_t off = (size_t)-1;
  int C = 0, H = 0, W = 0;
  size_t sums = (size_t)-1;  // offset of the per-tile partial (sum, sumsq) floats [B][tiles][stride][2], if computed
  int tiles = 0, stride = 0;
};

int gn_groups(int C) { return (C / 4 < 32) ? C / 4 : 32; }

// mirrors NCSNpp.__init__ (ncsnpp.py:102-251) for progressive='output_skip', progressive_input='input_skip',
// combine 'sum', biggan blocks, no attention at the resolution levels, optionally one AttnBlockpp at the bottleneck (:196-199)
void build_structure(fd_model* m) {
  const fd_model_config& c = m->cfg;
  const int nf = c.nf, R = c.num_levels, nrb = c.num_res_blocks, nch = 4;
  auto& mods = m->mods;
  auto& P = m->params;
  mods.clear(); P.clear();
  auto add_param = [&](const std::string& n, std::vector<int> s) { P.push_back(ParamInfo{n, s}); };
  auto pref = [](int i) { return "backbone.all_modules." + std::to_string(i) + "."; };
  const int ks = m->arch.output_ksize;
  add_param("backbone.output_layer.weight", {2, nch, ks, ks});
  int idx = 0;
  auto push = [&](Mod md) { md.idx = idx++; mods.push_back(md); return (int)mods.size() - 1; };
  auto add_rb = [&](int c0, int c1, int cout, bool up, bool down, int level) {
    Mod md{}; md.kind = M_RB; md.c0 = c0; md.c1 = c1; md.cin = c0 + c1; md.cout = cout; md.up = up; md.down = down; md.level = level;
    md.has_c2 = (md.cin != cout) || up || down;
    const int i = mods[push(md)].idx;
    add_param(pref(i) + "GroupNorm_0.weight", {md.cin}); add_param(pref(i) + "GroupNorm_0.bias", {md.cin});
    add_param(pref(i) + "Conv_0.weight", {cout, md.cin, 3, 3}); add_param(pref(i) + "Conv_0.bias", {cout});
    add_param(pref(i) + "Dense_0.weight", {cout, 4 * nf}); add_param(pref(i) + "Dense_0.bias", {cout});
    add_param(pref(i) + "GroupNorm_1.weight", {cout}); add_param(pref(i) + "GroupNorm_1.bias", {cout});
    add_param(pref(i) + "Conv_1.weight", {cout, cout, 3, 3}); add_param(pref(i) + "Conv_1.bias", {cout});
    if (md.has_c2) { add_param(pref(i) + "Conv_2.weight", {cout, md.cin, 1, 1}); add_param(pref(i) + "Conv_2.bias", {cout}); }
  };
  { Mod md{}; md.kind = M_GFP; push(md); add_param(pref(0) + "W", {nf}); }
  { Mod md{}; md.kind = M_LINEAR; md.cin = 2 * nf; md.cout = 4 * nf; push(md); add_param(pref(1) + "weight", {4 * nf, 2 * nf}); add_param(pref(1) + "bias", {4 * nf}); }
  { Mod md{}; md.kind = M_LINEAR; md.cin = 4 * nf; md.cout = 4 * nf; push(md); add_param(pref(2) + "weight", {4 * nf, 4 * nf}); add_param(pref(2) + "bias", {4 * nf}); }
  { Mod md{}; md.kind = M_CONV_IN; md.cin = nch; md.cout = nf; push(md); add_param(pref(3) + "weight", {nf, nch, 3, 3}); add_param(pref(3) + "bias", {nf}); }
  std::vector<int> hs_c{nf};
  int in_ch = nf;
  for (int lvl = 0; lvl < R; ++lvl) {
    for (int b = 0; b < nrb; ++b) {
      const int out_ch = nf * c.ch_mult[lvl];
      add_rb(in_ch, 0, out_ch, false, false, lvl);
      in_ch = out_ch;
      hs_c.push_back(in_ch);
    }
    if (lvl != R - 1) {
      add_rb(in_ch, 0, in_ch, false, true, lvl + 1);
      Mod md{}; md.kind = M_COMBINE; md.cin = nch; md.cout = in_ch;
      const int i = mods[push(md)].idx;
      add_param(pref(i) + "Conv_0.weight", {in_ch, nch, 1, 1}); add_param(pref(i) + "Conv_0.bias", {in_ch});
      hs_c.push_back(in_ch);
    }
  }
  in_ch = hs_c.back();
  add_rb(in_ch, 0, in_ch, false, false, R - 1);
  if (m->arch.bottleneck_attn) {   // layerspp.py:72-89: GroupNorm_0, then NIN_0..3 (W [in][out], b)
    Mod md{}; md.kind = M_ATTN; md.cin = md.cout = in_ch; md.level = R - 1;
    const int i = mods[push(md)].idx;
    add_param(pref(i) + "GroupNorm_0.weight", {in_ch}); add_param(pref(i) + "GroupNorm_0.bias", {in_ch});
    for (int k = 0; k < 4; ++k) {
      add_param(pref(i) + "NIN_" + std::to_string(k) + ".W", {in_ch, in_ch});
      add_param(pref(i) + "NIN_" + std::to_string(k) + ".b", {in_ch});
    }
  }
  add_rb(in_ch, 0, in_ch, false, false, R - 1);
  for (int lvl = R - 1; lvl >= 0; --lvl) {
    for (int b = 0; b < nrb + 1; ++b) {
      const int out_ch = nf * c.ch_mult[lvl];
      const int sk = hs_c.back(); hs_c.pop_back();
      add_rb(in_ch, sk, out_ch, false, false, lvl);
      in_ch = out_ch;
    }
    { Mod md{}; md.kind = M_GN; md.cin = in_ch; const int i = mods[push(md)].idx;
      add_param(pref(i) + "weight", {in_ch}); add_param(pref(i) + "bias", {in_ch}); }
    { Mod md{}; md.kind = M_CONV_HEAD; md.cin = in_ch; md.cout = nch; const int i = mods[push(md)].idx;
      add_param(pref(i) + "weight", {nch, in_ch, 3, 3}); add_param(pref(i) + "bias", {nch}); }
    if (lvl != 0) add_rb(in_ch, 0, in_ch, true, false, lvl - 1);
  }
}

int upload_f32(fd_model* m, const std::string& name, float** out) {
  auto it = m->host.find(name);
  if (it == m->host.end()) return fd_set_error(FD_ESTATE, "parameter '%s' was never set", name.c_str());
  float* d = nullptr;
  FD_HIP(hipMalloc(&d, sizeof(float) * it->second.size()));
  FD_HIP(hipMemcpy(d, it->second.data(), sizeof(float) * it->second.size(), hipMemcpyHostToDevice));
  m->dev_allocs.push_back(d);
  m->dev_f32[name] = d;
  *out = d;
  return FD_OK;
}

// 3x3 convolution `name` (+ the 1x1 shortcut `sc_name` folded into its K loop, if named) packed for the kernel of `algo`
int pack_conv(fd_model* m, const std::string& name, int Cout, int C0, int C1, const std::string& sc_name, int S0, int S1, int algo,
              const void** out, hipStream_t st) {
  float *src = nullptr, *sc = nullptr;
  FD_TRY(upload_f32(m, name, &src));
  if (!sc_name.empty()) FD_TRY(upload_f32(m, sc_name, &sc));
  void* dst = nullptr;
  const int wdtype = m->dt | algo | m->opflag;   // mixed / split modes: bf16 weights for f32 activations
  const long long bytes = fd_conv_packed_bytes(Cout, C0, C1, 3, S0, S1, wdtype);
  FD_REQUIRE(bytes > 0, "internal: no packing for conv '%s'", name.c_str());
  FD_HIP(hipMalloc(&dst, (size_t)bytes));
  m->dev_allocs.push_back(dst);
  FD_TRY(fd_conv_pack_weights(src, sc, dst, Cout, C0, C1, 3, S0, S1, wdtype, st));
  *out = dst;
  return FD_OK;
}

// One ResBlock convolution packed for every kernel that the model's schedule may pick for it (pick_conv) and whose shape rules it
// meets.  FD_WINOGRAD / FD_WINOGRAD_LOWRES keep one packing: F(2,3) where it applies, else direct.
int pack_rb_conv(fd_model* m, int level, const std::string& name, int Cout, int C0, int C1, const std::string& sc_name, int S0, int S1,
                 ConvW* w, hipStream_t st) {
  auto fits = [&](int algo) { return fd_conv_packed_bytes(Cout, C0, C1, 3, S0, S1, m->dt | algo) > 0; };
  auto pack = [&](int algo, const void** out) { return pack_conv(m, name, Cout, C0, C1, sc_name, S0, S1, algo, out, st); };
  const bool f23_only = m->sched == CS_WINOGRAD || (m->sched == CS_WINOGRAD_LOWRES && level >= 2);
  if (f23_only && fits(FD_WINOGRAD)) return pack(FD_WINOGRAD, &w->f23);
  const bool by_size = m->sched == CS_AUTO || m->sched == CS_LATENCY;
  if (by_size && fits(FD_WINOGRAD)) FD_TRY(pack(FD_WINOGRAD, &w->f23));
  if (by_size && fits(FD_WINOGRAD4)) FD_TRY(pack(FD_WINOGRAD4, &w->f43));
  if (m->sched == CS_AUTO_F32 && fits(FD_WINOGRAD44)) FD_TRY(pack(FD_WINOGRAD44, &w->f44));
  return pack(0, &w->direct);
}

// ---------------------------------------------------------------------------------------------------------------
// forward pass
// ---------------------------------------------------------------------------------------------------------------
// The kernel one model convolution runs: packed weights and the fd_conv2d algorithm / workgroup flags.  First match wins.  Every rule
// looks at the IMAGE (px_tiles: 16 x 16-pixel tiles of one output image), never at the batch: a clip must give the same bits alone, in
// a batch, or in a shard of a batch (section 8(e)).
struct ConvPick { const void* w; int flags; };
ConvPick pick_conv(ConvSchedule s, const ConvW& w, int px_tiles, bool whole_tiles, int cin, int cout, bool shortcut) {
  const bool autosel = s == CS_AUTO, latency = s == CS_LATENCY;
  // fp32 `auto`: 2-D F(4x4, 3x3) in float32, a quarter of the direct kernel's MFMAs: 1.8-2.2 x the direct kernel per launch at 128 couts,
  // and at 256 couts 1.1-1.4 x the F(4,3) float32 kernel (profiles/r06_wino44f.txt); the matrix pipe bounds the launch at any grid size
  if (s == CS_AUTO_F32 && w.f44 && whole_tiles) return {w.f44, FD_WINOGRAD44};
  // `latency` (one short clip on the whole chip; profiles/r02_latency_tiles.txt): images of at most 24 tiles run the direct kernel with
  // 32-channel workgroups and chunk-resident weights (8 x the workgroups, one barrier per chunk)
  if (latency && px_tiles <= 24 && cout >= 64) return {w.direct, FD_TILE_BN32_CHUNK};
  // the 96 x 32 level: 18.5 us vs 22.6 (Winograd) at 8 clips, 17.1 vs 21.9 at one
  if (autosel && px_tiles <= 16 && cout >= 64) return {w.direct, FD_TILE_BN64_CHUNK};
  // F(2,3): its 128-cout workgroups are half the size of the direct kernel's, so a small grid fills the chip better with them (measured:
  // 1.12-1.14x at 48 tiles per image x 8 clips, 0.93-0.97x at 192+ per image); `latency` takes it up to 128 tiles.  Never with a folded
  // 1x1 shortcut: its input is the UN-NORMALISED residual stream, which the F(2,3) kernel would narrow to the fp16 range (GroupNorm+SiLU
  // outputs and their FIR-resampled versions are bounded)
  if ((autosel || latency) && w.f23 && !shortcut && px_tiles <= (latency ? 128 : 96)) return {w.f23, FD_WINOGRAD};
  // F(4,3) with 256-cout workgroups: half the MFMAs of the direct kernel, 1.09-1.19x per launch on images of more than 96 tiles
  // (profiles/r04_wino4_vs_direct.txt), 1.07x on the 64-channel input of the first block.  In `auto` it ALSO takes the folded-shortcut
  // Conv_1 launches of images of 17..96 tiles: 1.17-1.20x over the direct kernel at 192 x 64 x 8 clips (MEASUREMENTS R4.2, "L2" row);
  // the shortcut runs as a bf16 GEMM on the raw residual stream in its epilogue (no fp16 range issue).  `latency`, above 128 tiles: one
  // 1 s clip 60.0 -> 63.4x, one 2 s clip 79 -> 88.8x real time
  if ((autosel || (latency && px_tiles > 128)) && w.f43 && whole_tiles && cin >= 64) return {w.f43, FD_WINOGRAD4};
  // `latency`, folded-shortcut convolutions of the 384 x 64 level (96 tiles): 96 workgroups of 256 channels leave 160 CUs idle; 128-channel
  // workgroups are 1.28-1.39x per launch there (scripts/ab_conv_b1.py with AB_H=384 AB_W=64), same bits
  if (latency && px_tiles <= 128 && cout >= 256 && cout % 128 == 0) return {w.direct, FD_TILE_BN128};
  // `winograd` / `winograd_lowres` packed an F(2,3)-capable convolution for that kernel alone
  return w.direct ? ConvPick{w.direct, 0} : ConvPick{w.f23, FD_WINOGRAD};
}

struct Fwd {
  fd_model* m;
  bool dry;            // plan only (no launches, no pointers)
  char* base;
  Arena arena;
  hipStream_t st;
  int B, F, T, dt, esz;
  int w4_launches = 0;   // F(4,3) launches so far in this walk (alternating tile order)

  void* ptr(size_t off) const { return dry ? nullptr : base + off; }
  // ---- side branch: work that the main chain does not need right away runs on m->side between fork() and back(), and the main
  // stream waits for it at join().  Buffers a side branch frees go to `deferred` and are released at the join: until then the
  // arena may not hand them to a kernel of the main stream.  Off in profiling mode (per-kernel event timing) and for the planner.
  hipStream_t st_main = nullptr;
  std::vector<size_t> deferred;
  bool side_plan() const { return m && m->side; }                 // memory discipline: identical for the planner and every run
  bool side_ok() const { return !dry && side_plan() && !m->profiling; }   // the streams really fork
  int fork() {
    if (!side_ok()) return FD_OK;
    st_main = st;
    FD_HIP(hipEventRecord(m->ev_fork, st_main));
    FD_HIP(hipStreamWaitEvent(m->side, m->ev_fork, 0));
    st = m->side;
    return FD_OK;
  }
  void back() { if (side_ok()) st = st_main; }
  int join() {
    if (side_ok()) {
      FD_HIP(hipEventRecord(m->ev_join, m->side));
      FD_HIP(hipStreamWaitEvent(st, m->ev_join, 0));
    }
    for (size_t off : deferred) arena.release(off);
    deferred.clear();
    return FD_OK;
  }
  void release_later(size_t off, bool on_side) { if (on_side) deferred.push_back(off); else arena.release(off); }
  Tens talloc(int C, int H, int W) { Tens t; t.C = C; t.H = H; t.W = W; t.off = arena.alloc((size_t)B * H * W * C * esz); return t; }
  void tfree(Tens& t) {
    if (t.off != (size_t)-1) arena.release(t.off);
    if (t.sums != (size_t)-1) arena.release(t.sums);
    t.off = t.sums = (size_t)-1;
  }
  int ensure_sums(Tens& t) {
    if (t.sums != (size_t)-1) return FD_OK;
    t.tiles = fd_channel_sums_tiles(t.H, t.W);
    t.stride = t.C;
    t.sums = arena.alloc(sizeof(float) * 2 * (size_t)B * t.tiles * t.stride);
    if (dry) return FD_OK;
    return fd_channel_sums(ptr(t.off), (float*)ptr(t.sums), B, t.H, t.W, t.C, dt, st);
  }
  // GroupNorm over the virtual concat [a | b] -> affine pairs
  int gn_affine(Tens& a, Tens* b, const float* gamma, const float* beta, size_t* aff_off) {
    FD_TRY(ensure_sums(a));
    if (b) FD_TRY(ensure_sums(*b));
    const int C = a.C + (b ? b->C : 0);
    *aff_off = arena.alloc(sizeof(float) * 2 * (size_t)B * C);
    if (dry) return FD_OK;
    return fd_gn_finalize((const float*)ptr(a.sums), a.tiles, a.stride, a.C, b ? (const float*)ptr(b->sums) : nullptr, b ? b->tiles : 0,
                          b ? b->stride : 0, b ? b->C : 0, gamma, beta, (float*)ptr(*aff_off), B, gn_groups(C), (long long)a.H * a.W, 1e-6f, st);
  }
  // profiling: one launch between the next event pair of `pool` (grown on demand)
  template <typename Launch>
  int timed(std::vector<std::pair<hipEvent_t, hipEvent_t>>& pool, size_t& used, Launch&& launch) {
    if (used == pool.size()) {
      hipEvent_t e0, e1;
      FD_HIP(hipEventCreate(&e0)); FD_HIP(hipEventCreate(&e1));
      pool.emplace_back(e0, e1);
    }
    FD_HIP(hipEventRecord(pool[used].first, st));
    const int rc = launch();
    FD_HIP(hipEventRecord(pool[used].second, st));
    ++used;
    return rc;
  }
  // out = scale * (conv_3x3(act([a|b])) + conv_1x1([s0|s1]) + bias + skip); optionally emits the GroupNorm partials of out
  int conv(const Tens& a, const Tens* b, size_t aff, const Tens* s0, const Tens* s1, const ConvW& w, const float* bias, int bias_rows,
           const Tens* skip, float scale, Tens& out, bool want_stats) {
    constexpr int ks = 3;
    const int cin = a.C + (b ? b->C : 0);
    const ConvPick pick = pick_conv(m ? m->sched : CS_DIRECT, w, fd_cdiv(out.H, 16) * fd_cdiv(out.W, 16), out.H % 16 == 0 && out.W % 16 == 0,
                                    cin, out.C, s0 != nullptr);
    int flags = pick.flags;
    // every other F(4,3) launch of a forward walks its tiles backwards: a consumer then starts on the lines its producer wrote last,
    // which the memory-side cache still holds (the position in the launch sequence decides, so every forward has the same schedule)
    if (flags == FD_WINOGRAD4 && !dry && (w4_launches++ & 1) != 0) flags |= FD_TILE_REVERSED;   // (counted in launching walks only: a planning walk cannot shift the schedule)
    if (want_stats) {
      out.tiles = fd_conv_stats_tiles(out.H, out.W);
      out.stride = fd_conv_cout_pad(out.C);
      out.sums = arena.alloc(sizeof(float) * 2 * (size_t)B * out.tiles * out.stride);
    }
    if (dry) return FD_OK;
    const bool prof = m && m->profiling;
    auto launch = [&]() {
      return fd_conv2d(ptr(a.off), a.C, b ? ptr(b->off) : nullptr, b ? b->C : 0, aff == (size_t)-1 ? nullptr : (const float*)ptr(aff),
                       s0 ? ptr(s0->off) : nullptr, s0 ? s0->C : 0, s1 ? ptr(s1->off) : nullptr, s1 ? s1->C : 0, pick.w, bias, bias_rows,
                       skip ? ptr(skip->off) : nullptr, scale, ptr(out.off), out.C, want_stats ? (float*)ptr(out.sums) : nullptr, B,
                       out.H, out.W, ks, dt | flags | (m ? m->opflag : 0), st);
    };
    const int rc = prof ? timed(m->ev, m->ev_used, launch) : launch();
    if (prof) {
      const double csc = (s0 ? s0->C : 0) + (s1 ? s1->C : 0);
      m->prof_flops += 2.0 * B * out.H * out.W * (double)out.C * (cin * ks * ks + csc);
      // F(4,3): 6 products per 4 outputs and kernel row instead of 12 (the folded shortcut runs as a plain GEMM); F(2,3): 4 instead of 6
      // F(4x4, 3x3): 36 products per 16 outputs instead of 144
      const double exec = (flags & FD_WINOGRAD44) ? 0.25 : (flags & FD_WINOGRAD4) ? 0.5 : (flags & FD_WINOGRAD) ? 2.0 / 3.0 : 1.0;
      m->prof_flops_exec += 2.0 * B * out.H * out.W * (double)out.C * (cin * ks * ks * exec + csc);
      m->prof_bytes += (double)B * out.H * out.W * esz * (cin + csc + (skip ? out.C : 0) + out.C) + (double)esz * out.C * (cin * ks * ks + csc);
    }
    return rc;
  }

  // fd_fir_resample with per-launch timing when profiling (bytes: input read once, every output written once)
  int fir(const void* x, const float* aff, void* o_raw, void* o_act, int H, int W, int C, int dir) {
    const bool prof = m && m->profiling;
    auto launch = [&]() { return fd_fir_resample(x, aff, o_raw, o_act, B, H, W, C, dir, dt, st); };
    const int rc = prof ? timed(m->ev_fir, m->ev_fir_used, launch) : launch();
    if (prof) {
      const double in = (double)B * H * W * C * esz, out1 = dir > 0 ? 4.0 * in : 0.25 * in;
      m->prof_fir_bytes += in + out1 * ((o_raw ? 1 : 0) + (o_act ? 1 : 0));
    }
    return rc;
  }

  int resblock(const Mod& md, Tens& x0, Tens* x1, int nt, Tens& out, bool out_given = false) {
    const float rs2 = 0.70710678118654752440f;
    size_t aff0;
    FD_TRY(gn_affine(x0, x1, md.gn0_g, md.gn0_b, &aff0));
    const int H = x0.H, W = x0.W;
    const int OH = md.up ? 2 * H : (md.down ? H / 2 : H), OW = md.up ? 2 * W : (md.down ? W / 2 : W);
    Tens h1 = talloc(md.cout, OH, OW);
    Tens xr, hr;
    if (md.up || md.down) {
      xr = talloc(md.cin, OH, OW); hr = talloc(md.cin, OH, OW);
      if (!dry) FD_TRY(fir(ptr(x0.off), (const float*)ptr(aff0), ptr(xr.off), ptr(hr.off), H, W, md.cin, md.up ? 1 : -1));
      FD_TRY(conv(hr, nullptr, (size_t)-1, nullptr, nullptr, md.conv0, md.bias0_eff, nt, nullptr, 1.f, h1, true));
      tfree(hr);
    } else {
      FD_TRY(conv(x0, x1, aff0, nullptr, nullptr, md.conv0, md.bias0_eff, nt, nullptr, 1.f, h1, true));
    }
    arena.release(aff0);
    size_t aff1;
    FD_TRY(gn_affine(h1, nullptr, md.gn1_g, md.gn1_b, &aff1));
    if (!out_given) out = talloc(md.cout, OH, OW);
    else { out.C = md.cout; out.H = OH; out.W = OW; out.sums = (size_t)-1; }   // fd_resblock: the caller's output tensor
    if (md.has_c2) {  // Conv_1(act(GN1(h))) + Conv_2(x) in one launch (shortcut conv folded in as extra K steps)
      if (md.up || md.down) FD_TRY(conv(h1, nullptr, aff1, &xr, nullptr, md.conv1, md.b1, 1, nullptr, rs2, out, true));
      else FD_TRY(conv(h1, nullptr, aff1, &x0, x1, md.conv1, md.b1, 1, nullptr, rs2, out, true));
    } else {
      FD_TRY(conv(h1, nullptr, aff1, nullptr, nullptr, md.conv1, md.b1, 1, &x0, rs2, out, true));
    }
    if (md.up || md.down) tfree(xr);
    arena.release(aff1);
    tfree(h1);
    return FD_OK;
  }

  // AttnBlockpp at the bottleneck (ncsnpp.py:326-327): GroupNorm_0 from the partials x's producer emitted, q|k|v in f32 scratch, out with
  // the partials the next ResBlock's GroupNorm_0 consumes
  int attn(const Mod& md, Tens& x, Tens& out) {
    size_t aff;
    FD_TRY(gn_affine(x, nullptr, md.gn0_g, md.gn0_b, &aff));
    const int N = x.H * x.W;
    const size_t qkv = arena.alloc(fd_attn_qkv_bytes(B, N, x.C));
    out = talloc(x.C, x.H, x.W);
    out.tiles = fd_attn_stats_tiles(x.H, x.W); out.stride = x.C;
    out.sums = arena.alloc(sizeof(float) * 2 * (size_t)B * out.tiles * out.stride);
    if (!dry) {
      fd_attn_desc d{}; d.C = x.C; d.gn_gamma = md.gn0_g; d.gn_beta = md.gn0_b; d.w_qkv = md.w_qkv; d.b_qkv = md.b_qkv; d.w_out = md.w_f32; d.b_out = md.b_f32;
      FD_TRY(fd_attn_launch(ptr(x.off), (const float*)ptr(aff), d, (float*)ptr(qkv), ptr(out.off), (float*)ptr(out.sums), B, N, dt, st));
    }
    arena.release(qkv);
    arena.release(aff);
    return FD_OK;
  }

  // ncsnpp.py:254-399
  int run(const float* x, const float* y, const float* t, float t_imm, int nt, const OutSpec& os) {
    const fd_model_config& c = m->cfg;
    const int R = c.num_levels, nrb = c.num_res_blocks;
    const auto& mods = m->mods;
    const bool side = side_plan();
    if (!dry) {   // time embedding + the 22 Dense_0 biases: needed by the first ResBlock only -> beside the input packing / first conv
      if (side) FD_TRY(fork());
      FD_TRY(fd_time_embedding_impl(t, t_imm, nt, m->dev_f32["backbone.all_modules.0.W"], c.nf, m->dev_f32["backbone.all_modules.1.weight"],
                                    m->dev_f32["backbone.all_modules.1.bias"], m->dev_f32["backbone.all_modules.2.weight"],
                                    m->dev_f32["backbone.all_modules.2.bias"], m->temb, st));
      FD_TRY(fd_temb_bias_batched(m->jobs_dev, m->njobs, m->temb, nt, m->temb_dim, st));
      if (side) back();
    }
    size_t mi = 3;
    Tens in4 = talloc(8, F, T);   // 4 real channels + 4 zero channels (MFMA conv needs Cin % 8 == 0)
    if (!dry) { fd_edge_args a; a.x = x; a.y = y; a.out = ptr(in4.off); a.B = B; a.H = F; a.W = T; FD_TRY(fd_edge_pack_input(a, dt, st)); }
    std::vector<Tens> hs;
    {
      const Mod& md = mods[mi++];
      Tens h0 = talloc(md.cout, F, T);
      // all_modules.3 (3x3, 4 -> nf), emitting the GroupNorm partials of its output.  bf16 mode, whole tiles: a vector-FMA kernel next to
      // its stores (conv_in_kernel: the layer is all prologue and epilogue on the matrix cores, 237 -> 60 us at 8 x 768 x 256); otherwise
      // the MFMA kernel on the zero-padded 8-channel input
      const bool vec_in = dt == FD_BF16 && md.w_f32 && F % 16 == 0 && T % 16 == 0 && (md.cout == 8 || md.cout == 16 || md.cout == 32 || md.cout == 64 || md.cout == 128);
      if (vec_in) {
        h0.tiles = (F / 16) * (T / 16); h0.stride = md.cout;
        h0.sums = arena.alloc(sizeof(float) * 2 * (size_t)B * h0.tiles * h0.stride);
        if (!dry) { fd_edge_args a; a.x = ptr(in4.off); a.w = md.w_f32; a.bias = md.b_f32; a.out = ptr(h0.off); a.stats = (float*)ptr(h0.sums);
                    a.B = B; a.H = F; a.W = T; a.Cout = md.cout; FD_TRY(fd_edge_conv_in(a, dt, st)); }
      } else {
        FD_TRY(conv(in4, nullptr, (size_t)-1, nullptr, nullptr, md.conv0, md.b_f32, 1, nullptr, 1.f, h0, true));
        if (!dry && m->profiling) {   // the 4 padding channels are not algorithmic work
          m->prof_flops -= 2.0 * B * F * T * (double)md.cout * 4 * 9;
          m->prof_flops_exec -= 2.0 * B * F * T * (double)md.cout * 4 * 9;
        }
      }
      hs.push_back(h0);
    }
    if (side) FD_TRY(join());   // the time-embedding biases are ready
    Tens pyr_in = in4;  // input pyramid (owned here)
    Tens h;
    for (int lvl = 0; lvl < R; ++lvl) {
      for (int b = 0; b < nrb; ++b) {
        FD_TRY(resblock(mods[mi++], hs.back(), nullptr, nt, h));
        hs.push_back(h);
      }
      if (lvl != R - 1) {
        Tens hd;
        FD_TRY(resblock(mods[mi++], hs.back(), nullptr, nt, hd));
        Tens p2 = talloc(8, pyr_in.H / 2, pyr_in.W / 2);
        if (!dry) FD_TRY(fir(ptr(pyr_in.off), nullptr, ptr(p2.off), nullptr, pyr_in.H, pyr_in.W, 8, -1));
        tfree(pyr_in);
        pyr_in = p2;
        const Mod& md = mods[mi++];
        Tens hc = talloc(md.cout, hd.H, hd.W);
        hc.tiles = fd_combine_tiles(hd.H, hd.W); hc.stride = md.cout;     // the combine kernel emits the GroupNorm partials of hc
        hc.sums = arena.alloc(sizeof(float) * 2 * (size_t)B * hc.tiles * hc.stride);
        if (!dry) { fd_edge_args a; a.x = ptr(pyr_in.off); a.y = ptr(hd.off); a.w = md.w_f32; a.bias = md.b_f32; a.out = ptr(hc.off);
                    a.stats = (float*)ptr(hc.sums); a.B = B; a.H = hd.H; a.W = hd.W; a.Cout = md.cout; FD_TRY(fd_edge_combine(a, dt, st)); }
        tfree(hd);
        hs.push_back(hc);
      }
    }
    tfree(pyr_in);
    {
      Tens a1, a2;
      FD_TRY(resblock(mods[mi++], hs.back(), nullptr, nt, a1));
      if (mods[mi].kind == M_ATTN) {
        Tens at;
        FD_TRY(attn(mods[mi++], a1, at));
        tfree(a1);
        a1 = at;
      }
      FD_TRY(resblock(mods[mi++], a1, nullptr, nt, a2));
      tfree(a1);
      h = a2;
    }
    Tens pyramid; bool have_pyr = false;
    for (int lvl = R - 1; lvl >= 0; --lvl) {
      for (int b = 0; b < nrb + 1; ++b) {
        Tens sk = hs.back(); hs.pop_back();
        Tens o;
        FD_TRY(resblock(mods[mi++], h, &sk, nt, o));
        tfree(h); tfree(sk);
        h = o;
      }
      const Mod& gn = mods[mi++];
      const Mod& head = mods[mi++];
      // The head chain (GroupNorm + 3x3 conv to 4 channels + FIR-up of the running pyramid) only meets the main chain again at the
      // output layer: it runs on the side stream next to the up-sampling ResBlock that reads the same h.
      if (side) FD_TRY(fork());
      size_t aff;
      FD_TRY(gn_affine(h, nullptr, gn.gn0_g, gn.gn0_b, &aff));
      Tens pnew = talloc(4, h.H, h.W);
      if (have_pyr) {
        Tens pu = talloc(4, h.H, h.W);
        if (!dry) FD_TRY(fir(ptr(pyramid.off), nullptr, ptr(pu.off), nullptr, pyramid.H, pyramid.W, 4, +1));
        FD_TRY(conv(h, nullptr, aff, nullptr, nullptr, head.conv0, head.b_f32, 1, &pu, 1.f, pnew, false));
        release_later(pu.off, side); release_later(pyramid.off, side);
        pu.off = pyramid.off = (size_t)-1;
      } else {
        FD_TRY(conv(h, nullptr, aff, nullptr, nullptr, head.conv0, head.b_f32, 1, nullptr, 1.f, pnew, false));
      }
      release_later(aff, side);
      pyramid = pnew; have_pyr = true;
      if (side) back();
      if (lvl != 0) {
        Tens o;
        FD_TRY(resblock(mods[mi++], h, nullptr, nt, o));
        if (side) FD_TRY(join());   // the head has read h; its scratch goes back to the arena
        tfree(h);
        h = o;
      } else if (side) {
        FD_TRY(join());
      }
    }
    tfree(h);
    if (!hs.empty() || mi != mods.size()) return fd_set_error(FD_ESTATE, "internal: module walk mismatch");
    if (!dry) {
      fd_edge_args a; a.x = ptr(pyramid.off); a.w = m->wo; a.base = os.base; a.kold = os.kold; a.coef = os.coef; a.out = os.dst; a.ksave = os.ksave;
      a.B = B; a.H = F; a.W = T; a.ks = m->arch.output_ksize;
      if (os.score) { a.y = os.yv; a.z = os.z; a.cb = os.cb; a.cy = os.cy; a.cz = os.cz; a.ctab = os.ctab; }
      FD_TRY(os.score ? fd_edge_score_update(a, dt, st) : fd_edge_output_update(a, dt, st));
    }
    tfree(pyramid);
    return FD_OK;
  }
};

}  // namespace

namespace fdm {   // what solve.hip and enhance.hip call (model_internal.h)

int check_ready(const fd_model* m) {
  if (!m) return fd_set_error(FD_EINVAL, "null model");
  if (!m->finalized) return fd_set_error(FD_ESTATE, "model not finalised (call fd_model_finalize)");
  return FD_OK;
}

size_t forward_ws_bytes(const fd_model* m, int B, int T) {
  Fwd f{const_cast<fd_model*>(m), true, nullptr, Arena(), nullptr, B, m->n_freq, T, m->dt, (int)fd_dtype_size(m->dt)};
  OutSpec os;
  if (f.run(nullptr, nullptr, nullptr, 0.f, 1, os) != FD_OK) return 0;
  return f.arena.peak() + 256;
}

int check_shape(const fd_model* m, int B, int T) {
  const int div = 1 << (m->cfg.num_levels - 1);
  FD_REQUIRE(B > 0 && T > 0 && T % div == 0, "T_pad=%d must be a positive multiple of %d (B=%d)", T, div, B);
  FD_REQUIRE(m->n_freq % div == 0, "n_freq=%d not divisible by %d", m->n_freq, div);
  return FD_OK;
}

int forward_call(fd_model* m, const float* x, const float* y, const float* t, float t_imm, int nt, const OutSpec& os, int B, int T, void* ws,
                 size_t ws_bytes, hipStream_t st) {
  Fwd f{m, false, (char*)ws, Arena(), st, B, m->n_freq, T, m->dt, (int)fd_dtype_size(m->dt)};
  (void)ws_bytes;
  return f.run(x, y, t, t_imm, nt, os);
}

}  // namespace fdm

// ---------------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------------
extern "C" int fd_model_create_ex(const fd_model_config* cfg, const fd_model_arch* arch, fd_model** out) {
  FD_REQUIRE(cfg && arch && out, "fd_model_create: null pointer");
  FD_REQUIRE(cfg->nf >= 8 && cfg->nf % 8 == 0 && cfg->nf <= 128, "fd_model_create: nf must be a multiple of 8 in [8, 128] (got %d)", cfg->nf);
  FD_REQUIRE(arch->bottleneck_attn == 0 || arch->bottleneck_attn == 1, "fd_model_create_ex: bottleneck_attn must be 0 or 1");
  FD_REQUIRE(arch->output_ksize == 1 || arch->output_ksize == 3, "fd_model_create_ex: output_ksize must be 1 or 3 (got %d)", arch->output_ksize);
  FD_REQUIRE(cfg->num_levels >= 1 && cfg->num_levels <= 8 && cfg->num_res_blocks >= 1, "fd_model_create: bad level / block counts");
  const int act_nos = cfg->act_dtype & ~FD_NO_SIDE_STREAM;
  FD_REQUIRE(((act_nos & 0xff) == FD_BF16 && !(act_nos & (FD_BF16_OPERANDS | FD_BF16X3_OPERANDS))) || act_nos == FD_F32 || act_nos == (FD_F32 | FD_WINOGRAD_AUTO) ||
                 act_nos == (FD_F32 | FD_BF16_OPERANDS) || act_nos == (FD_F32 | FD_BF16X3_OPERANDS),
             "fd_model_create: act_dtype must be FD_BF16 [| FD_WINOGRAD | FD_WINOGRAD_LOWRES | FD_WINOGRAD_AUTO | FD_LOW_LATENCY], FD_F32 [| FD_WINOGRAD_AUTO], "
             "FD_F32 | FD_BF16_OPERANDS or FD_F32 | FD_BF16X3_OPERANDS");
  {
    const int algo = cfg->act_dtype & (FD_WINOGRAD | FD_WINOGRAD_LOWRES | FD_WINOGRAD_AUTO | FD_LOW_LATENCY);
    FD_REQUIRE((algo & (algo - 1)) == 0, "fd_model_create: at most one of FD_WINOGRAD / FD_WINOGRAD_LOWRES / FD_WINOGRAD_AUTO / FD_LOW_LATENCY (got 0x%x)", algo);
    FD_REQUIRE(algo == 0 || (cfg->act_dtype & 0xff) == FD_BF16 || (algo == FD_WINOGRAD_AUTO && act_nos == (FD_F32 | FD_WINOGRAD_AUTO)),
               "fd_model_create: the convolution-algorithm flags go with FD_BF16 storage (FD_WINOGRAD_AUTO also with pure FD_F32: 2-D F(4x4, 3x3) in float32)");
    FD_REQUIRE((cfg->act_dtype & FD_TILE_MASK) == 0, "fd_model_create: FD_TILE_* selects the workgroup width of ONE fd_conv2d launch, not of a model");
    FD_REQUIRE((cfg->act_dtype & ~(0xff | FD_WINOGRAD | FD_WINOGRAD_LOWRES | FD_WINOGRAD_AUTO | FD_LOW_LATENCY | FD_BF16_OPERANDS | FD_BF16X3_OPERANDS |
                                  FD_NO_SIDE_STREAM)) == 0, "fd_model_create: unknown bits in act_dtype (0x%x)", cfg->act_dtype);
  }
  FD_REQUIRE(cfg->n_fft > 0 && cfg->n_fft % 2 == 0 && cfg->hop > 0, "fd_model_create: bad STFT geometry");
  for (int i = 0; i < cfg->num_levels; ++i) {
    const int ch = cfg->nf * cfg->ch_mult[i];
    FD_REQUIRE(ch >= 8 && ch <= 256 && (ch & (ch - 1)) == 0, "fd_model_create: level width nf*ch_mult=%d must be a power of two in [8, 256]", ch);
  }
  if (arch->bottleneck_attn) {
    const int C = cfg->nf * cfg->ch_mult[cfg->num_levels - 1];
    FD_REQUIRE(C >= 16, "fd_model_create_ex: the bottleneck attention block needs >= 16 channels (got %d)", C);
  }
  fd_model* m = new fd_model();
  m->cfg = *cfg;
  m->arch = *arch;
  m->dt = cfg->act_dtype & 0xff;
  m->opflag = cfg->act_dtype & (FD_BF16_OPERANDS | FD_BF16X3_OPERANDS);
  const int algo = cfg->act_dtype & (FD_WINOGRAD | FD_WINOGRAD_LOWRES | FD_WINOGRAD_AUTO | FD_LOW_LATENCY);   // (at most one, checked above)
  m->sched = algo == FD_WINOGRAD ? CS_WINOGRAD : algo == FD_WINOGRAD_LOWRES ? CS_WINOGRAD_LOWRES : algo == FD_LOW_LATENCY ? CS_LATENCY :
             algo != FD_WINOGRAD_AUTO ? CS_DIRECT : m->dt == FD_F32 ? CS_AUTO_F32 : CS_AUTO;
  m->n_freq = cfg->n_fft / 2 + 1;
  m->temb_dim = 4 * cfg->nf;
  build_structure(m);
  *out = m;
  return FD_OK;
}

extern "C" int fd_model_create(const fd_model_config* cfg, fd_model** out) {
  const fd_model_arch arch{0, 1};
  return fd_model_create_ex(cfg, &arch, out);
}

extern "C" void fd_model_destroy(fd_model* m) {
  if (!m) return;
  for (auto& g : m->graphs) (void)hipGraphExecDestroy(g.second);
  for (void* p : m->dev_allocs) (void)hipFree(p);
  for (auto& e : m->ev) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
  for (auto& e : m->ev_fir) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
  fd_stft_plan_destroy(m->stft);
  if (m->pin_clips) (void)hipHostFree(m->pin_clips);
  if (m->ev_fork) (void)hipEventDestroy(m->ev_fork);
  if (m->ev_join) (void)hipEventDestroy(m->ev_join);
  if (m->side) (void)hipStreamDestroy(m->side);
  delete m;
}

extern "C" int fd_model_num_params(const fd_model* m) { return m ? (int)m->params.size() : 0; }

extern "C" int fd_model_param_info(const fd_model* m, int i, const char** name, int* ndim, int shape[4]) {
  FD_REQUIRE(m && i >= 0 && i < (int)m->params.size(), "fd_model_param_info: index out of range");
  const ParamInfo& p = m->params[i];
  if (name) *name = p.name.c_str();
  if (ndim) *ndim = (int)p.shape.size();
  if (shape) for (size_t k = 0; k < 4; ++k) shape[k] = k < p.shape.size() ? p.shape[k] : 1;
  return FD_OK;
}

extern "C" int fd_model_set_param(fd_model* m, const char* name, const float* host_data, long long numel) {
  FD_REQUIRE(m && name && host_data, "fd_model_set_param: null pointer");
  if (m->finalized) return fd_set_error(FD_ESTATE, "fd_model_set_param: model already finalised");
  for (const ParamInfo& p : m->params)
    if (p.name == name) {
      FD_REQUIRE(p.numel() == numel, "fd_model_set_param: '%s' expects %lld elements, got %lld", name, p.numel(), numel);
      m->host[name].assign(host_data, host_data + numel);
      return FD_OK;
    }
  return fd_set_error(FD_EINVAL, "fd_model_set_param: unknown parameter '%s'", name);
}

extern "C" int fd_model_set_sigma_y(fd_model* m, const double* host_sigma, int n) {
  FD_REQUIRE(m && host_sigma, "fd_model_set_sigma_y: null pointer");
  FD_REQUIRE(n == 1 || n == m->n_freq, "fd_model_set_sigma_y: expected 1 or %d values, got %d", m->n_freq, n);
  m->sigma_host.assign(host_sigma, host_sigma + n);
  m->sigma_n = n;
  if (m->sigma_dev) {
    FD_HIP(hipDeviceSynchronize());   // (rare, init-time) captured solves bake sigma_n into their launches: drop them
    for (auto& g : m->graphs) (void)hipGraphExecDestroy(g.second);
    m->graphs.clear(); m->seen.clear();
    FD_HIP(hipMemcpy(m->sigma_dev, m->sigma_host.data(), sizeof(double) * n, hipMemcpyHostToDevice));
  }
  return FD_OK;
}

extern "C" int fd_model_set_normalize(fd_model* m, int normalize) {
  FD_REQUIRE(m, "fd_model_set_normalize: null model");
  m->normalize = normalize != 0;
  return FD_OK;
}

extern "C" int fd_model_finalize(fd_model* m, void* stream) {
  FD_REQUIRE(m, "fd_model_finalize: null model");
  if (m->finalized) return FD_OK;
  hipStream_t st = fd_stream(stream);
  for (const ParamInfo& p : m->params)
    if (!m->host.count(p.name)) return fd_set_error(FD_ESTATE, "fd_model_finalize: parameter '%s' missing", p.name.c_str());
  FD_TRY(fd_conv_init_attributes());
  auto pref = [](int i) { return "backbone.all_modules." + std::to_string(i) + "."; };
  float* tmp;
  for (int i = 0; i < 3; ++i) {
    if (i == 0) FD_TRY(upload_f32(m, pref(0) + "W", &tmp));
    else { FD_TRY(upload_f32(m, pref(i) + "weight", &tmp)); FD_TRY(upload_f32(m, pref(i) + "bias", &tmp)); }
  }
  FD_TRY(upload_f32(m, "backbone.output_layer.weight", &m->wo));
  std::vector<fd_temb_job> jobs;
  size_t bias_total = 0;
  for (Mod& md : m->mods) if (md.kind == M_RB) bias_total += (size_t)fd_model::MAX_NT * md.cout;
  float* bias_pool = nullptr;
  FD_HIP(hipMalloc(&bias_pool, sizeof(float) * (bias_total ? bias_total : 1)));
  m->dev_allocs.push_back(bias_pool);
  size_t bias_off = 0;
  for (Mod& md : m->mods) {
    const std::string p = pref(md.idx);
    switch (md.kind) {
      case M_CONV_IN: {
        // zero-pad the 4 input channels to 8 and pack for the MFMA conv
        const std::vector<float>& w4 = m->host[p + "weight"];
        std::vector<float>& w8 = m->host[p + "weight.pad8"];
        w8.assign((size_t)md.cout * 8 * 9, 0.f);
        for (int o = 0; o < md.cout; ++o)
          for (int c = 0; c < 4; ++c)
            for (int k = 0; k < 9; ++k) w8[((size_t)o * 8 + c) * 9 + k] = w4[((size_t)o * 4 + c) * 9 + k];
        FD_TRY(pack_conv(m, p + "weight.pad8", md.cout, 8, 0, "", 0, 0, 0, &md.conv0.direct, st));
        FD_TRY(upload_f32(m, p + "bias", &md.b_f32));
        FD_TRY(upload_f32(m, p + "weight", &md.w_f32));   // [Cout][4][3][3] for the vector-FMA kernel of the bf16 mode
        break;
      }
      case M_COMBINE: {
        const std::string q = md.kind == M_COMBINE ? p + "Conv_0." : p;
        FD_TRY(upload_f32(m, q + "weight", &md.w_f32));
        FD_TRY(upload_f32(m, q + "bias", &md.b_f32));
        break;
      }
      case M_ATTN: {
        FD_TRY(upload_f32(m, p + "GroupNorm_0.weight", &md.gn0_g)); FD_TRY(upload_f32(m, p + "GroupNorm_0.bias", &md.gn0_b));
        const int Cc = md.cout;
        std::vector<float>& wq = m->host[p + "qkv.W"];
        std::vector<float>& bq = m->host[p + "qkv.b"];
        wq.assign((size_t)Cc * 3 * Cc, 0.f); bq.assign((size_t)3 * Cc, 0.f);
        for (int k = 0; k < 3; ++k) {
          const std::vector<float>& w = m->host[p + "NIN_" + std::to_string(k) + ".W"];
          const std::vector<float>& bb = m->host[p + "NIN_" + std::to_string(k) + ".b"];
          for (int r = 0; r < Cc; ++r)
            for (int c = 0; c < Cc; ++c) wq[(size_t)r * 3 * Cc + k * Cc + c] = w[(size_t)r * Cc + c];
          for (int c = 0; c < Cc; ++c) bq[(size_t)k * Cc + c] = bb[c];
        }
        FD_TRY(upload_f32(m, p + "qkv.W", &md.w_qkv)); FD_TRY(upload_f32(m, p + "qkv.b", &md.b_qkv));
        FD_TRY(upload_f32(m, p + "NIN_3.W", &md.w_f32)); FD_TRY(upload_f32(m, p + "NIN_3.b", &md.b_f32));
        break;
      }
      case M_GN:
        FD_TRY(upload_f32(m, p + "weight", &md.gn0_g));
        FD_TRY(upload_f32(m, p + "bias", &md.gn0_b));
        break;
      case M_CONV_HEAD:
        FD_TRY(pack_conv(m, p + "weight", md.cout, md.cin, 0, "", 0, 0, 0, &md.conv0.direct, st));
        FD_TRY(upload_f32(m, p + "bias", &md.b_f32));
        break;
      case M_RB: {
        FD_TRY(upload_f32(m, p + "GroupNorm_0.weight", &md.gn0_g)); FD_TRY(upload_f32(m, p + "GroupNorm_0.bias", &md.gn0_b));
        FD_TRY(upload_f32(m, p + "GroupNorm_1.weight", &md.gn1_g)); FD_TRY(upload_f32(m, p + "GroupNorm_1.bias", &md.gn1_b));
        // up/down blocks resample the (single) input first, so Conv_0 / Conv_2 see one tensor of cin channels
        FD_TRY(pack_rb_conv(m, md.level, p + "Conv_0.weight", md.cout, md.c0, md.c1, "", 0, 0, &md.conv0, st));
        // Conv_1 with the 1x1 shortcut Conv_2 folded into its K loop; biases add
        FD_TRY(pack_rb_conv(m, md.level, p + "Conv_1.weight", md.cout, md.cout, 0, md.has_c2 ? p + "Conv_2.weight" : std::string(),
                            md.has_c2 ? md.c0 : 0, md.has_c2 ? md.c1 : 0, &md.conv1, st));
        if (md.has_c2) {
          std::vector<float>& b1 = m->host[p + "Conv_1.bias"];
          const std::vector<float>& b2 = m->host[p + "Conv_2.bias"];
          for (size_t i = 0; i < b1.size(); ++i) b1[i] += b2[i];
        }
        FD_TRY(upload_f32(m, p + "Conv_1.bias", &md.b1));
        fd_temb_job j{};
        FD_TRY(upload_f32(m, p + "Dense_0.weight", &tmp)); j.dense_w = tmp;
        FD_TRY(upload_f32(m, p + "Dense_0.bias", &tmp)); j.dense_b = tmp;
        FD_TRY(upload_f32(m, p + "Conv_0.bias", &tmp)); j.conv_b = tmp;
        md.bias0_eff = bias_pool + bias_off; bias_off += (size_t)fd_model::MAX_NT * md.cout;
        j.out = md.bias0_eff; j.Cout = md.cout;
        jobs.push_back(j);
        break;
      }
      default: break;
    }
  }
  m->njobs = (int)jobs.size();
  FD_HIP(hipMalloc(&m->jobs_dev, sizeof(fd_temb_job) * jobs.size()));
  m->dev_allocs.push_back(m->jobs_dev);
  FD_HIP(hipMemcpy(m->jobs_dev, jobs.data(), sizeof(fd_temb_job) * jobs.size(), hipMemcpyHostToDevice));
  FD_HIP(hipMalloc(&m->temb, sizeof(float) * fd_model::MAX_NT * m->temb_dim));
  m->dev_allocs.push_back(m->temb);
  if (m->sigma_host.empty()) { m->sigma_host.assign(1, 0.0); m->sigma_n = 1; }
  FD_HIP(hipMalloc(&m->sigma_dev, sizeof(double) * m->n_freq));
  m->dev_allocs.push_back(m->sigma_dev);
  FD_HIP(hipMemcpy(m->sigma_dev, m->sigma_host.data(), sizeof(double) * m->sigma_n, hipMemcpyHostToDevice));
  FD_TRY(fd_stft_plan_create(m->cfg.n_fft, m->cfg.hop, &m->stft));
  if (!(m->cfg.act_dtype & FD_NO_SIDE_STREAM)) {   // (a config bit, not process state: FD_NO_SIDE_STREAM keeps everything on the caller's stream)
    FD_HIP(hipStreamCreateWithFlags(&m->side, hipStreamNonBlocking));
    FD_HIP(hipEventCreateWithFlags(&m->ev_fork, hipEventDisableTiming));
    FD_HIP(hipEventCreateWithFlags(&m->ev_join, hipEventDisableTiming));
  }
  FD_HIP(hipStreamSynchronize(st));
  m->host.clear();
  m->finalized = true;
  return FD_OK;
}

extern "C" size_t fd_model_workspace_bytes(const fd_model* m, int B, int T_pad) {
  if (!m || check_shape(m, B, T_pad) != FD_OK) return 0;
  return ode_ws_bytes(m, B, T_pad);
}

extern "C" int fd_ncsnpp_forward(fd_model* m, const float* x, const float* y, const float* t, int nt, float* v, int B, int T_pad, void* ws,
                                 size_t ws_bytes, void* stream) {
  FD_MODEL_ENTER(m, "fd_ncsnpp_forward");
  FD_TRY(check_ready(m));
  FD_REQUIRE(x && y && t && v && ws, "fd_ncsnpp_forward: null pointer");
  FD_TRY(check_shape(m, B, T_pad));
  FD_REQUIRE(nt == 1 || nt == B, "fd_ncsnpp_forward: t must have 1 or B entries (got %d)", nt);
  FD_REQUIRE(nt <= fd_model::MAX_NT, "fd_ncsnpp_forward: per-sample t supports at most %d clips", fd_model::MAX_NT);
  const size_t need = forward_ws_bytes(m, B, T_pad);
  if (ws_bytes < need) return fd_set_error(FD_ENOMEM, "fd_ncsnpp_forward: workspace %zu < required %zu bytes", ws_bytes, need);
  OutSpec os; os.dst = v; os.coef = 1.f;
  return forward_call(m, x, y, t, 0.f, nt, os, B, T_pad, ws, ws_bytes, fd_stream(stream));
}

// ---- one ResnetBlockBigGANpp as a stand-alone call (layerspp.py:252-284; the fusion unit of SURVEY 8(a13)) -----------
namespace {
int resblock_run(const fd_resblock_desc& d, const void* x0, const void* x1, void* out, int B, int H, int W, int dtype, bool dry, void* ws,
                 hipStream_t st, size_t* peak) {
  Mod md; md.kind = M_RB; md.cin = d.cin0 + d.cin1; md.c0 = d.cin0; md.c1 = d.cin1; md.cout = d.cout;
  md.up = d.up != 0; md.down = d.down != 0; md.has_c2 = d.has_conv2 != 0;
  md.conv0 = ConvW{d.w0}; md.conv1 = ConvW{d.w1};
  md.gn0_g = const_cast<float*>(d.gn0_gamma); md.gn0_b = const_cast<float*>(d.gn0_beta);
  md.gn1_g = const_cast<float*>(d.gn1_gamma); md.gn1_b = const_cast<float*>(d.gn1_beta);
  md.bias0_eff = const_cast<float*>(d.bias0); md.b1 = const_cast<float*>(d.bias1);
  Fwd f{nullptr, dry, (char*)ws, Arena(), st, B, 0, 0, dtype, (int)fd_dtype_size(dtype)};
  // tensors that live outside the workspace are addressed relative to it (never released to the arena)
  auto external = [&](const void* p, int C, int h, int w) { Tens t; t.off = (size_t)((const char*)p - (const char*)ws); t.C = C; t.H = h; t.W = w; return t; };
  Tens a = external(dry ? ws : x0, d.cin0, H, W), b, o = external(dry ? ws : out, d.cout, 0, 0);
  if (d.cin1) b = external(dry ? ws : x1, d.cin1, H, W);
  const int rc = f.resblock(md, a, d.cin1 ? &b : nullptr, d.bias0_rows, o, true);
  if (peak) *peak = f.arena.peak() + 256;
  return rc;
}
int check_resblock(const fd_resblock_desc* d, int B, int H, int W, int dtype) {
  FD_REQUIRE(d, "fd_resblock: null descriptor");
  FD_REQUIRE(d->cin0 > 0 && d->cin0 % 8 == 0 && d->cin1 >= 0 && d->cin1 % 8 == 0 && d->cout > 0 && d->cout % 8 == 0, "fd_resblock: channel counts must be multiples of 8");
  FD_REQUIRE(!(d->up && d->down) && (!(d->up || d->down) || d->cin1 == 0), "fd_resblock: up / down blocks take a single input tensor");
  FD_REQUIRE(d->has_conv2 || d->cin0 + d->cin1 == d->cout, "fd_resblock: identity shortcut needs Cin == Cout");
  FD_REQUIRE(B > 0 && H > 0 && W > 0 && (!d->down || (H % 2 == 0 && W % 2 == 0)), "fd_resblock: bad shape");
  FD_REQUIRE(dtype == FD_BF16 || dtype == FD_F32, "fd_resblock: bad dtype");
  return FD_OK;
}
}  // namespace

extern "C" size_t fd_resblock_workspace_bytes(const fd_resblock_desc* d, int B, int H, int W, int dtype) {
  if (check_resblock(d, B, H, W, dtype) != FD_OK) return 0;
  size_t peak = 0;
  if (resblock_run(*d, nullptr, nullptr, nullptr, B, H, W, dtype, true, nullptr, nullptr, &peak) != FD_OK) return 0;
  return peak;
}

extern "C" int fd_resblock(const fd_resblock_desc* d, const void* x0, const void* x1, void* out, int B, int H, int W, int dtype, void* ws,
                           size_t ws_bytes, void* stream) {
  FD_TRY(check_resblock(d, B, H, W, dtype));
  FD_REQUIRE(x0 && out && ws && (d->cin1 == 0) == (x1 == nullptr), "fd_resblock: null pointer / x1 mismatch");
  FD_REQUIRE(d->w0 && d->w1 && d->gn0_gamma && d->gn0_beta && d->gn1_gamma && d->gn1_beta && d->bias0 && d->bias1, "fd_resblock: incomplete descriptor");
  FD_REQUIRE(d->bias0_rows == 1 || d->bias0_rows == B, "fd_resblock: bias0_rows must be 1 or B");
  const size_t need = fd_resblock_workspace_bytes(d, B, H, W, dtype);
  if (ws_bytes < need) return fd_set_error(FD_ENOMEM, "fd_resblock: workspace %zu < required %zu bytes", ws_bytes, need);
  return resblock_run(*d, x0, x1, out, B, H, W, dtype, false, ws, fd_stream(stream), nullptr);
}

extern "C" int fd_profile_enable(fd_model* m, int enable) {
  FD_REQUIRE(m, "fd_profile_enable: null model");
  m->profiling = enable != 0;
  m->ev_used = 0;
  m->prof_flops = 0.0;
  m->prof_flops_exec = 0.0;
  m->prof_bytes = 0.0;
  m->ev_fir_used = 0;
  m->prof_fir_bytes = 0.0;
  if (m->stft) FD_TRY(fd_stft_plan_profile(m->stft, enable));
  return FD_OK;
}

extern "C" int fd_profile_read_stft(fd_model* m, double* ms6, int* calls2) {
  FD_REQUIRE(m && m->stft, "fd_profile_read_stft: null model / model not finalised");
  return fd_stft_plan_profile_read(m->stft, ms6, calls2);
}

extern "C" int fd_profile_read_fir(fd_model* m, double* ms_total, long long* launches, double* bytes_total) {
  FD_REQUIRE(m, "fd_profile_read_fir: null model");
  double ms = 0.0;
  for (size_t i = 0; i < m->ev_fir_used; ++i) {
    FD_HIP(hipEventSynchronize(m->ev_fir[i].second));
    float e = 0.f;
    FD_HIP(hipEventElapsedTime(&e, m->ev_fir[i].first, m->ev_fir[i].second));
    ms += e;
  }
  if (ms_total) *ms_total = ms;
  if (launches) *launches = (long long)m->ev_fir_used;
  if (bytes_total) *bytes_total = m->prof_fir_bytes;
  m->ev_fir_used = 0;
  m->prof_fir_bytes = 0.0;
  return FD_OK;
}

extern "C" int fd_profile_read(fd_model* m, double* conv_ms_total, long long* conv_launches, double* conv_flops_total, double* conv_bytes_total) {
  FD_REQUIRE(m, "fd_profile_read: null model");
  double ms = 0.0;
  for (size_t i = 0; i < m->ev_used; ++i) {
    FD_HIP(hipEventSynchronize(m->ev[i].second));
    float e = 0.f;
    FD_HIP(hipEventElapsedTime(&e, m->ev[i].first, m->ev[i].second));
    ms += e;
  }
  if (conv_ms_total) *conv_ms_total = ms;
  if (conv_launches) *conv_launches = (long long)m->ev_used;
  if (conv_flops_total) *conv_flops_total = m->prof_flops;
  if (conv_bytes_total) *conv_bytes_total = m->prof_bytes;
  m->prof_bytes = 0.0;
  m->ev_used = 0;
  m->prof_flops = 0.0;
  return FD_OK;
}

extern "C" int fd_profile_read_executed(fd_model* m, double* conv_flops_executed) {
  FD_REQUIRE(m && conv_flops_executed, "fd_profile_read_executed: null argument");
  *conv_flops_executed = m->prof_flops_exec;
  m->prof_flops_exec = 0.0;
  return FD_OK;
}
