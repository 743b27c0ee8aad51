// ndac_plan_check.cpp -- the codec's structure as flowdec_amd/csrc/ndac_plan.h states it, stand-alone and without a GPU.
//
//   ndac_plan_check ENCODER_DIM ENC_RATES LATENT_DIM DECODER_DIM DEC_RATES N_CODEBOOKS CODEBOOK_SIZE CODEBOOK_DIM [len L]... [frames T]... [slot L]...
//
// (rates as 2,4,5) prints one line per fact:
//   param NAME DIM...                                              the parameter table, in order
//   enc|dec KIND Ci Co K STRIDE PAD DIL WEIGHT BIAS ALPHA RES RAW TANH   one record per convolution, in execution order (KIND conv | convT; WEIGHT /
//                                                                  BIAS / ALPHA as parameter NAMES, ALPHA `-` for none; the flags as 0 | 1)
//   hop H / up U
//   len L FRAMES / frames T SAMPLES / slot L ELEMS                 encoder frames of L samples, decoded samples of T frames, elements per batch item
//                                                                  of one workspace slot
//   whole_frames ok|MESSAGE / even_rates ok|MESSAGE
//   encode_halo LEFT RIGHT / decode_halo LEFT RIGHT                (printed whatever the two preconditions say)
// and checks what holds for every configuration: the records chain (each Ci is the Co before it), the frame-table advance gives the
// clips' lengths that out_len gives, and a record's dependency interval covers exactly the inputs its kernel reads.  Exit status 1 and a
// line `FAIL ...` otherwise.  tests/test_model_host_cpu.py drives it.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ndac_plan.h"

static int parse_rates(const char* s, int out[8]) {
  int n = 0;
  for (const char* p = s; *p && n < 8;) {
    out[n++] = (int)strtol(p, const_cast<char**>(&p), 10);
    if (*p == ',') ++p;
  }
  return n;
}

static int fail(const char* what, long long a, long long b) { printf("FAIL %s: %lld vs %lld\n", what, a, b); return 1; }

// the inputs output n of a record reads, by the definition of the operation (every tap that lands on an integer input position)
static void taps_of(const ndac::Layer& l, long long n, long long& lo, long long& hi) {
  lo = 1ll << 40; hi = -(1ll << 40);
  for (int k = 0; k < l.K; ++k) {
    long long t;
    if (l.transposed) {
      if ((n + l.pad - k) % l.stride != 0) continue;
      t = (n + l.pad - k) / l.stride;
    } else {
      t = n * l.stride - l.pad + (long long)k * l.dil;
    }
    if (t < lo) lo = t;
    if (t > hi) hi = t;
  }
}

static int check_stack(const char* tag, const ndac::Plan& p, const std::vector<ndac::Layer>& s, int first_ci, int mul) {
  int ci = first_ci, add = 0;
  const long long frames = 5;
  long long T = frames * mul;
  for (const ndac::Layer& l : s) {
    if (l.Ci != ci) return fail("channels do not chain", l.Ci, ci);
    ci = l.Co;
    const bool whole = l.transposed || p.whole_frames_error.empty();
    T = l.out_len(T);
    l.advance(mul, add);
    if (whole && frames * mul + add != T) return fail("frame-table advance", frames * mul + add, T);
    for (long long n = 64 * l.stride; n < 64 * l.stride + 2 * l.stride + 2; ++n) {   // (positive positions: % and / as the kernels use them)
      long long lo = n, hi = n, tl, th;
      l.depends_on(lo, hi);
      taps_of(l, n, tl, th);
      if (lo != tl) return fail("dependency interval, low end", lo, tl);
      if (hi != th) return fail("dependency interval, high end", hi, th);
    }
    printf("%s %s %d %d %d %d %d %d %s %s %s %d %d %d\n", tag, l.transposed ? "convT" : "conv", l.Ci, l.Co, l.K, l.stride, l.pad, l.dil,
           p.params[l.weight].name.c_str(), p.params[l.bias].name.c_str(), l.alpha_out >= 0 ? p.params[l.alpha_out].name.c_str() : "-", (int)l.residual,
           (int)l.keep_raw, (int)l.tanh_out);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 9) return 2;
  fd_ndac_config c;
  memset(&c, 0, sizeof c);
  c.encoder_dim = atoi(argv[1]); c.n_encoder_rates = parse_rates(argv[2], c.encoder_rates); c.latent_dim = atoi(argv[3]);
  c.decoder_dim = atoi(argv[4]); c.n_decoder_rates = parse_rates(argv[5], c.decoder_rates);
  c.n_codebooks = atoi(argv[6]); c.codebook_size = atoi(argv[7]); c.codebook_dim = atoi(argv[8]);
  const ndac::Plan p = ndac::make_plan(c);
  for (const ndac::Param& q : p.params) {
    printf("param %s", q.name.c_str());
    for (int d : q.shape) printf(" %d", d);
    printf("\n");
    if (p.find(q.name.c_str()) != (int)(&q - p.params.data())) return fail("find", p.find(q.name.c_str()), &q - p.params.data());
  }
  if (p.find("no.such.parameter") != -1) return fail("find of an unknown name", p.find("no.such.parameter"), -1);
  if (check_stack("enc", p, p.enc, 1, p.hop) || check_stack("dec", p, p.dec, c.latent_dim, 1)) return 1;
  if (p.enc.back().Co != c.latent_dim || p.dec.back().Co != 1 || !p.dec.back().tanh_out) return fail("stack ends", p.enc.back().Co, p.dec.back().Co);
  printf("hop %d\nup %d\n", p.hop, p.up);
  for (int i = 9; i + 1 < argc; i += 2) {
    const long long v = atoll(argv[i + 1]);
    if (!strcmp(argv[i], "len")) printf("len %lld %lld\n", v, p.latent_frames(v));
    else if (!strcmp(argv[i], "frames")) printf("frames %lld %lld\n", v, p.decoded_length(v));
    else if (!strcmp(argv[i], "slot")) printf("slot %lld %lld\n", v, p.slot_elems(v));
    else return 2;
  }
  printf("whole_frames %s\n", p.whole_frames_error.empty() ? "ok" : p.whole_frames_error.c_str());
  printf("even_rates %s\n", p.even_rates_error.empty() ? "ok" : p.even_rates_error.c_str());
  int l = 0, r = 0;
  p.encode_halo(&l, &r);
  printf("encode_halo %d %d\n", l, r);
  p.decode_halo(&l, &r);
  printf("decode_halo %d %d\n", l, r);
  return 0;
}
