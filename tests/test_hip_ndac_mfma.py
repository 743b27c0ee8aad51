"""csrc/ndac_mfma.hip -- the codec's matrix-core convolution (split-bf16 operands, three products, f32 accumulation) -- tested on its own
through fd_ndac_mfma_conv1d, against float64 references of the same operation.

(a) Exact data.  x and w are bf16-exact (their lo terms are zero) on power-of-two grids, bias and residual lie on the grid of the
    products, and every partial sum stays below 2^24 grid steps (asserted for each case).  Then every float32 sum is exact in any order,
    and the output must EQUAL oracle/ndac_oracle.py's float64 convolution: zero mismatches, for every (MT, S, NT) instantiation,
    transposed stride and FULL / guarded epilogue (test_variant_coverage), ragged and tile-multiple lengths, partial strided chunks.
(b) The same with x carrying a nonzero lo term (w bf16-exact), and the reverse: pins the al*bh and ah*bl products one at a time.
(c) Random float32 data against a deterministic worst-case bound; the measured relative L2 error goes into the parity report.
(d) The Snake second output against float64 Snake of the kernel's own first output.
(e) Bit identity: NT = 1 vs NT = 2, a clip alone vs in a batch, and the exact vector path (fd_conv1d / fd_conv_transpose1d) on exact data.
(f) Host-side refusals leave the outputs untouched."""
import math
import zlib

import numpy as np
import pytest
import torch

from oracle import ndac_oracle as N
from test_hip_ops import dev, report
from test_ndac_mfma_cpu import variant as variant_rule

pytestmark = pytest.mark.gpu

FD_EINVAL = -1


def ops():
    from flowdec_amd import ops as _ops
    return _ops


def geometry(B, Ci, T, Co, K, s, p, d, tr):
    """(To, N, ostride, ooff, nphase): GEMM column n of phase r is output position n * ostride + r + ooff (ndac_mfma.hip)."""
    if tr:
        return (T - 1) * s - 2 * p + K, T + K // s - 1, s, -p, s
    if s > 1:
        To = (T + 2 * p - K) // s + 1
        return To, To, 1, 0, 1
    To = T + 2 * p - d * (K - 1)
    return To, To, 1, 0, 1


def epilogue_kinds(case):
    """Which epilogues the launch's waves take: True = FULL (every column of the wave's tiles is a real output), False = guarded."""
    _, B, Ci, T, Co, K, s, p, d, tr = case
    v = ops().ndac_mfma_variant(B, Ci, T, Co, K, stride=s, pad=p, dil=d, transposed=tr)
    To, Ncol, ostride, ooff, nphase = geometry(B, Ci, T, Co, K, s, p, d, tr)
    n = np.arange(v["grid"][0] * 128 * v["NT"]).reshape(-1, 4, v["NT"], 32)     # [workgroup][wave][tile][lane]
    kinds = set()
    for r in range(nphase):
        t = n * ostride + r + ooff
        ok = (n < Ncol) & (t >= 0) & (t < To)
        kinds |= set(ok.all(axis=(2, 3)).ravel().tolist())
    return kinds


def coverage_key(case, full):
    _, B, Ci, T, Co, K, s, p, d, tr = case
    v = ops().ndac_mfma_variant(B, Ci, T, Co, K, stride=s, pad=p, dil=d, transposed=tr)
    return (v["MT"], v["S"], v["NT"], s if tr else 0, full)


def nterms(case):
    """Products per output: Ci K (stride 1, strided), Ci K / s (transposed: one tap in s per phase)."""
    _, B, Ci, T, Co, K, s, p, d, tr = case
    return Ci * (K // s if tr else K)


def run(case, x, w, bias, residual=None, want_out=True, alpha=None, want_act=False):
    """fd_ndac_mfma_conv1d; outputs start as NaN so that a position the kernel does not write is a mismatch."""
    _, B, Ci, T, Co, K, s, p, d, tr = case
    To = geometry(B, Ci, T, Co, K, s, p, d, tr)[0]
    packed = torch.from_numpy(ops().ndac_mfma_pack_weights(w, s, tr).view(np.int16)).cuda()
    out = torch.full((B, Co, To), float("nan"), device="cuda") if want_out else None
    act = torch.full((B, Co, To), float("nan"), device="cuda") if want_act else None
    dx, db = dev(x), dev(bias)
    dr = dev(residual) if residual is not None else None
    da = dev(alpha) if alpha is not None else None
    ops().ndac_mfma_conv1d(dx, packed, db, Co, K, stride=s, pad=p, dil=d, transposed=tr, residual=dr, out=out, out_act=act, alpha_out=da)
    torch.cuda.synchronize()
    return (out.cpu().numpy() if want_out else None), (act.cpu().numpy() if want_act else None)


def oracle_conv(case, x, w, b):
    _, B, Ci, T, Co, K, s, p, d, tr = case
    return N.conv_transpose1d(x, w, b, stride=s, padding=p) if tr else N.conv1d(x, w, b, stride=s, padding=p, dilation=d)


# --------------------------------------------------------------------------------------------------------------------------------------
# exact data
# --------------------------------------------------------------------------------------------------------------------------------------
def ints(rng, m, shape):
    return rng.integers(-m, m + 1, shape).astype(np.float64)


# mode -> (x integer range, x grid, w integer range, w grid).  "bf16": both operands bf16-exact (5-bit integers).  "x16": x has up to
# 15 significant bits (a nonzero lo term whose split is exact: x - hi(x) is a multiple of x's grid below 2^7 of it), w 2-bit.  "w16": the reverse.
MODES = {"bf16": (31, 2.0 ** -4, 31, 2.0 ** -6), "x16": (2 ** 14 - 1, 2.0 ** -12, 3, 2.0 ** -2), "w16": (3, 2.0 ** -2, 2 ** 14 - 1, 2.0 ** -16)}


def exact_data(case, mode, with_residual=False):
    name, B, Ci, T, Co, K, s, p, d, tr = case
    rng = np.random.default_rng(zlib.crc32((name + mode).encode()))
    mx, gx, mw, gw = MODES[mode]
    g = gx * gw                                                                      # grid of every product
    x = (ints(rng, mx, (B, Ci, T)) * gx).astype(np.float32)
    w = (ints(rng, mw, (Ci, Co, K) if tr else (Co, Ci, K)) * gw).astype(np.float32)
    b = (ints(rng, 2 ** 12, Co) * g).astype(np.float32)
    To = geometry(B, Ci, T, Co, K, s, p, d, tr)[0]
    res = (ints(rng, 2 ** 12, (B, Co, To)) * g).astype(np.float32) if with_residual else None
    # the premise, asserted: operands on their grids; lo terms as the mode says; |partial sum| <= max|x| max_co sum|w| + |b| + |res| < 2^24 g
    for a, ga in ((x, gx), (w, gw), (b, g)) + (((res, g),) if with_residual else ()):
        assert np.array_equal(a / ga, np.round(a / ga))
    for a, want_lo in ((x, mode == "x16"), (w, mode == "w16")):
        t = torch.from_numpy(a)
        hi = t.to(torch.bfloat16).float()
        lo = (t - hi).to(torch.bfloat16).float()
        assert torch.equal(hi + lo, t)                                              # the hi + lo split is exact
        assert bool((lo != 0).any()) == want_lo
    aw = np.abs(w.astype(np.float64))                                              # (transposed: an output of phase r takes taps r, r + s, ..)
    wsum = max(aw[:, :, r::s].sum(axis=(0, 2)).max() for r in range(s)) if tr else aw.sum(axis=(1, 2)).max()
    bound = float(np.abs(x).max()) * wsum + float(np.abs(b).max()) + (float(np.abs(res).max()) if with_residual else 0.0)
    assert bound < 2.0 ** 24 * g, f"{name}: partial sums may reach {bound / g:.3g} grid steps (>= 2^24)"
    return x, w, b, res


def assert_equal_exact(name, got, ref):
    assert got.shape == ref.shape
    bad = got != ref                                                                # (NaN: a position the kernel did not write)
    n = int(bad.sum())
    report(f"ndac_mfma_exact_mismatches[{name}]", float(n), 0.5)
    if n:
        i = tuple(int(a[0]) for a in np.nonzero(bad))
        raise AssertionError(f"{name}: {n} of {ref.size} outputs differ from the float64 reference; first at [b, co, t] = {i}: "
                             f"{got[i]!r} != {ref[i]!r}")


STRIDES = (2, 4, 5, 8, 10)


def cover_cases():
    """One case per (MT, S, NT, transposed stride), N = 300 GEMM columns: full waves, a wave whose second tile is partial (NT = 2), and
    waves past the end -- both epilogues.  NT = 2 gets enough workgroups (wgs256 >= 512) from the batch size."""
    cases = []
    for mt in (2, 3):
        for nt in (1, 2):
            Co = {(2, 1): 128, (3, 1): 192, (2, 2): 256, (3, 2): 384}[(mt, nt)]
            ncob = Co // (32 * mt)
            forms = [("s1", 1, False)] + [("tr", s, True) for s in STRIDES] + [("str", s, False) for s in STRIDES]
            for kind, s, tr in forms:
                nphase = s if tr else 1
                B = 2 if nt == 1 else -(-512 // (2 * ncob * nphase))
                if kind == "s1":
                    case = (32, 300, 3, 1)                                          # Ci, T, K, pad
                elif tr:
                    case = (32, 299, 2 * s, math.ceil(s / 2))
                else:
                    K, p = 2 * s, math.ceil(s / 2)
                    case = (32 // s + 1, 299 * s + K - 2 * p, K, p)                 # Ci: one channel in the last chunk
                Ci, T, K, p = case
                cases.append((f"{kind if kind == 's1' else kind + str(s)}_mt{mt}_nt{nt}", B, Ci, T, Co, K, s, p, 1, tr))
    return cases


COVER_CASES = cover_cases()
EDGE_CASES = [  # name, B, Ci, T, Co, K, stride, pad, dilation, transposed
    ("s1_k1_ci1536", 1, 1536, 100, 96, 1, 1, 0, 1, False),
    ("s1_k7_ci1536", 1, 1536, 70, 96, 7, 1, 3, 1, False),
    ("s1_k7_d3_ci64", 2, 64, 513, 192, 7, 1, 9, 3, False),
    ("s1_k7_d9_ci32", 1, 32, 300, 128, 7, 1, 27, 9, False),
    ("s1_k7_d9_ci512", 1, 512, 200, 384, 7, 1, 27, 9, False),
    ("s1_k3_ci256", 2, 256, 129, 64, 3, 1, 1, 1, False),
    ("s1_tile_multiple", 1, 32, 256, 96, 7, 1, 3, 1, False),
    ("s1_n_below_32", 1, 32, 20, 96, 7, 1, 3, 1, False),
    ("s1_valid_pad0", 1, 32, 40, 64, 7, 1, 0, 3, False),
    ("s1_pad_beyond_halo", 1, 32, 50, 96, 3, 1, 5, 1, False),
] + [(f"tr{s}_T{T}", 1, 32 * (1 + T), T, 96 * (3 - T), 2 * s, s, math.ceil(s / 2), 1, True) for s in STRIDES for T in (1, 2)] + [
    ("str10_ci40", 1, 40, 1000, 96, 20, 10, 5, 1, False),
    ("str5_ci40", 2, 40, 503, 192, 10, 5, 3, 1, False),
    ("str8_ci9", 1, 9, 333, 128, 16, 8, 4, 1, False),
    ("str4_ci64", 1, 64, 1001, 64, 8, 4, 2, 1, False),
    ("str10_n_below_32", 1, 5, 100, 96, 20, 10, 5, 1, False),
    ("str2_ci1", 1, 1, 64, 64, 4, 2, 1, 1, False),
    ("str4_pad0", 1, 16, 401, 64, 8, 4, 0, 1, False),        # paddings other than the codec's ceil(s / 2)
    ("str5_pad5", 1, 12, 300, 96, 10, 5, 5, 1, False),
    ("tr4_pad0", 1, 32, 50, 64, 8, 4, 0, 1, True),
    ("tr5_pad4", 1, 32, 40, 96, 10, 5, 4, 1, True),
]
EXACT_CASES = COVER_CASES + EDGE_CASES


@pytest.mark.parametrize("case", EXACT_CASES, ids=[c[0] for c in EXACT_CASES])
def test_exact_data_equals_float64(case):
    name, B, Ci, T, Co, K, s, p, d, tr = case
    v = ops().ndac_mfma_variant(B, Ci, T, Co, K, stride=s, pad=p, dil=d, transposed=tr)
    assert (v["MT"], v["S"], v["NT"], *v["grid"]) == variant_rule(B, Ci, T, Co, K, s, p, d, tr)
    if name in dict((c[0], c) for c in COVER_CASES):
        kind, mt, nt = name.split("_")[0], int(name.split("_mt")[1][0]), int(name.split("_nt")[1][0])
        assert (v["MT"], v["S"], v["NT"]) == (mt, s if kind.startswith("str") else 0, nt)
    x, w, b, _ = exact_data(case, "bf16")
    out, _ = run(case, x, w, b)
    assert_equal_exact(name, out, oracle_conv(case, x, w, b))


LO_CASES = [
    ("s1_k3", 1, 32, 300, 96, 3, 1, 1, 1, False),
    ("s1_k7_d9", 1, 32, 200, 128, 7, 1, 27, 9, False),
    ("s1_k3_nt2", 64, 32, 300, 384, 3, 1, 1, 1, False),
    ("tr4", 2, 32, 77, 192, 8, 4, 2, 1, True),
    ("tr10", 1, 32, 50, 64, 20, 10, 5, 1, True),
    ("str2", 1, 17, 500, 128, 4, 2, 1, 1, False),
    ("str5", 1, 7, 1003, 96, 10, 5, 3, 1, False),
    ("str10", 2, 7, 2000, 64, 20, 10, 5, 1, False),
]


@pytest.mark.parametrize("mode", ["x16", "w16"])
@pytest.mark.parametrize("case", LO_CASES, ids=[c[0] for c in LO_CASES])
def test_lo_terms_exact(case, mode):
    """x16: x = hi + lo with lo != 0, w bf16-exact -- the result needs the ah*bl product (weight hi x input lo).  w16: the reverse,
    the al*bh product.  The dropped al*bl term is zero in both, so the output still equals the float64 reference bit for bit."""
    x, w, b, _ = exact_data(case, mode)
    out, _ = run(case, x, w, b)
    assert_equal_exact(f"{case[0]}_{mode}", out, oracle_conv(case, x, w, b))


# --------------------------------------------------------------------------------------------------------------------------------------
# epilogues and the Snake second output
# --------------------------------------------------------------------------------------------------------------------------------------
SNAKE_ARG_MAX = 64.0        # |alpha v| of every asserted Snake output (no checkpoint is available offline to take the range from)
# __sinf / __builtin_amdgcn_rcpf carry no documented error bound in the ROCm device library on this toolchain: SNAKE_SIN_TOL bounds
# |sin^2 error| / (1 + |alpha v|) and was MEASURED once on the MI355X (empirical, ~4x margin; the measured value goes to the report).
SNAKE_SIN_TOL = 2.0 ** -21   # (measured: 1.1e-7 = 2^-23.1)


def snake_check(name, v, act, alpha):
    """out_act against float64 v + sin^2(alpha v) / (alpha + 1e-9) of the kernel's own first output v, where |alpha v| <= SNAKE_ARG_MAX:
    |act - ref| <= 2^-22 |ref| + SNAKE_SIN_TOL (1 + |alpha v|) / (alpha + 1e-9)."""
    a = alpha.astype(np.float64)[None, :, None]
    v64 = v.astype(np.float64)
    arg = np.abs(a * v64)
    inr = arg <= SNAKE_ARG_MAX
    inv = 1.0 / (a + 1e-9)
    ref = v64 + inv * np.sin(a * v64) ** 2
    e = (np.abs(act - ref) - 2.0 ** -22 * np.abs(ref)) / (inv * (1 + arg))
    worst = float(e[inr].max())
    report(f"ndac_mfma_snake_sin_err[{name}]", worst, SNAKE_SIN_TOL)
    assert np.isfinite(act[inr]).all() and worst <= SNAKE_SIN_TOL, f"{name}: Snake error {worst:.3g} (1 + |alpha v|) / alpha"


def alphas(Co):
    return np.geomspace(0.05, 20.0, Co).astype(np.float32)[np.random.default_rng(Co).permutation(Co)]


EPI_CASES = [c for c in COVER_CASES if c[0] in ("s1_mt3_nt2", "tr5_mt2_nt1", "str10_mt3_nt1", "str5_mt2_nt2", "tr8_mt3_nt2")]


@pytest.mark.parametrize("case", EPI_CASES, ids=[c[0] for c in EPI_CASES])
def test_epilogue_combinations(case):
    """Every combination the host accepts: out, out + out_act, out_act, residual + out + out_act, residual + out_act.  The raw output
    is exact (as in (a), the residual on the same grid); out_act is the Snake of it and the same bits whether or not out is written."""
    name = case[0]
    x, w, b, res = exact_data(case, "bf16", with_residual=True)
    ref = oracle_conv(case, x, w, b)
    alpha = alphas(case[4])
    o1, _ = run(case, x, w, b)
    assert_equal_exact(f"{name}_out", o1, ref)
    o2, a2 = run(case, x, w, b, alpha=alpha, want_act=True)
    assert_equal_exact(f"{name}_out_act", o2, ref)
    _, a3 = run(case, x, w, b, alpha=alpha, want_act=True, want_out=False)
    assert np.array_equal(a3, a2)
    o4, a4 = run(case, x, w, b, residual=res, alpha=alpha, want_act=True)
    assert_equal_exact(f"{name}_res_out_act", o4, ref + res)
    _, a5 = run(case, x, w, b, residual=res, alpha=alpha, want_act=True, want_out=False)
    assert np.array_equal(a5, a4)
    snake_check(f"{name}_res", o4, a4, alpha)


SNAKE_CASES = [("s1_k1", 1, 32, 4096, 96, 1, 1, 0, 1, False), ("tr2", 2, 32, 999, 192, 4, 2, 1, 1, True), ("str4", 1, 8, 8192, 128, 8, 4, 2, 1, False)]


@pytest.mark.parametrize("case", SNAKE_CASES, ids=[c[0] for c in SNAKE_CASES])
def test_snake_second_output(case):
    """alpha spread over [0.05, 20] (geometric) across the channels, outputs of unit scale (|v| up to ~5), so that |alpha v| covers
    [0, SNAKE_ARG_MAX] (asserted) and beyond (not asserted)."""
    name, B, Ci, T, Co, K, s, p, d, tr = case
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    x = rng.uniform(-1, 1, (B, Ci, T)).astype(np.float32)
    n = nterms(case)
    w = (rng.uniform(-1, 1, (Ci, Co, K) if tr else (Co, Ci, K)) * 3.0 / math.sqrt(n)).astype(np.float32)
    b = rng.uniform(-1, 1, Co).astype(np.float32)
    alpha = alphas(Co)
    v, act = run(case, x, w, b, alpha=alpha, want_act=True)
    arg = np.abs(alpha[None, :, None] * v)
    assert float(arg.max()) > SNAKE_ARG_MAX and (arg <= SNAKE_ARG_MAX).mean() > 0.9
    snake_check(name, v, act, alpha)


# --------------------------------------------------------------------------------------------------------------------------------------
# random float32 data
# --------------------------------------------------------------------------------------------------------------------------------------
RAND_CASES = [
    ("s1_k7_ci1536", 1, 1536, 100, 96, 7, 1, 3, 1, False),
    ("s1_k7_d3_ci768", 2, 768, 300, 384, 7, 1, 9, 3, False),
    ("s1_k1_ci96_nt2", 40, 96, 1000, 192, 1, 1, 0, 1, False),
    ("tr8_ci256", 2, 256, 40, 128, 16, 8, 4, 1, True),
    ("tr10_ci1536", 1, 1536, 7, 768, 20, 10, 5, 1, True),
    ("str10_ci40", 2, 40, 2000, 96, 20, 10, 5, 1, False),
    ("str2_ci64", 1, 64, 4000, 128, 4, 2, 1, 1, False),
    ("str5_ci256", 1, 256, 2000, 384, 10, 5, 3, 1, False),
]


def torch_conv64(case, x, w, b):
    _, B, Ci, T, Co, K, s, p, d, tr = case
    F = torch.nn.functional
    x, w = torch.from_numpy(x).double(), torch.from_numpy(w).double()
    b = torch.from_numpy(b).double() if b is not None else None
    y = F.conv_transpose1d(x, w, b, stride=s, padding=p) if tr else F.conv1d(x, w, b, stride=s, padding=p, dilation=d)
    return y.numpy()


@pytest.mark.parametrize("case", RAND_CASES, ids=[c[0] for c in RAND_CASES])
def test_random_data_within_worst_case_bound(case):
    """Elementwise |out - ref64| <= (3 2^-16 + 2^-30) A + (3 n + 2) 2^-24 (1.02 A + |b|), A = sum_i |w_i| |x_i| over the n = Ci K
    (transposed: Ci K / s) products of the output.  Derivation: hi = RNE_bf16(x) is within 2^-8 |x| of x, lo = RNE_bf16(x - hi)
    within 2^-8 |x - hi| of it, so x = hi + lo + e with |e| <= 2^-16 |x|, the same for w.  wh xh + wh xl + wl xh differs from w x by
    wl xl + (wh + wl) e_x + e_w x, at most (3 2^-16 + 2^-32) |w| |x|; each bf16 x bf16 product is exact in float32.  The 3 n products
    and the bias are summed in float32 in some order: at most 3 n + 1 roundings, plus the final bias add, each within 2^-24 of a
    partial sum, and every partial sum is at most (1 + 2^-8)^2 (1 + 2^-7) A + |b| <= 1.02 A + |b|.  Deterministic: it cannot flake.
    The measured relative L2 error goes to the parity report (the header's "~1e-6 relative per layer"; not asserted here)."""
    name, B, Ci, T, Co, K, s, p, d, tr = case
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    n = nterms(case)
    x = rng.standard_normal((B, Ci, T)).astype(np.float32)
    w = (rng.standard_normal((Ci, Co, K) if tr else (Co, Ci, K)) / math.sqrt(n)).astype(np.float32)
    b = rng.standard_normal(Co).astype(np.float32)
    out, _ = run(case, x, w, b)
    ref = torch_conv64(case, x, w, b)
    A = torch_conv64(case, np.abs(x), np.abs(w), None)
    bound = (3 * 2.0 ** -16 + 2.0 ** -30) * A + (3 * n + 2) * 2.0 ** -24 * (1.02 * A + np.abs(b)[None, :, None])
    err = np.abs(out.astype(np.float64) - ref)
    rel = float(np.linalg.norm(err) / np.linalg.norm(ref))
    report(f"ndac_mfma_random_rel_l2[{name}]", rel, float("inf"))
    report(f"ndac_mfma_random_err_over_bound[{name}]", float((err / bound).max()), 1.0)
    assert np.isfinite(out).all() and np.all(err <= bound), f"{name}: {int((err > bound).sum())} outputs beyond the bound"


# --------------------------------------------------------------------------------------------------------------------------------------
# bit identity
# --------------------------------------------------------------------------------------------------------------------------------------
IDENT_CASES = [  # name, B (NT = 2), Ci, T, Co, K, stride, pad, dilation, transposed
    ("s1_k7", 64, 32, 300, 384, 7, 1, 3, 1, False),
    ("tr4", 40, 32, 299, 192, 8, 4, 2, 1, True),
    ("str8", 70, 5, 2400, 256, 16, 8, 4, 1, False),
]


@pytest.mark.parametrize("case", IDENT_CASES, ids=[c[0] for c in IDENT_CASES])
def test_nt_and_batch_bit_identity(case):
    """The same bits from NT = 2 (the whole batch) and NT = 1 (one clip alone, two clips): the K order of an output is the same."""
    name, B, Ci, T, Co, K, s, p, d, tr = case
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    x = rng.standard_normal((B, Ci, T)).astype(np.float32)
    n = nterms(case)
    w = (rng.standard_normal((Ci, Co, K) if tr else (Co, Ci, K)) / math.sqrt(n)).astype(np.float32)
    b = rng.standard_normal(Co).astype(np.float32)
    alpha = alphas(Co)
    assert ops().ndac_mfma_variant(B, Ci, T, Co, K, stride=s, pad=p, dil=d, transposed=tr)["NT"] == 2
    out, act = run(case, x, w, b, alpha=alpha, want_act=True)
    for b0, nb in ((0, 1), (B - 1, 1), (B // 2, 2)):
        sub = (name, nb) + case[2:]
        assert ops().ndac_mfma_variant(nb, Ci, T, Co, K, stride=s, pad=p, dil=d, transposed=tr)["NT"] == 1
        o1, a1 = run(sub, np.ascontiguousarray(x[b0:b0 + nb]), w, b, alpha=alpha, want_act=True)
        assert np.array_equal(o1, out[b0:b0 + nb]) and np.array_equal(a1, act[b0:b0 + nb]), f"{name}: clips {b0}..{b0 + nb - 1} differ"


VECTOR_CASES = [c for c in EXACT_CASES if c[0] in ("s1_k7_d3_ci64", "s1_k7_d9_ci32", "s1_k1_ci1536", "s1_k3_ci256", "tr2_T2", "tr10_T1",
                                                   "str10_ci40", "str5_ci40", "str8_ci9", "tr5_mt3_nt1", "tr8_mt2_nt1")]


@pytest.mark.parametrize("case", VECTOR_CASES, ids=[c[0] for c in VECTOR_CASES])
def test_exact_data_matches_vector_path(case):
    """On exact data both paths are exact: fd_ndac_mfma_conv1d and fd_conv1d / fd_conv_transpose1d (ndac.hip) give the same bits."""
    from flowdec_amd import _lib as L
    name, B, Ci, T, Co, K, s, p, d, tr = case
    x, w, b, _ = exact_data(case, "bf16")
    out, _ = run(case, x, w, b)
    vec = torch.full(out.shape, float("nan"), device="cuda")
    dx, dw, db = dev(x), dev(w), dev(b)
    if tr:
        rc = L.load().fd_conv_transpose1d(L.ptr(dx), L.ptr(dw), L.ptr(db), None, L.ptr(vec), B, Ci, T, Co, K, s, p, L.stream())
    else:
        rc = L.load().fd_conv1d(L.ptr(dx), L.ptr(dw), L.ptr(db), None, None, L.ptr(vec), B, Ci, T, Co, K, s, p, d, 0, L.stream())
    L.check(rc)
    assert np.array_equal(vec.cpu().numpy(), out), f"{name}: the matrix-core and vector paths differ on exact data"


# --------------------------------------------------------------------------------------------------------------------------------------
# refusals and coverage
# --------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_outputs_untouched():
    """Shapes the kernel does not support return FD_EINVAL with a message, and nothing is written.  (Buffers are sized for the
    nearest supported shape.  A residual without out_act is refused the same way: tests/test_ndac_mfma_cpu.py, in a process
    without a GPU.)"""
    from flowdec_amd import _lib as L
    lib = L.load()
    x = torch.zeros(2, 64, 128, device="cuda")
    wp = torch.zeros(1 << 20, dtype=torch.int16, device="cuda")
    bias, alpha = torch.zeros(96, device="cuda"), torch.ones(96, device="cuda")
    out = torch.full((2, 96, 1024), float("nan"), device="cuda")
    act = torch.full((2, 96, 1024), float("nan"), device="cuda")
    for Ci, T, K, s, p, d, tr, why in ((40, 128, 7, 1, 3, 1, 0, "unsupported"), (32, 128, 7, 3, 3, 1, 0, "unsupported"),
                                      (32, 128, 7, 1, 3, 26, 0, "unsupported"), (32, 100, 9, 2, 1, 1, 1, "unsupported"),
                                      (32, 100, 8, 4, 2, 2, 1, "unsupported"), (32, 5, 7, 1, 0, 1, 0, "empty output"),
                                      (5, 9, 20, 10, 0, 1, 0, "empty output")):
        rc = lib.fd_ndac_mfma_conv1d(L.ptr(x), L.ptr(wp), L.ptr(bias), None, L.ptr(out), L.ptr(act), L.ptr(alpha), 2, Ci, T, 96, K, s, p, d,
                                     tr, L.stream())
        assert rc == FD_EINVAL and why in lib.fd_last_error().decode(), (Ci, T, K, s, p, d, tr)
    torch.cuda.synchronize()
    assert bool(out.isnan().all()) and bool(act.isnan().all())


def full_coverage_set():
    forms = [(s, 0) for s in STRIDES] + [(0, t) for t in (0,) + STRIDES]    # (S, transposed stride)
    return {(mt, S, nt, t, full) for mt in (2, 3) for nt in (1, 2) for S, t in forms for full in (True, False)}


def test_variant_coverage():
    """The exact cases above execute every instantiated kernel -- 2 MT x 6 S x 2 NT, the S = 0 kernels for stride 1 and every
    transposed stride -- with both the FULL and the guarded epilogue."""
    got = {coverage_key(c, full) for c in EXACT_CASES for full in epilogue_kinds(c)}
    want = full_coverage_set()
    assert len(want) == 88
    assert got == want, f"missing {sorted(want - got)}"
