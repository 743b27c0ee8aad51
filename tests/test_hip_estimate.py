"""csrc/estimate.hip -- fd_select_f32 and fd_estimate_pair_stats (include/flowdec_hip.h "Parameter estimation"), flowdec_amd/estimate.py and
flowdec_amd/estimate_cli.py on the GPU.

(a) fd_select_f32 is EXACT: bit for bit np.partition(host copy, rank)[rank] at ranks 0, n - 1, floor((n - 1) 0.997) and that + 1, for sizes
    around the vector width, the workgroup and the grid, constant arrays, arrays whose two neighbouring ranks part at the first / at the
    last radix pass, and zeros, -0.0 (counts as +0.0: the host copy holds +0.0), denormals and +inf; from pointers of every alignment;
    a permuted copy gives the same bits; one NaN or one negative value gives bad_out == 1.
(b) fd_estimate_pair_stats: normfac == max|y| + 1e-5 in float32, bit for bit (a silent y gives 1e-5, not 1); |X_c| bit for bit the
    float64-sqrt magnitude of the plain fd_stft_compress(normalize = 0, beta = 1) of the pre-divided clean clips; band_sq against math.fsum
    of the float32-component squared differences of those downloaded spectra, with the bound of test_hip_metrics.py (a): the terms
    dr^2, di^2 are exact in float64, so the kernel's 2 T - 1 additions are all the error there is: C1 n u sum|t_i|, n = 2 T, C1 = 4.
(c) A pair's three outputs have the same bits alone, in a batch and in the reversed batch.
(d) Refusals: FD_EINVAL with a message, nothing launched.
(e) Golden g32_estimate_params.npz: estimate_params on the rebuilt corpus against the reference's float32 numbers, each within
    4 |ref_f32 - ref_f64| / |ref_f64| (floored at 4 float32 eps): the reference's own float32 error, times 4 because the DFT GEMM orders
    its 1534-term sums differently from the reference's FFT -- an error of the reference's own order, not a smaller one.
(f) estimate_cli end to end: the reference's file names, its printed numbers, and a second run that only prints the file.
"""
import ctypes as C
import io
import math
import os

import numpy as np
import pytest
import torch

import estimate_corpus as EC
from conftest import load_golden
from test_hip_stft import dev, report

pytestmark = pytest.mark.gpu

U64 = 2.0 ** -53
C1 = 4.0
EPS32 = float(np.finfo(np.float32).eps)
FD_EINVAL = -1


def L_():
    from flowdec_amd import _lib
    return _lib


def lib():
    return L_().load()


# ---- (a) select -------------------------------------------------------------------------------------------------------------------------
def call_select(values, ranks):
    """device float32 tensor (any 4-byte alignment), ranks -> (out float32 [R] as uint32 bits, bad_out)."""
    l = L_()
    R = len(ranks)
    nws = lib().fd_select_workspace_bytes(R)
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    out = torch.full((R,), 7.0, dtype=torch.float32, device="cuda")
    bad = torch.full((1,), -5, dtype=torch.int64, device="cuda")
    l.check(lib().fd_select_f32(l.ptr(values), values.numel(), (C.c_longlong * R)(*ranks), R, l.ptr(out), l.ptr(bad), l.ptr(ws), nws, l.stream()))
    return out.cpu().numpy().view(np.uint32), int(bad.item())


def ranks_of(n):
    k = (n - 1) * 997 // 1000
    return [0, n - 1, k, min(k + 1, n - 1)]


def check_select(a, what):
    """a: host float32 array of non-negative values (-0.0 allowed) -> asserts every rank bit for bit, returns the bits."""
    n = len(a)
    host = a + np.float32(0.0)                      # -0.0 -> +0.0, everything else unchanged
    ranks = ranks_of(n)
    got, bad = call_select(dev(a), ranks)
    assert bad == 0, (what, bad)
    part = np.partition(host, sorted(set(ranks)))
    want = part[ranks].view(np.uint32)
    assert np.array_equal(got, want), f"{what}: n = {n} ranks {ranks}: got {got} want {want}"
    return got


SELECT_SIZES = [1, 2, 255, 256, 257, 65537, 3000001]


@pytest.mark.parametrize("n", SELECT_SIZES)
def test_select_exact_sizes(n):
    rng = np.random.default_rng(n)
    a = (np.abs(rng.standard_normal(n)) ** 0.3).astype(np.float32)
    bits = check_select(a, "|randn|^0.3")
    assert np.array_equal(check_select(rng.permutation(a), "permuted"), bits)


def test_select_exact_special_arrays():
    rng = np.random.default_rng(11)
    n = 70001
    k = ranks_of(n)[2]
    check_select(np.full(n, 0.731, np.float32), "all equal")                                # one bucket holds everything in every pass
    # ranks k and k + 1 part at the FIRST pass (top byte 0x3f | 0x40) / only at the LAST (low byte 0x10 | 0x11)
    for what, lo, hi in (("first-pass split", 0x3FC00000, 0x40200000), ("last-pass split", 0x3F800010, 0x3F800011)):
        a = np.where(np.arange(n) <= k, np.uint32(lo), np.uint32(hi)).astype(np.uint32).view(np.float32)
        a = rng.permutation(a)
        got = check_select(a, what)
        assert got[2] == lo and got[3] == hi
    # zeros of both signs, denormals, the smallest normal, +inf among ordinary values
    special = np.array([0.0, -0.0, 1e-45, 3e-42, 1.1e-38, 1.17549435e-38, np.inf, 0.5, 2.0], np.float32)
    a = special[rng.integers(0, len(special), n)]
    a[rng.integers(0, n, n // 4)] = (np.abs(rng.standard_normal(n // 4)) ** 0.3).astype(np.float32)
    got = check_select(a, "special values")
    assert got[0] == 0 and got[1] == 0x7F800000                                             # +0.0 bits (never -0.0), +inf
    check_select(np.array([-0.0, -0.0, -0.0], np.float32), "only -0.0")
    check_select(np.array([1e-45, 0.0, 1e-45, np.inf], np.float32), "tiny")


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_select_unaligned_pointer(offset):
    rng = np.random.default_rng(offset)
    a = (np.abs(rng.standard_normal(65537 + offset)) ** 0.3).astype(np.float32)
    d = dev(a)
    assert d.data_ptr() % 16 == 0
    for n in (65537, 5, 2):
        ranks = ranks_of(n)
        got, bad = call_select(d[offset:offset + n], ranks)
        want = np.partition(a[offset:offset + n], sorted(set(ranks)))[ranks].view(np.uint32)
        assert bad == 0 and np.array_equal(got, want), (offset, n)


def test_select_counts_bad_values():
    rng = np.random.default_rng(3)
    a = (np.abs(rng.standard_normal(10007)) ** 0.3).astype(np.float32)
    for v in (np.nan, -1e-3, -np.inf):
        b = a.copy()
        b[4321] = v
        assert call_select(dev(b), [0, 10006])[1] == 1
    b = a.copy()
    b[[0, 5000, 10006]] = [np.nan, -2.0, -0.0]
    assert call_select(dev(b), [5])[1] == 2                                                  # -0.0 is not bad
    from flowdec_amd import estimate as E
    with pytest.raises(ValueError, match="2 of the 10007 values are negative or NaN"):
        E.select_f32(dev(b), [5])
    assert E.select_f32(dev(a), [0, 10006]).tolist() == [a.min(), a.max()]


# ---- (b) pair statistics ----------------------------------------------------------------------------------------------------------------
PAIR_SHAPES = [(126, 32, 1000, 3), (1534, 384, 96000, 2)]       # n_fft, hop, L, B
ALPHA = 0.3


def make_pairs(n_fft, hop, Lc, B):
    """B pairs of float32 clips; the last pair of the small shape has a SILENT y."""
    rng = np.random.default_rng(n_fft + B)
    xs = [(0.1 * (b + 1) * rng.standard_normal(Lc)).astype(np.float32) for b in range(B)]
    ys = [(x + 0.02 * rng.standard_normal(Lc)).astype(np.float32) for x in xs]
    if B == 3:
        ys[2] = np.zeros(Lc, np.float32)
    return xs, ys


def call_pair_stats(n_fft, hop, xs, ys, with_abs=True):
    """lists of float32 clips -> (normfac [B] f32, absx [B, F, T] f32 or None, band_sq [B, F] f64) of ONE call."""
    from flowdec_amd import ops
    l = L_()
    x, y = dev(np.stack(xs)), dev(np.stack(ys))
    B, Lc = x.shape
    F, T = n_fft // 2 + 1, 1 + Lc // hop
    nws = lib().fd_estimate_workspace_bytes(B, Lc, n_fft, hop)
    assert nws > 0
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    nf = torch.full((B,), 7.0, dtype=torch.float32, device="cuda")
    ab = torch.full((B, F, T), 7.0, dtype=torch.float32, device="cuda") if with_abs else None
    bs = torch.full((B, F), 7.0, dtype=torch.float64, device="cuda")
    l.check(lib().fd_estimate_pair_stats(ops.stft_plan(n_fft, hop, "cuda"), l.ptr(x), l.ptr(y), B, Lc, ALPHA, l.ptr(nf), l.ptr(ab), l.ptr(bs), l.ptr(ws),
                                         nws, l.stream()))
    return nf.cpu().numpy(), (ab.cpu().numpy() if with_abs else None), bs.cpu().numpy()


def compressed(n_fft, hop, clips):
    """The plain front end on clips as they are: fd_stft_compress(normalize = 0, beta = 1) -> complex64 [B, F, T]."""
    from flowdec_amd import ops
    Y, nf, T = ops.stft_compress(dev(np.stack(clips)), n_fft=n_fft, hop=hop, alpha=ALPHA, beta=1.0, normalize=False)
    assert bool((nf == 1.0).all())
    return Y[:, 0, :, :T].cpu().numpy()


@pytest.mark.parametrize("n_fft,hop,Lc,B", PAIR_SHAPES)
def test_pair_stats_operator_level(n_fft, hop, Lc, B):
    xs, ys = make_pairs(n_fft, hop, Lc, B)
    nf, ab, bs = call_pair_stats(n_fft, hop, xs, ys)
    F, T = n_fft // 2 + 1, 1 + Lc // hop
    want_nf = np.array([np.float32(np.abs(y).max()) + np.float32(1e-5) for y in ys], np.float32)
    assert want_nf.dtype == np.float32 and np.array_equal(nf.view(np.uint32), want_nf.view(np.uint32)), (nf, want_nf)
    if B == 3:
        assert nf[2] == np.float32(1e-5) and nf[2] != 1.0                      # no zero guard here
    Xc = compressed(n_fft, hop, [x / f for x, f in zip(xs, want_nf)])          # float32 / float32: sample by sample, as the kernel divides
    Yc = compressed(n_fft, hop, [y / f for y, f in zip(ys, want_nf)])
    assert Xc.shape == (B, F, T) and Xc.dtype == np.complex64 and np.isfinite(Xc.view(np.float32)).all()
    want_ab = np.sqrt(Xc.real.astype(np.float64) ** 2 + Xc.imag.astype(np.float64) ** 2).astype(np.float32)
    assert np.array_equal(ab.view(np.uint32), want_ab.view(np.uint32)), f"{(ab != want_ab).sum()} of {ab.size} magnitudes differ"
    dr, di = (Yc.real - Xc.real), (Yc.imag - Xc.imag)                          # float32 per component: complex64 subtraction
    assert dr.dtype == np.float32
    terms = np.concatenate([dr.astype(np.float64) ** 2, di.astype(np.float64) ** 2], axis=-1)       # [B, F, 2 T], each exact
    worst = 0.0
    for b in range(B):
        for f in range(F):
            ref = math.fsum(terms[b, f])
            bound = C1 * (2 * T) * U64 * ref                                  # the terms are non-negative: sum|t_i| = the sum
            err = abs(bs[b, f] - ref)
            assert err <= bound, (b, f, bs[b, f], ref, bound)
            worst = max(worst, err / max(bound, 1e-300))
    assert (bs > 0).all()
    # absx_out may be NULL: the same band sums
    nf2, _, bs2 = call_pair_stats(n_fft, hop, xs, ys, with_abs=False)
    assert np.array_equal(nf2.view(np.uint32), nf.view(np.uint32)) and np.array_equal(bs2.view(np.uint64), bs.view(np.uint64))
    report(f"estimate pair_stats n_fft={n_fft} hop={hop} L={Lc} B={B}: normfac and |X_c| bit-exact; band_sq max err/bound = {worst:.3e} (C1 = {C1:g}, n = {2 * T})")


# ---- (c) batch invariance ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,hop,Lc,B", PAIR_SHAPES)
def test_pair_stats_batch_invariance(n_fft, hop, Lc, B):
    xs, ys = make_pairs(n_fft, hop, Lc, B)
    alone = [call_pair_stats(n_fft, hop, [x], [y]) for x, y in zip(xs, ys)]

    def check(order):
        nf, ab, bs = call_pair_stats(n_fft, hop, [xs[i] for i in order], [ys[i] for i in order])
        for r, i in enumerate(order):
            assert nf[r].view(np.uint32) == alone[i][0][0].view(np.uint32)
            assert np.array_equal(ab[r].view(np.uint32), alone[i][1][0].view(np.uint32)), f"pair {i} at row {r} of {len(order)}: |X_c| differs from its one-pair call"
            assert np.array_equal(bs[r].view(np.uint64), alone[i][2][0].view(np.uint64)), f"pair {i} at row {r} of {len(order)}: band_sq differs from its one-pair call"

    check(list(range(B)))
    check(list(range(B))[::-1])


# ---- (d) refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    from flowdec_amd import ops
    l = L_()
    n_fft, hop, B, Lc = 126, 32, 2, 1000
    F, T = n_fft // 2 + 1, 1 + Lc // hop
    x = torch.zeros(B, Lc, device="cuda")
    nws = lib().fd_estimate_workspace_bytes(B, Lc, n_fft, hop)
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    nf = torch.full((B,), 7.0, device="cuda")
    ab = torch.full((B, F, T), 7.0, device="cuda")
    bs = torch.full((B, F), 7.0, dtype=torch.float64, device="cuda")
    p, X, W, st = ops.stft_plan(n_fft, hop, "cuda"), l.ptr(x), l.ptr(ws), l.stream()
    NF, AB, BS = l.ptr(nf), l.ptr(ab), l.ptr(bs)

    def refused(rc, text):
        assert rc == FD_EINVAL and text in lib().fd_last_error(), (rc, lib().fd_last_error())

    f = lib().fd_estimate_pair_stats
    refused(f(None, X, X, B, Lc, ALPHA, NF, AB, BS, W, nws, st), b"null pointer")
    refused(f(p, None, X, B, Lc, ALPHA, NF, AB, BS, W, nws, st), b"null pointer")
    refused(f(p, X, None, B, Lc, ALPHA, NF, AB, BS, W, nws, st), b"null pointer")
    refused(f(p, X, X, B, Lc, ALPHA, None, AB, BS, W, nws, st), b"null pointer")
    refused(f(p, X, X, B, Lc, ALPHA, NF, AB, None, W, nws, st), b"null pointer")
    refused(f(p, X, X, B, Lc, ALPHA, NF, AB, BS, None, nws, st), b"null pointer")
    refused(f(p, X, X, 0, Lc, ALPHA, NF, AB, BS, W, nws, st), b"bad batch")
    refused(f(p, X, X, B, 0, ALPHA, NF, AB, BS, W, nws, st), b"bad batch")
    refused(f(p, X, X, B, n_fft // 2, ALPHA, NF, AB, BS, W, nws, st), b"cannot be reflect-padded")
    refused(f(p, X, X, B, Lc, 0.0, NF, AB, BS, W, nws, st), b"alpha must be positive")
    refused(f(p, X, X, B, Lc, ALPHA, NF, AB, BS, W, nws - 1, st), b"workspace too small")
    assert lib().fd_estimate_workspace_bytes(0, Lc, n_fft, hop) == 0 and lib().fd_estimate_workspace_bytes(B, Lc, 125, hop) == 0

    n = 1000
    v = torch.rand(n, device="cuda")
    out = torch.full((8,), 7.0, device="cuda")
    bad = torch.full((1,), 7, dtype=torch.int64, device="cuda")
    sws_n = lib().fd_select_workspace_bytes(2)
    sws = torch.empty(sws_n, dtype=torch.uint8, device="cuda")
    V, O, Bd, SW = l.ptr(v), l.ptr(out), l.ptr(bad), l.ptr(sws)
    rk = lambda *r: (C.c_longlong * len(r))(*r)
    s = lib().fd_select_f32
    refused(s(None, n, rk(0, 1), 2, O, Bd, SW, sws_n, st), b"null pointer")
    refused(s(V, n, None, 2, O, Bd, SW, sws_n, st), b"null pointer")
    refused(s(V, n, rk(0, 1), 2, None, Bd, SW, sws_n, st), b"null pointer")
    refused(s(V, n, rk(0, 1), 2, O, None, SW, sws_n, st), b"null pointer")
    refused(s(V, n, rk(0, 1), 2, O, Bd, None, sws_n, st), b"null pointer")
    refused(s(V, n, rk(0, 1), 0, O, Bd, SW, sws_n, st), b"0 ranks")
    refused(s(V, n, rk(*range(9)), 9, O, Bd, SW, lib().fd_select_workspace_bytes(8), st), b"9 ranks")
    refused(s(V, 0, rk(0, 1), 2, O, Bd, SW, sws_n, st), b"n = 0 values")
    refused(s(V, n, rk(0, n), 2, O, Bd, SW, sws_n, st), b"is outside [0, 1000)")
    refused(s(V, n, rk(-1, 1), 2, O, Bd, SW, sws_n, st), b"is outside [0, 1000)")
    refused(s(V, n, rk(0, 1), 2, O, Bd, SW, sws_n - 1, st), b"workspace too small")
    assert lib().fd_select_workspace_bytes(0) == 0 and lib().fd_select_workspace_bytes(9) == 0
    torch.cuda.synchronize()
    assert bool((nf == 7.0).all()) and bool((ab == 7.0).all()) and bool((bs == 7.0).all()) and bool((out == 7.0).all()) and int(bad.item()) == 7
    # the Python layer names what is wrong
    from flowdec_amd import estimate as E
    with pytest.raises(ValueError, match="pair 1 has 999 / 999 samples, pair 0 has 1000"):
        E.estimate_params([torch.zeros(1000), torch.zeros(999)], [torch.zeros(1000), torch.zeros(999)], alpha=0.3, n_fft=126, hop=32)
    with pytest.raises(ValueError, match="cannot be reflect-padded"):
        E.estimate_params([torch.zeros(60)], [torch.zeros(60)], alpha=0.3, n_fft=126, hop=32)


# ---- (e) the golden ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("estimate_corpus"))
    pairs = EC.build(d)
    assert EC.hashes(d) == [str(h) for h in load_golden("g32_estimate_params.npz")["hashes"]]
    return pairs


def golden_tolerance(g, key):
    f32, f64 = g[key + "_f32"].astype(np.float64), g[key + "_f64"].astype(np.float64)
    return max(4.0 * float(np.max(np.abs(f32 - f64) / np.abs(f64))), 4.0 * EPS32)


def test_golden_estimate_params(corpus):
    from flowdec_amd import estimate as E
    from flowdec_amd.eval_cli import load_mono
    g = load_golden("g32_estimate_params.npz")
    with open(corpus) as f:
        lines = [l.strip() for l in f.readlines()]
    idx, pairs = E.select_pairs(lines, 8, 302, EC.DELIM)
    assert idx == g["sel"].tolist()
    xs, ys = [], []
    for fx, fy in pairs:
        x, y, _ = E.crop_or_pad_pair(load_mono(fx, 48000), load_mono(fy, 48000), 96000, name=fx)
        xs.append(x); ys.append(y)
    kw = dict(alpha=0.3, n_fft=1534, hop=384, batch_pairs=3)                    # 3: batches of 3, 3 and 2 pairs
    glob = E.estimate_params(xs, ys, **kw)
    band = E.estimate_params(xs, ys, per_band=True, **kw)
    assert glob.n_bins == 8 * 768 * 251 and band.sigma_y.shape == (768,) and band.sigma_y.dtype == np.float32 and band.rmses.shape == (8, 768)
    assert (band.abs_quantile_x, band.max_abs_x, band.beta) == (glob.abs_quantile_x, glob.max_abs_x, glob.beta)
    assert glob.sigma_y == glob.rmse_quantile / 3 and np.array_equal(band.sigma_y, band.rmse_quantile / 3)
    got = {"q_x": glob.abs_quantile_x, "max_x": glob.max_abs_x, "beta": glob.beta, "rmse_q": glob.rmse_quantile, "rmse_max": glob.rmse_max,
           "sigma_y": glob.sigma_y, "curve": band.sigma_y.astype(np.float64), "rmses": glob.rmses}
    failed = []
    for key, val in got.items():
        ref = g[key + "_f32"].astype(np.float64)
        err, tol = float(np.max(np.abs(val - ref) / np.abs(ref))), golden_tolerance(g, key)
        report(f"estimate golden g32 {key}: max rel err vs reference float32 = {err:.3e}, tolerance 4 |f32 - f64| / |f64| = {tol:.3e}, ratio {err / tol:.3f}")
        if not err <= tol:
            failed.append((key, err, tol))
    assert not failed, failed


# ---- (f) the command line ---------------------------------------------------------------------------------------------------------------
def test_estimate_cli_end_to_end(corpus, tmp_path, monkeypatch):
    from flowdec_amd import estimate as E, estimate_cli as CLI
    g = load_golden("g32_estimate_params.npz")
    pairs = tmp_path / "pairs.txt"
    pairs.write_text(open(corpus).read())
    common = ["--pairs-file", str(pairs), "--alpha", "0.3", "--nfft", "1534", "--hop", "384", "--n-samples", "8", "--seed", "302"]
    stem = "flowdec_autoparams_nfft1534_hop384_alpha0.3_seed302_n8"

    def run(flags):
        buf = io.StringIO()
        res = CLI.run(common + flags, out=buf)
        return res, buf.getvalue().splitlines()

    res, text = run([])
    assert res is not None and sorted(os.listdir(tmp_path)) == sorted(["pairs.txt", stem + ".txt"])
    assert text[0] == f"Input pairs file: {pairs}" and text[1].startswith("Args: Namespace(") and text[2] == "=== Results ==="
    assert EC.printed_numbers(text[3:]) == EC.printed_numbers([str(l) for l in g["lines_global"]]) and len(text) == 6
    assert [EC.printed_numbers([a]) for a in text[3:]] == [EC.printed_numbers([str(b)]) for b in g["lines_global"]]
    assert (tmp_path / (stem + ".txt")).read_text().splitlines() == text

    res, text = run(["--per-band"])
    npy = stem + "_perbandsigy_perband.npy"
    assert sorted(os.listdir(tmp_path)) == sorted(["pairs.txt", stem + ".txt", stem + "_perband.txt", npy])
    assert [l.replace(str(tmp_path), "{DIR}") for l in text[3:]] == [str(l) for l in g["lines_perband"]]
    curve = np.load(tmp_path / npy)
    assert curve.shape == (768,) and curve.dtype == np.float32 and np.array_equal(curve, res.sigma_y)

    # a second run without --overwrite prints the file and computes nothing
    def boom(*a, **k):
        raise AssertionError("estimate_params ran although the results file exists")
    monkeypatch.setattr(E, "estimate_params", boom)
    again, text2 = run(["--per-band"])
    assert again is None and text2 == text == (tmp_path / (stem + "_perband.txt")).read_text().splitlines()
    with pytest.raises(AssertionError, match="although the results file exists"):
        run(["--per-band", "--overwrite"])
