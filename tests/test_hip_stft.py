"""csrc/stft.hip -- the STFT / iSTFT of every enhance call (normalise, frame, DFT GEMM, compression; decompression, DFT GEMM,
overlap-add) -- tested piece by piece and as a whole against float64 references, at the production shapes and at the edges.

(a) The DFT GEMM alone (fd_stft_gemm_f32) on exact grid data: integer A in [-8, 8], B on a 1/4 grid in [-2, 2].  Every partial sum is a
    multiple of 1/4 below 2^22, exact in float32 in any order, so C must EQUAL the float64 product, for both tile widths.
(b) The tile width does not change a bit: rows of an M = 5377 call (BN = 128) equal the M = 5376 call (BN = 32) on random data.
(c) The forward spectrum (alpha = beta = 1, no normalisation: ComplexSTFT) against float64 rfft of the reflect-padded, windowed frames,
    within a worst-case bound per bin and frame.  Sparse impulse rows (clip ends, frame borders, the first and last k-blocks) make an
    indexing error show far above the bound even where the window is ~1e-3.
(d) normfac bit for bit (maximum at either end, the 1e-8 silence rule, ragged tails ignored) and the normalised spectrum.
(e) Fused and stand-alone compression give the same bits; fd_compress_spec against float64 within a stated number of ulps.
(f) The inverse on random complex spectra (a round trip cannot hide a shared error) against float64 irfft / window / overlap-add /
    envelope, within a worst-case bound per sample; lengths at or past the zero-envelope boundary are refused.
(g) A 32-clip ragged batch (BN = 128) against float64 per clip, with NaN behind every clip's end.

Measured relative L2 errors and the largest error / bound ratio go into the parity report; only the bounds are asserted."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from test_hip_ops import REPORT     # the parity report every GPU test module appends to

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NFFT, HOP = 1534, 384
# The worst-case bounds below are c * K * u * (sum of |terms|) with c = 2.  One output is a K-term float32 dot product: the table entry
# carries one rounding (<= u relative), the MFMA product at most one more, and the K - 1 additions of the running sum at most (K - 1) u
# of the sum of |terms| -- (K + 1) u in all, to first order.  The inverse adds at most 2 ceil(n_fft / hop) + 2 roundings (overlap-add,
# envelope, division), fewer than K.  c = 2 covers both with the second-order terms for every K >= 128 used here.
C_BOUND = 2.0


def ops():
    from flowdec_amd import ops as _ops
    return _ops


def lib():
    from flowdec_amd import _lib
    return _lib.load()


def report(line):
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    with open(REPORT, "a") as f:
        f.write(line + "\n")
    print(line)


def kpad(n_fft):
    return (n_fft + 2 + 127) // 128 * 128


def padded(T):
    return -(-T // 64) * 64


def hann(n_fft):
    k = np.arange(n_fft, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * k / (n_fft - 1))).astype(np.float32).astype(np.float64)


def gemm_bn(M, N, K):
    return 128 if -(-M // 128) * (N // 128) >= 512 else 32


# ---- float64 references -----------------------------------------------------------------------------------------------------------------
def stft_ref(x, n_fft, hop):
    """x [L] float64 -> (X [F, T] complex128 of torch.stft(center, reflect, sym-Hann float32 window), S [T] = sum_k |x_k| w_k per frame)."""
    pad, w = n_fft // 2, hann(n_fft)
    T = 1 + len(x) // hop
    xp = np.pad(x, pad, mode="reflect")
    fr = xp[hop * np.arange(T)[:, None] + np.arange(n_fft)[None, :]]
    return np.fft.rfft(fr * w, axis=-1).T, np.abs(fr) @ w


def istft_ref(Z, n_fft, hop, L):
    """Z [F, T] complex -> (y [L] float64 of torch.istft(center, length = L), G [L] = sum_t (2 w_n / n_fft) sum_j |Z_tj| overlapping each
    sample, env [L]).  irfft drops the imaginary parts of DC and Nyquist; the envelope is the overlap-add of the float32 w^2."""
    F, T = Z.shape
    w = hann(n_fft)
    w2 = (w.astype(np.float32) * w.astype(np.float32)).astype(np.float64)
    fr = np.fft.irfft(Z.T, n=n_fft, axis=-1) * w
    S = np.abs(Z.real).sum(0) + np.abs(Z.imag).sum(0)
    total = n_fft + hop * (T - 1)
    out, env, g = np.zeros(total), np.zeros(total), np.zeros(total)
    for t in range(T):
        out[hop * t:hop * t + n_fft] += fr[t]
        env[hop * t:hop * t + n_fft] += w2
        g[hop * t:hop * t + n_fft] += 2.0 * w / n_fft * S[t]
    s = slice(n_fft // 2, min(n_fft // 2 + L, total))
    assert env[s].min() >= 1e-11
    y, G, E = np.zeros(L), np.zeros(L), np.ones(L)
    n = s.stop - s.start
    y[:n], G[:n], E[:n] = out[s] / env[s], g[s], env[s]
    return y, G, E


def rel_l2(a, b):
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-300))


def check_forward(name, Y, x32, n_fft, hop, T_own=None):
    """Y: the kernel's [F, T_pad] complex64 spectrum of the float32 signal x32 (exactly what the framing kernel read): every bin within
    C_BOUND K u sum_k |x_k| w_k of float64, the frames behind T (T_own for a ragged clip) zero.  -> (rel L2, max error / bound)."""
    X, S = stft_ref(x32.astype(np.float64), n_fft, hop)
    T = X.shape[1]
    assert T_own is None or T_own == T
    got = Y[:, :T].astype(np.complex128)
    err = np.maximum(np.abs(got.real - X.real), np.abs(got.imag - X.imag))
    bound = C_BOUND * kpad(n_fft) * U * S[None, :]
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    bad = np.argwhere(~(err <= bound))
    assert bad.size == 0, f"{name}: {len(bad)} bins over the bound, first (f, t) = {bad[0].tolist()}: err {err[tuple(bad[0])]:.3e} bound {bound[tuple(bad[0])]:.3e}"
    assert not Y[:, T:].any(), f"{name}: frames behind T = {T} must be zero"
    return rel_l2(got, X), ratio


def check_inverse(name, y, Z, n_fft, hop, L):
    """y: the kernel's [>= L] output for spectrum Z [F, T] (alpha = beta = 1, no normfac): every sample within C_BOUND K u G / env of float64,
    samples from L on zero.  -> (rel L2, max error / bound)."""
    ref, G, env = istft_ref(Z.astype(np.complex128), n_fft, hop, L)
    err = np.abs(y[:L].astype(np.float64) - ref)
    bound = C_BOUND * kpad(n_fft) * U * G / env
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    bad = np.flatnonzero(~(err <= bound))
    assert bad.size == 0, f"{name}: {bad.size} samples over the bound, first s = {bad[0]}: err {err[bad[0]]:.3e} bound {bound[bad[0]]:.3e}"
    assert not y[L:].any()
    return rel_l2(y[:L].astype(np.float64), ref), ratio


# ---- signals ----------------------------------------------------------------------------------------------------------------------------
def impulse_ends(L):
    y = np.zeros(L, np.float32)
    for i, s in enumerate((0, 1, 2, L - 3, L - 2, L - 1)):
        y[s] = (1.0 + i) * (-1) ** i
    return y


def impulse_borders(L, n_fft, hop, seed):
    """One impulse per group of frames, at chosen in-frame positions k of frame t_j: both window ends, the first and last 16-sample
    k-blocks, the middle.  Consecutive impulses are >= n_fft apart, so no frame holds two."""
    ks = [1, 2, 3, 8, 15, 16, 17, n_fft // 2 - 1, n_fft // 2, n_fft // 2 + 1, n_fft - 2, n_fft - 3, n_fft - 8, n_fft - 15, n_fft - 16,
          n_fft - 17, (n_fft - 1) // 16 * 16, (n_fft - 1) // 16 * 16 - 1]
    rng = np.random.default_rng(seed)
    y = np.zeros(L, np.float32)
    step = -(-(2 * n_fft) // hop)
    j = 0
    while True:
        t = step * (j + 1)
        s = hop * t + ks[j % len(ks)] - n_fft // 2
        if s >= L:
            return y
        y[s] = rng.uniform(0.5, 2.0) * rng.choice((-1, 1))
        j += 1


def signals(B, L, n_fft, hop, seed):
    """B rows: Gaussian noise, the clip-end impulses, the frame-border impulses, then noise again."""
    rng = np.random.default_rng(seed)
    y = (0.1 * rng.standard_normal((B, L))).astype(np.float32)
    if B > 1:
        y[1] = impulse_ends(L)
    if B > 2:
        y[2] = impulse_borders(L, n_fft, hop, seed)
    return y


def random_spectra(B, F, T_pad, T, seed, nan_tail=True):
    """Random complex spectra [B, 1, F, T_pad], nonzero imaginary DC / Nyquist, NaN in the frames t >= T (they must not be read).  Row 1 is
    sparse: one bin per frame, cycling through DC, Nyquist and their neighbours -- a wrong DC / Nyquist factor shows far above the bound."""
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((B, 1, F, T_pad)) + 1j * rng.standard_normal((B, 1, F, T_pad))).astype(np.complex64)
    if B > 1:
        X[1] = 0
        bins = [0, F - 1, 1, F - 2, F // 2]
        for t in range(T):
            X[1, 0, bins[t % len(bins)], t] = np.complex64(rng.standard_normal() + 1j * rng.standard_normal())
    if nan_tail:
        X[..., T:] = np.nan
    return X


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- (a) / (b) the DFT GEMM -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [16, 128, 1536])
@pytest.mark.parametrize("N", [128, 640, 1536])
def test_gemm_exact(N, K):
    gen = torch.Generator(device="cuda").manual_seed(N * 7 + K)
    seen = set()
    for M in (1, 31, 127, 128, 129, 5376, 5377, 8032):
        A = torch.randint(-8, 9, (M, K), device="cuda", generator=gen).float()
        Bm = torch.randint(-8, 9, (K, N), device="cuda", generator=gen).float() / 4
        bn = ops().stft_gemm_variant(M, N, K)
        assert bn == gemm_bn(M, N, K)
        seen.add(bn)
        got = ops().stft_gemm(A, Bm)
        want = (A.double() @ Bm.double())
        assert float(want.abs().max()) < 2 ** 22 / 4
        bad = (got.double() != want).nonzero()
        assert bad.numel() == 0, f"M {M} N {N} K {K} (BN {bn}): {bad.shape[0]} of {M * N} outputs differ, first {bad[0].tolist()}"
    assert seen == ({32, 128} if N == 1536 else {32})


@pytest.mark.parametrize("N,K,M0", [(1536, 1536, 5376), (640, 640, 13056)])
def test_gemm_tile_width_does_not_change_bits(N, K, M0):
    """sgemm_mfma_kernel sums every output in the same k order at both tile widths: random inexact data, equal bits."""
    assert (ops().stft_gemm_variant(M0, N, K), ops().stft_gemm_variant(M0 + 1, N, K)) == (32, 128)
    gen = torch.Generator(device="cuda").manual_seed(M0)
    A = torch.randn(M0 + 1, K, device="cuda", generator=gen)
    Bm = torch.randn(K, N, device="cuda", generator=gen)
    wide, narrow = ops().stft_gemm(A, Bm), ops().stft_gemm(A[:M0], Bm)
    assert torch.equal(wide[:M0], narrow)
    # and the result is the product: inexact data within the worst-case bound
    err = (wide.double() - A.double() @ Bm.double()).abs()
    assert bool((err <= C_BOUND * K * U * (A.double().abs() @ Bm.double().abs())).all())


def test_gemm_refusal_leaves_output_untouched():
    A = torch.ones(64, 1536, device="cuda")
    Bm = torch.ones(1536, 1536, device="cuda")
    Cm = torch.full((64, 1536), 7.0, device="cuda")
    rc = lib().fd_stft_gemm_f32(C.c_void_p(A.data_ptr() + 4), C.c_void_p(Bm.data_ptr()), C.c_void_p(Cm.data_ptr()), 63, 1536, 1536, None)
    assert rc == -1 and b"aligned" in lib().fd_last_error()
    rc = lib().fd_stft_gemm_f32(C.c_void_p(A.data_ptr()), C.c_void_p(Bm.data_ptr()), C.c_void_p(Cm.data_ptr()), 64, 1536, 1528, None)
    assert rc == -1 and b"unsupported shape" in lib().fd_last_error()
    torch.cuda.synchronize()
    assert bool((Cm == 7.0).all())


# ---- (c) the forward spectrum -----------------------------------------------------------------------------------------------------------
FORWARD_CASES = [  # (n_fft, hop, B, L): BN = 128 / 32 at production size, the shortest clip, L mod hop = 0 with T = T_pad, other geometries
    (1534, 384, 32, 96000), (1534, 384, 8, 96000), (1534, 384, 1, 768), (1534, 384, 3, 48768), (1534, 384, 2, 50001),
    (510, 128, 16, 130048), (510, 128, 8, 130048), (512, 128, 16, 104448), (512, 128, 8, 104448), (64, 16, 32, 32768), (64, 16, 8, 32768),
]


@pytest.mark.parametrize("n_fft,hop,B,L", FORWARD_CASES)
def test_forward_spectrum_float64(n_fft, hop, B, L):
    y = signals(B, L, n_fft, hop, seed=L + B)
    T = 1 + L // hop
    bn = ops().stft_gemm_variant(B * T, kpad(n_fft), kpad(n_fft))
    Y, nf, T_k = ops().stft_compress(dev(y), n_fft=n_fft, hop=hop, alpha=1.0, beta=1.0, normalize=False)
    assert T_k == T and Y.shape == (B, 1, n_fft // 2 + 1, padded(T))
    assert bool((nf == 1).all())
    Yh = Y.cpu().numpy()[:, 0]
    worst, rels = 0.0, []
    for b in range(B):
        rel, ratio = check_forward(f"stft n_fft {n_fft} hop {hop} B {B} L {L} row {b}", Yh[b], y[b], n_fft, hop)
        worst = max(worst, ratio)
        if b not in (1, 2):
            rels.append(rel)
    report(f"stft_fwd n_fft={n_fft} hop={hop} B={B} L={L} BN={bn}: noise rel_l2 max={max(rels):.3e}  max err/bound={worst:.3e}")


# ---- (d) normalisation ------------------------------------------------------------------------------------------------------------------
def test_normfac_bits_and_normalised_spectrum():
    L = 50001                                             # not a multiple of 1024 (the block's stride)
    rng = np.random.default_rng(5)
    y = (0.1 * rng.standard_normal((4, L))).astype(np.float32)
    y[0, 0], y[1, L - 1], y[2, L - 1], y[3, 1023] = 3.0, -4.0, 2.5, -1.75
    Y, nf, T = ops().stft_compress(dev(y), alpha=1.0, beta=1.0, normalize=True)
    nf = nf.cpu().numpy()
    assert np.array_equal(nf, np.abs(y).max(axis=1)) and list(nf) == [3.0, 4.0, 2.5, 1.75]
    Yh = Y.cpu().numpy()[:, 0]
    for b in range(4):
        check_forward(f"normalised row {b}", Yh[b], y[b] / nf[b], NFFT, HOP)   # float32 y / normfac, exactly as the framing kernel divides


def test_normfac_silence_rule_matches_torch_isclose():
    tiny = np.float32(1e-8)
    vals = [np.nextafter(tiny, np.float32(0)), tiny, np.nextafter(tiny, np.float32(1)), np.float32(2e-8), np.float32(5e-9), np.float32(0)]
    y = np.zeros((2 * len(vals), 4000), np.float32)
    for i, v in enumerate(vals):
        y[2 * i, 1234] = v
        y[2 * i + 1, 3999] = -v
    _, nf, _ = ops().stft_compress(dev(y), alpha=1.0, beta=1.0, normalize=True)
    m = torch.from_numpy(np.abs(y).max(axis=1))
    want = torch.where(torch.isclose(m, torch.zeros_like(m)), torch.ones_like(m), m)
    assert torch.equal(nf.cpu(), want), (nf.cpu(), want)
    assert nf[0] == 1 and nf[2] == 1 and nf[4] == vals[2]          # the rule's edge: at 1e-8 still silent, one ulp above not


def test_normfac_ragged_ignores_the_tail():
    lengths = [24576, 30000, 41234, 49151]
    Lrow = max(lengths)
    rng = np.random.default_rng(6)
    y = (0.1 * rng.standard_normal((4, Lrow))).astype(np.float32)
    y[0, lengths[0]:] = 1e3
    y[1, lengths[1]:] = np.nan
    y[2, lengths[2]] = 1e3
    y[2, lengths[2] - 1] = 0.75
    Y, nf, T = ops().stft_compress(dev(y), alpha=1.0, beta=1.0, normalize=True, lengths=lengths)
    want = np.array([np.abs(y[b, :l]).max() for b, l in enumerate(lengths)], np.float32)
    assert np.array_equal(nf.cpu().numpy(), want) and nf[2] == 0.75
    Yh = Y.cpu().numpy()[:, 0]
    for b, l in enumerate(lengths):
        check_forward(f"ragged normalised row {b}", Yh[b], y[b, :l] / want[b], NFFT, HOP, T_own=1 + l // HOP)


# ---- (e) compression --------------------------------------------------------------------------------------------------------------------
def compress_spec(X, alpha, beta, inverse):
    X = X.contiguous()
    out = torch.empty_like(X)
    rc = lib().fd_compress_spec(C.c_void_p(X.data_ptr()), C.c_void_p(out.data_ptr()), X.numel(), alpha, beta, int(inverse), None)
    assert rc == 0
    torch.cuda.synchronize()
    return out


ALPHA, BETA = 0.3, 0.33


def test_fused_and_standalone_compression_same_bits():
    rng = np.random.default_rng(7)
    y = (0.1 * rng.standard_normal((3, 48000))).astype(np.float32)
    y[1] = impulse_ends(48000)
    for normalize in (False, True):
        Y1, nf1, T = ops().stft_compress(dev(y), alpha=1.0, beta=1.0, normalize=normalize)
        Yab, nf, _ = ops().stft_compress(dev(y), alpha=ALPHA, beta=BETA, normalize=normalize)
        assert torch.equal(nf, nf1)
        assert torch.equal(torch.view_as_real(Yab), torch.view_as_real(compress_spec(Y1, ALPHA, BETA, False)))
    X = dev(random_spectra(3, 768, 128, 126, seed=8, nan_tail=False))
    L = HOP * 125
    a = ops().decompress_istft(X, 126, L, None, alpha=ALPHA, beta=BETA)
    b = ops().decompress_istft(compress_spec(X, ALPHA, BETA, True), 126, L, None, alpha=1.0, beta=1.0)
    assert torch.equal(a, b)


def compression_inputs(seed):
    rng = np.random.default_rng(seed)
    n = 1 << 16
    mag = 10.0 ** rng.uniform(-10, 10, n)
    x = (mag * np.exp(1j * rng.uniform(-np.pi, np.pi, n))).astype(np.complex64)
    specials = np.array([0, -1.5, -2e-9, -3e9, 1j, -1j, 2.5, -0.0 + 0j, complex(-7.0, -0.0), complex(4e-10, 0), complex(0, 9e9)], np.complex64)
    return np.concatenate([specials, x])


def ulps_of(got, ref):
    return np.abs(got.astype(np.complex128) - ref) / (U * np.maximum(np.abs(ref), 1e-300))


# fd_compress_spec against float64 with the float32 alpha / beta the call receives: |got - ref| <= (ULP_BOUND + extra) u |ref| per
# element.  The forward has no extra term.  The inverse raises z = x / beta to 1 / alpha, and the kernel rounds that exponent to float32
# (<= u / alpha absolute), which moves the result by up to |ln |z|| u / alpha relative: extra = |ln |z|| / alpha (80 u at |z| = 3e10,
# the largest tested; 0 at |z| = 1).  ULP_BOUND is twice the measured worst case beyond that (parity report), rounded up.
ULP_BOUND = 20


def test_compress_spec_float64():
    x = compression_inputs(9)
    xd = dev(x)
    a32, b32 = float(np.float32(ALPHA)), float(np.float32(BETA))
    for inverse in (False, True):
        got = compress_spec(xd, ALPHA, BETA, inverse).cpu().numpy()
        x64 = x.astype(np.complex128)
        if inverse:
            z = x64 / b32
            ref = np.abs(z) ** (1 / a32) * np.exp(1j * np.angle(z))
            extra = np.abs(np.log(np.maximum(np.abs(z), 1e-300))) / a32
        else:
            ref = b32 * np.abs(x64) ** a32 * np.exp(1j * np.angle(x64))
            extra = np.zeros(len(x))
        zero = x == 0
        assert not got[zero].real.any() and not got[zero].imag.any(), "exact zeros must stay zero"
        r = ulps_of(got[~zero], ref[~zero])
        beyond = r - extra[~zero]
        report(f"compress_spec {'inverse' if inverse else 'forward'} alpha={ALPHA} beta={BETA}: max err = {r.max():.2f} u |ref|, "
               f"{beyond.max():.2f} u |ref| beyond the exponent term")
        worst = int(np.argmax(beyond))
        assert beyond.max() <= ULP_BOUND, (inverse, x[~zero][worst], got[~zero][worst], ref[~zero][worst])
        # the negative real axis keeps its sign and lands within the bound (atan2 = +-pi)
        neg = (x.real < 0) & (x.imag == 0)
        assert neg.sum() >= 4 and (got[neg].real < 0).all()


# ---- (f) the inverse --------------------------------------------------------------------------------------------------------------------
INVERSE_CASES = [  # (n_fft, hop, B, T, L)
    (1534, 384, 32, 251, 96000), (1534, 384, 8, 251, 96000), (1534, 384, 2, 9, 3838), (1534, 384, 2, 9, 3000), (1534, 384, 3, 128, 48768),
    (1534, 384, 2, 251, 96000 + 766), (510, 128, 16, 1017, 130048), (64, 16, 32, 2049, 32768), (64, 16, 8, 2049, 32768),
]


@pytest.mark.parametrize("n_fft,hop,B,T,L", INVERSE_CASES)
def test_inverse_float64(n_fft, hop, B, T, L):
    F = n_fft // 2 + 1
    assert ops().istft_envelope_ok(n_fft, hop, T, L)
    X = random_spectra(B, F, padded(T), T, seed=T + B)
    bn = ops().stft_gemm_variant(B * T, kpad(n_fft), kpad(n_fft))
    y = ops().decompress_istft(dev(X), T, L, None, n_fft=n_fft, hop=hop, alpha=1.0, beta=1.0).cpu().numpy()
    worst, rels = 0.0, []
    for b in range(B):
        rel, ratio = check_inverse(f"istft n_fft {n_fft} B {B} T {T} L {L} row {b}", y[b], X[b, 0, :, :T], n_fft, hop, L)
        worst = max(worst, ratio)
        if b != 1:
            rels.append(rel)
    report(f"istft n_fft={n_fft} hop={hop} B={B} T={T} L={L} BN={bn}: random rel_l2 max={max(rels):.3e}  max err/bound={worst:.3e}")


def test_inverse_refuses_zero_envelope_lengths():
    """At and past n_fft/2 + hop (T - 1) the last kept sample is covered only by w[n_fft - 1] = 0: torch.istft raises, and so does the
    kernel's host side -- before any launch, the output is untouched.  This includes every length reaching into the zero tail."""
    from flowdec_amd import _lib as L_
    plan = ops().stft_plan(NFFT, HOP, "cuda")
    X = dev(random_spectra(2, 768, 256, 9, seed=1))
    for T, L in ((9, 3839), (9, 3840), (9, 5000), (251, 96000 + 767), (13, 4800 + 767)):
        assert not ops().istft_envelope_ok(NFFT, HOP, T, L)
        nws = lib().fd_stft_workspace_bytes(2, max(L, HOP * T), NFFT, HOP)
        ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
        y = torch.full((2, L), 7.0, device="cuda")
        rc = lib().fd_decompress_istft(plan, L_.ptr(X), 2, T, 256, 1.0, 1.0, None, L_.ptr(y), L, L_.ptr(ws), nws, None)
        assert rc == -1 and b"zero window envelope" in lib().fd_last_error(), (T, L, rc)
        with pytest.raises(RuntimeError, match="zero window envelope"):
            ops().decompress_istft(X, T, L, None, alpha=1.0, beta=1.0)
        torch.cuda.synchronize()
        assert bool((y == 7.0).all())
    # the ragged form cannot see its lengths: hop > n_fft / 2 is refused as a geometry
    lengths = [3100, 3200]                 # one T_pad = 128 bucket at hop 48
    with pytest.raises(RuntimeError, match="hop 48 > n_fft / 2"):
        ops().decompress_istft(dev(random_spectra(2, 33, 128, 67, seed=2)), 67, 3200, None, n_fft=64, hop=48, alpha=1.0, beta=1.0, lengths=lengths)


def test_enhance_geometry_never_meets_a_zero_envelope():
    """enhance's own T = 1 + L / hop with hop <= n_fft / 2: L mod hop < n_fft / 2, so every length is taken."""
    for n_fft, hop in ((1534, 384), (1534, 767), (510, 128), (64, 16), (64, 32)):
        for L in list(range(n_fft // 2 + 1, n_fft // 2 + 3 * hop)) + [96000, 96000 + hop - 1]:
            assert ops().istft_envelope_ok(n_fft, hop, 1 + L // hop, L), (n_fft, hop, L)


# ---- (g) a ragged batch at the wide tile width ------------------------------------------------------------------------------------------
def test_ragged_batch_float64():
    rng = np.random.default_rng(11)
    lengths = [73728, 98303] + sorted(int(v) for v in rng.integers(73728, 98304, 30))     # one T_pad = 256 bucket
    B, Lrow = len(lengths), max(lengths)
    T = 1 + Lrow // HOP
    assert ops().stft_gemm_variant(B * T, 1536, 1536) == 128
    y = np.full((B, Lrow), np.nan, np.float32)                 # any read behind a clip's end poisons that clip
    for b, l in enumerate(lengths):
        y[b, :l] = signals(3, l, NFFT, HOP, seed=b)[b % 3]
    Y, nf, T_k = ops().stft_compress(dev(y), alpha=1.0, beta=1.0, normalize=True, lengths=lengths)
    assert T_k == T and Y.shape[-1] == 256
    Yh, nfh = Y.cpu().numpy()[:, 0], nf.cpu().numpy()
    worst = 0.0
    for b, l in enumerate(lengths):
        assert nfh[b] == np.abs(y[b, :l]).max()
        rel, ratio = check_forward(f"ragged clip {b} ({l})", Yh[b], y[b, :l] / nfh[b], NFFT, HOP, T_own=1 + l // HOP)
        worst = max(worst, ratio)
    report(f"stft_fwd ragged B={B} lengths {min(lengths)}..{max(lengths)} BN=128: max err/bound={worst:.3e}")
    # the inverse: random spectra, NaN in every frame behind a clip's own T
    X = random_spectra(B, 768, 256, T, seed=12)
    for b, l in enumerate(lengths):
        X[b, ..., 1 + l // HOP:] = np.nan
    out = ops().decompress_istft(dev(X), T, Lrow, None, alpha=1.0, beta=1.0, lengths=lengths).cpu().numpy()
    worst, rels = 0.0, []
    for b, l in enumerate(lengths):
        rel, ratio = check_inverse(f"ragged istft clip {b} ({l})", out[b], X[b, 0, :, :1 + l // HOP], NFFT, HOP, l)
        worst = max(worst, ratio)
        if b != 1:
            rels.append(rel)
    report(f"istft ragged B={B} BN=128: random rel_l2 max={max(rels):.3e}  max err/bound={worst:.3e}")
