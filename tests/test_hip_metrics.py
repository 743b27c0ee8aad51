"""csrc/metrics.hip -- SI-SDR / SI-SIR / SI-SAR and the log-spectral MSE over ragged batches (include/flowdec_hip.h "Evaluation metrics";
flowdec_amd/metrics.py si_sxr_batch / logspec_mse_batch; flowdec_amd/eval_cli.py) -- against float64 references.

(a) The eight float64 sums of fd_metrics_sisxr against math.fsum over float64 terms, at lengths that cover the wave tail, the slice tail, a
    clip with fewer samples than slices and one with many samples per slice; on small-integer data every sum is exact in any order, so the
    values must be EQUAL.
(b) The nine values of golden g14_metrics.npz (reference code on seeded signals) within 1e-4 dB.
(c) fd_metrics_power_spec per bin against float64 rfft of the reflect-padded, windowed frames: the per-bin bound of test_hip_stft.py (c)
    propagated to re^2 + im^2.
(d) The log-spectral MSE: the interval that the per-bin bounds of (c) leave for the mean must contain the kernel's value.
(e) A clip's sums and its MSE have the same bits alone, in a ragged batch in either order, and in a batch of 32, with NaN behind every
    clip's end.
(f) Refusals: FD_EINVAL with a message, nothing launched.
(g) eval_cli end to end, and enhance_cli --eval.

The bound of (a).  One sum has n terms t_i.  Pass 1 (x.x, x_hat.x, x_hat.n, n.n): the samples are float32, so x_i x_i and x_hat_i x_i are
exact in float64; n_i = y_i -+ x_i is ONE float64 rounding, the same bits in the kernel and in NumPy, so it counts as data.  The kernel
adds the terms in some tree with at most n - 1 inexact additions (adding a zero is exact): at most (n - 1) u sum|t_i|, u = 2^-53, plus
u sum|t_i| if the compiler does not fuse the product into the addition.  The reference's float64 products carry u |t_i| each and fsum one
last rounding: (n + 2) u sum|t_i| in all, below C1 n u sum|t_i| with C1 = 4 (second-order terms: n u <= 1.2e-11).
Pass 2 (|s_target|^2, |e_noise|^2, |e_art|^2, |e_noise + e_art|^2) is compared with alpha_s = [1] / [0] and alpha_n = [2] / [3] formed in
float64 from the KERNEL's pass-1 sums, as the kernel forms them (an IEEE division: the same bits; should a device division ever differ in
the last place, e_art moves by at most 2 u M_i, with M_i below).  With M_i = |x_hat_i| + |alpha_s x_i| + |alpha_n n_i|:
s_target_i and e_noise_i carry one rounding each (<= u M_i), e_art_i = x_hat_i - s_target_i - e_noise_i those two and two subtractions
(<= 4 u M_i), e_noise_i + e_art_i one more (<= 6 u M_i); every one of the four values v is at most M_i in size, so its square is off by at
most 2 M_i 6 u M_i + u M_i^2 = 13 u M_i^2 -- in the kernel (less where it fuses) and in the NumPy reference alike: 26 u sum M_i^2, plus
4 u sum M_i^2 for the division's last place, plus the summation (n - 1) u sum|t_i| <= (n - 1) u sum M_i^2 and fsum's rounding:
(n + 30) u sum M_i^2 <= C2 n u sum M_i^2 with C2 = 32.

Measured errors and error / bound ratios go into the parity report; only the bounds are asserted."""
import csv
import ctypes as C
import math

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_hip_stft import C_BOUND, U, dev, impulse_borders, impulse_ends, kpad, report, stft_ref

pytestmark = pytest.mark.gpu

U64 = 2.0 ** -53
C1, C2 = 4.0, 32.0
NFFT, HOP, NFREQ, EPS = 1536, 384, 769, 1e-8
FD_EINVAL = -1


def L_():
    from flowdec_amd import _lib
    return _lib


def lib():
    return L_().load()


def plan():
    from flowdec_amd import ops
    return ops.stft_plan(NFFT, HOP, "cuda")


def rows_of(clips, Lrow=None, fill=np.nan):
    """[B, Lrow] float32 rows, `fill` (NaN: any read behind a clip's end poisons its result) behind every clip."""
    Lrow = Lrow or max(len(c) for c in clips)
    r = np.full((len(clips), Lrow), fill, np.float32)
    for b, c in enumerate(clips):
        r[b, :len(c)] = c
    return r


def call_sisxr(hs, xs, ys, Lrow=None):
    """lists of float32 clips -> [B, 8] float64 sums of one ragged call."""
    l = L_()
    h, x, y = (dev(rows_of(v, Lrow)) for v in (hs, xs, ys))
    lens = torch.tensor([len(c) for c in xs], dtype=torch.int32, device="cuda")
    B, Lr = x.shape
    nws = lib().fd_metrics_workspace_bytes(B, Lr, 0, 0)
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    out = torch.full((B, 8), 7.0, dtype=torch.float64, device="cuda")
    l.check(lib().fd_metrics_sisxr(l.ptr(h), l.ptr(x), l.ptr(y), l.ptr(lens), B, Lr, l.ptr(out), l.ptr(ws), nws, l.stream()))
    return out.cpu().numpy()


def call_logspec(hs, xs, Lrow=None):
    l = L_()
    h, x = (dev(rows_of(v, Lrow)) for v in (hs, xs))
    lens = torch.tensor([len(c) for c in xs], dtype=torch.int32, device="cuda")
    B, Lr = x.shape
    nws = lib().fd_metrics_workspace_bytes(B, Lr, NFFT, HOP)
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    out = torch.full((B,), 7.0, dtype=torch.float64, device="cuda")
    l.check(lib().fd_metrics_logspec_mse(plan(), l.ptr(h), l.ptr(x), l.ptr(lens), B, Lr, EPS, l.ptr(out), l.ptr(ws), nws, l.stream()))
    return out.cpu().numpy()


def call_power(xs, Lrow=None):
    l = L_()
    x = dev(rows_of(xs, Lrow))
    lens = torch.tensor([len(c) for c in xs], dtype=torch.int32, device="cuda")
    B, Lr = x.shape
    T = 1 + Lr // HOP
    nws = lib().fd_metrics_workspace_bytes(B, Lr, NFFT, HOP)
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    P = torch.full((B, T, NFREQ), 7.0, dtype=torch.float32, device="cuda")
    l.check(lib().fd_metrics_power_spec(plan(), l.ptr(x), l.ptr(lens), B, Lr, l.ptr(P), l.ptr(ws), nws, l.stream()))
    return P.cpu().numpy()


# ---- (a) SI-SxR sums --------------------------------------------------------------------------------------------------------------------
SUM_LENGTHS = [1, 3, 63, 64, 65, 511, 513, 4000, 100003]


def random_triple(n, seed, flip=False):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n).astype(np.float32)
    y = ((-x if flip else x) + 0.3 * rng.standard_normal(n)).astype(np.float32)
    h = (x + 0.1 * rng.standard_normal(n) + 0.05 * (y - x)).astype(np.float32)
    return h, x, y


def sums_reference(h, x, y, got):
    """-> (ref [8] by math.fsum over float64 terms, bound [8]); pass 2 with the alphas of the kernel's own pass-1 sums `got`."""
    h, x, y = (a.astype(np.float64) for a in (h, x, y))
    n = len(x)
    nv = y + x if math.fsum(x * y) < 0 else y - x
    t1 = [x * x, h * x, h * nv, nv * nv]
    a_s, a_n = got[1] / got[0], got[2] / got[3]
    st, en = a_s * x, a_n * nv
    ea = h - st - en
    t2 = [st * st, en * en, ea * ea, (en + ea) * (en + ea)]
    M2 = math.fsum((np.abs(h) + np.abs(st) + np.abs(en)) ** 2)
    ref = np.array([math.fsum(t) for t in t1 + t2])
    bound = np.array([C1 * n * U64 * math.fsum(np.abs(t)) for t in t1] + [C2 * n * U64 * M2] * 4)
    return ref, bound


def test_sisxr_sums_against_fsum():
    trip = [random_triple(n, seed=n, flip=(i % 3 == 1)) for i, n in enumerate(SUM_LENGTHS)]
    got = call_sisxr(*zip(*trip))
    worst1 = worst2 = 0.0
    flips = 0
    for b, (h, x, y) in enumerate(trip):
        assert np.isfinite(got[b]).all(), (SUM_LENGTHS[b], got[b])
        ref, bound = sums_reference(h, x, y, got[b])
        flips += math.fsum(x.astype(np.float64) * y.astype(np.float64)) < 0
        err = np.abs(got[b] - ref)
        ratio = err / np.maximum(bound, 1e-300)
        print(f"sisxr sums n={len(x)}: err/bound = {np.array2string(ratio, precision=3)}")
        worst1, worst2 = max(worst1, ratio[:4].max()), max(worst2, ratio[4:].max())
        assert (err <= bound).all(), (len(x), err, bound)
    assert 2 <= flips < len(trip)          # both signs of n ran
    report(f"metrics sisxr sums lengths {SUM_LENGTHS}: max err/bound pass 1 = {worst1:.3e} (C1 = {C1:g}), pass 2 = {worst2:.3e} (C2 = {C2:g})")


def integer_triple(n, seed, flip):
    """x, n and a residual e on the three residue classes mod 3 (mutually orthogonal), x_hat = 2 x + n / 2 + e: alpha_s = 2 and alpha_n = 1 / 2
    exactly, every term a multiple of 1 / 4 and every partial sum far below 2^53 -- exact in any order."""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    v = rng.integers(1, 9, n) * rng.choice((-1, 1), n)
    x, nz, e = (np.where(i % 3 == k, v, 0).astype(np.float64) for k in (0, 1, 2))
    y = (-x if flip else x) + nz
    return (2 * x + 0.5 * nz + e).astype(np.float32), x.astype(np.float32), y.astype(np.float32)


def test_sisxr_sums_exact_on_integer_data():
    trip = [integer_triple(n, seed=100 + n, flip=(i % 2 == 1)) for i, n in enumerate(SUM_LENGTHS)]
    got = call_sisxr(*zip(*trip))
    for b, (h, x, y) in enumerate(trip):
        h, x, y = (a.astype(np.float64) for a in (h, x, y))
        nv = y + x if np.dot(x, y) < 0 else y - x
        with np.errstate(invalid="ignore", divide="ignore"):
            a_s, a_n = np.dot(h, x) / np.dot(x, x), np.dot(h, nv) / np.dot(nv, nv)        # 2 and 1/2; 0/0 where a clip of 1 sample has no n
            st, en = a_s * x, a_n * nv
            ea = h - st - en
            want = np.array([np.dot(x, x), np.dot(h, x), np.dot(h, nv), np.dot(nv, nv), np.dot(st, st), np.dot(en, en), np.dot(ea, ea),
                             np.dot(en + ea, en + ea)])
        if len(x) >= 3:
            assert (a_s, a_n) == (2.0, 0.5) and np.isfinite(want).all()
        assert np.array_equal(got[b], want, equal_nan=True), (len(x), got[b], want)


# ---- (b) the golden ---------------------------------------------------------------------------------------------------------------------
def test_sisxr_golden():
    from flowdec_amd import metrics
    g = load_golden("g14_metrics.npz")
    got = metrics.si_sxr_batch([g[f"xhat{i}"] for i in range(3)], [g[f"x{i}"] for i in range(3)], [g[f"y{i}"] for i in range(3)])
    want = np.stack([g[f"sisxr{i}"] for i in range(3)])
    assert got.shape == (3, 3) and got.dtype == np.float64
    err = np.abs(got - want)
    report(f"metrics sisxr golden g14: max |dB - reference| = {err.max():.3e} (atol 1e-4, ratio {err.max() / 1e-4:.3e})")
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-4)
    assert sum(float(np.dot(g[f"x{i}"].astype(np.float64), g[f"y{i}"].astype(np.float64))) < 0 for i in range(3)) >= 1      # the flipped case is in


# ---- (c) / (d) the spectral metric ------------------------------------------------------------------------------------------------------
SPEC_LENGTHS = [769, 1536, 1921, 4000, 20011]        # 769: the shortest legal clip (T = 3)
_power_cache = {}


def power_reference(x32):
    """float32 clip -> (P [T, F] float64 = |X|^2 of the float64 transform, bound [T, F] on the kernel's float32 re^2 + im^2).
    Each of re, im is within e_t = C_BOUND K u S_t of float64 (test_hip_stft.py (c)): re^2 + im^2 moves by at most
    dP = e (2 |re| + e) + e (2 |im| + e); the float32 squares and their sum add at most 3 u (P + dP)."""
    key = x32.tobytes()
    if key not in _power_cache:
        X, S = stft_ref(x32.astype(np.float64), NFFT, HOP)
        X, e = X.T, (C_BOUND * kpad(NFFT) * U * S)[:, None]
        P = X.real ** 2 + X.imag ** 2
        dP = e * (2 * np.abs(X.real) + e) + e * (2 * np.abs(X.imag) + e)
        _power_cache[key] = (P, dP + 3 * U * (P + dP))
    return _power_cache[key]


def spectral_signals(L):
    rng = np.random.default_rng(L)
    return [(0.1 * rng.standard_normal(L)).astype(np.float32), impulse_ends(L), impulse_borders(L, NFFT, HOP, L)]


def test_power_spec_float64():
    clips = [s for L in SPEC_LENGTHS for s in spectral_signals(L)]
    P = call_power(clips)
    assert P.shape == (len(clips), 1 + max(SPEC_LENGTHS) // HOP, NFREQ)
    worst = 0.0
    for b, c in enumerate(clips):
        ref, bound = power_reference(c)
        T = ref.shape[0]
        assert T == 1 + len(c) // HOP
        err = np.abs(P[b, :T].astype(np.float64) - ref)
        bad = np.argwhere(~(err <= bound))
        assert bad.size == 0, f"clip {b} ({len(c)} samples): {len(bad)} bins over the bound, first (t, f) = {bad[0].tolist()}: err {err[tuple(bad[0])]:.3e} bound {bound[tuple(bad[0])]:.3e}"
        assert not P[b, T:].any(), f"clip {b}: frames behind T = {T} must be zero"
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    report(f"metrics power_spec n_fft={NFFT} hop={HOP} lengths {SPEC_LENGTHS} x (noise, end impulses, border impulses): max err/bound={worst:.3e}")


# float64 arithmetic of the epilogue: a device log10 within a few ulps of a level below 200 dB, and the summation roundings -- orders of
# magnitude below the float32 terms above; added to every level and to the mean so that the interval is a strict one
LEVEL_SLACK, MEAN_SLACK = 1e-12, 1e-12


def level_interval(x32, scale=1.0):
    P, bound = power_reference(x32)
    lo, hi = np.maximum(P - bound, 0.0), P + bound
    return (10 * np.log10(np.maximum(lo, EPS)) - LEVEL_SLACK, 10 * np.log10(np.maximum(hi, EPS)) + LEVEL_SLACK, 10 * np.log10(np.maximum(P, EPS)))


def mse_interval(h32, x32):
    """-> (lo, hi, float64 value): every bin's power interval clamped, logged and differenced; the squared difference's interval; the mean's."""
    alo, ahi, a = level_interval(h32)
    blo, bhi, b = level_interval(x32)
    dlo, dhi = alo - bhi, ahi - blo
    sq_hi = np.maximum(dlo ** 2, dhi ** 2)
    sq_lo = np.where((dlo <= 0) & (dhi >= 0), 0.0, np.minimum(dlo ** 2, dhi ** 2))
    return float(sq_lo.mean()) * (1 - MEAN_SLACK), float(sq_hi.mean()) * (1 + MEAN_SLACK), float(((a - b) ** 2).mean())


def logspec_pairs(L):
    """(x_hat, x): broadband noise at 0.1 against a perturbed copy; a 440 Hz tone on a 1e-3 white floor against a detuned copy.  The tone's
    amplitude is 0.01: the worst-case bound of a bin grows with the frame's sum |x_k| w_k, and at this amplitude it stays a twentieth of the
    floor's typical bin while the tone stands 40 dB above the floor."""
    rng = np.random.default_rng(7 * L)
    x = (0.1 * rng.standard_normal(L)).astype(np.float32)
    h = (x + 0.01 * rng.standard_normal(L)).astype(np.float32)
    t = np.arange(L) / 48000.0
    floor = 1e-3 * rng.standard_normal(L)
    tone = (0.01 * np.sin(2 * np.pi * 440.0 * t) + floor).astype(np.float32)
    detuned = (0.01 * np.sin(2 * np.pi * 446.0 * t) + floor + 1e-4 * rng.standard_normal(L)).astype(np.float32)
    return [(h, x), (detuned, tone)]


def test_logspec_mse_float64():
    """The interval of (d) is a worst case over every bin (a noise bin near zero leaves a wide level interval), so it is wide; the second
    assertion closes what it leaves open: given the kernel's OWN float32 powers (fd_metrics_power_spec, held per bin by (c)), the epilogue
    is float64 arithmetic only.  A level is below 80 dB in size (1e-8 <= P < 1e8) and a float64 log10 within 4 ulps of it: 7e-14; a
    difference d within 2e-13, its square within 4e-13 |d|; the mean's own roundings stay below 1e-11 of it (4e4 terms of 2^-53)."""
    pairs = [p for L in SPEC_LENGTHS for p in logspec_pairs(L)]
    got = call_logspec([p[0] for p in pairs], [p[1] for p in pairs])
    Ph, Px = call_power([p[0] for p in pairs]).astype(np.float64), call_power([p[1] for p in pairs]).astype(np.float64)
    worst_rel = worst_pos = widest = worst_own = 0.0
    for b, (h, x) in enumerate(pairs):
        T = 1 + len(x) // HOP
        d = 10 * np.log10(np.maximum(Ph[b, :T], EPS)) - 10 * np.log10(np.maximum(Px[b, :T], EPS))
        own, tol = float((d ** 2).mean()), 4e-13 * float(np.abs(d).max()) + 1e-11 * float((d ** 2).mean())
        assert abs(got[b] - own) <= tol, (len(x), b % 2, got[b], own, tol)
        worst_own = max(worst_own, abs(got[b] - own) / tol)
        lo, hi, ref = mse_interval(h, x)
        rel, pos = abs(got[b] - ref) / ref, abs(got[b] - ref) / max(hi - ref, ref - lo)
        print(f"logspec_mse L={len(x)} pair {b % 2}: got {got[b]:.9g} float64 {ref:.9g} interval [{lo:.9g}, {hi:.9g}] rel err {rel:.3e}")
        assert lo <= got[b] <= hi, (len(x), b % 2, got[b], lo, hi)
        worst_rel, worst_pos, widest = max(worst_rel, rel), max(worst_pos, pos), max(widest, (hi - lo) / ref)
    report(f"metrics logspec_mse lengths {SPEC_LENGTHS} x (noise, tone): max |got - float64| / float64 = {worst_rel:.3e}, max error / interval "
           f"half-width = {worst_pos:.3e} (widest interval: {widest:.3e} of the value); against float64 on the kernel's own powers: "
           f"max error / tolerance = {worst_own:.3e}")


def test_logspec_mse_identities():
    rng = np.random.default_rng(5)
    xs = [(0.1 * rng.standard_normal(L)).astype(np.float32) for L in SPEC_LENGTHS]
    same = call_logspec(xs, xs)
    assert (same == 0.0).all() and not np.signbit(same).any(), same
    twice = call_logspec([2 * x for x in xs], xs)
    want = (20 * math.log10(2.0)) ** 2
    for b, x in enumerate(xs):
        lo, hi, ref = mse_interval(2 * x, x)
        assert lo <= twice[b] <= hi and lo <= want <= hi, (len(x), twice[b], want, lo, hi)
    report(f"metrics logspec_mse(2x, x): max |got - (20 log10 2)^2| / it = {np.abs(twice - want).max() / want:.3e}")


# ---- (e) batch invariance ---------------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_batch_invariance_bit_for_bit():
    lengths = [4000, 769, 20011]
    trip = [random_triple(n, seed=9 + n) for n in lengths]
    hs, xs, ys = (list(v) for v in zip(*trip))
    alone_s = [call_sisxr([h], [x], [y])[0] for h, x, y in trip]
    alone_m = [call_logspec([h], [x])[0] for h, x, _ in trip]
    assert all(np.isfinite(s).all() for s in alone_s) and np.isfinite(alone_m).all() and min(alone_m) > 0

    def check(order, Lrow=None):
        s = call_sisxr([hs[i] for i in order], [xs[i] for i in order], [ys[i] for i in order], Lrow)
        m = call_logspec([hs[i] for i in order], [xs[i] for i in order], Lrow)
        for r, i in enumerate(order):
            assert np.array_equal(bits(s[r]), bits(alone_s[i])), f"clip of {lengths[i]} samples at row {r} of {len(order)}: sums differ from its one-clip call"
            assert bits(m[r]) == bits(alone_m[i]), f"clip of {lengths[i]} samples at row {r} of {len(order)}: MSE differs from its one-clip call"

    check([0, 1, 2])
    check([2, 1, 0])
    check([0, 1, 2], Lrow=25000)                  # a longer row: L must not matter either
    check([(5 * r + r // 7) % 3 for r in range(32)])


# ---- (f) refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    l = L_()
    B, Lr = 2, 4000
    x = torch.zeros(B, Lr, device="cuda")
    lens = torch.full((B,), Lr, dtype=torch.int32, device="cuda")
    nws = lib().fd_metrics_workspace_bytes(B, Lr, NFFT, HOP)
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    sums = torch.full((B, 8), 7.0, dtype=torch.float64, device="cuda")
    mse = torch.full((B,), 7.0, dtype=torch.float64, device="cuda")
    P = torch.full((B, 1 + Lr // HOP, NFREQ), 7.0, device="cuda")
    p, X, N, W, st = plan(), l.ptr(x), l.ptr(lens), l.ptr(ws), l.stream()

    def refused(rc, text):
        assert rc == FD_EINVAL and text in lib().fd_last_error(), (rc, lib().fd_last_error())

    # a clip under 769 samples for the spectral metric (the row length is what the host sees)
    refused(lib().fd_metrics_logspec_mse(p, X, X, N, B, 768, EPS, l.ptr(mse), W, nws, st), b"cannot be reflect-padded")
    refused(lib().fd_metrics_power_spec(p, X, N, B, 768, l.ptr(P), W, nws, st), b"cannot be reflect-padded")
    # a null pointer
    refused(lib().fd_metrics_sisxr(X, None, X, N, B, Lr, l.ptr(sums), W, nws, st), b"null pointer")
    refused(lib().fd_metrics_sisxr(X, X, X, None, B, Lr, l.ptr(sums), W, nws, st), b"null pointer")
    refused(lib().fd_metrics_logspec_mse(None, X, X, N, B, Lr, EPS, l.ptr(mse), W, nws, st), b"null pointer")
    refused(lib().fd_metrics_logspec_mse(p, X, X, N, B, Lr, EPS, None, W, nws, st), b"null pointer")
    refused(lib().fd_metrics_power_spec(p, X, N, B, Lr, l.ptr(P), None, nws, st), b"null pointer")
    # a workspace that is too small
    refused(lib().fd_metrics_sisxr(X, X, X, N, B, Lr, l.ptr(sums), W, lib().fd_metrics_workspace_bytes(B, Lr, 0, 0) - 1, st), b"workspace too small")
    refused(lib().fd_metrics_logspec_mse(p, X, X, N, B, Lr, EPS, l.ptr(mse), W, nws - 1, st), b"workspace too small")
    refused(lib().fd_metrics_power_spec(p, X, N, B, Lr, l.ptr(P), W, nws - 1, st), b"workspace too small")
    refused(lib().fd_metrics_logspec_mse(p, X, X, N, B, Lr, 0.0, l.ptr(mse), W, nws, st), b"eps must be positive")
    torch.cuda.synchronize()
    assert bool((sums == 7.0).all()) and bool((mse == 7.0).all()) and bool((P == 7.0).all())
    # the Python layer names the clip
    from flowdec_amd import metrics
    with pytest.raises(ValueError, match="clip 1 has 768 samples"):
        metrics.logspec_mse_batch([torch.zeros(4000), torch.zeros(768)], [torch.zeros(4000), torch.zeros(768)])
    # a DEVICE length the host cannot see: NaN for that clip, the neighbour untouched by it
    lens2 = torch.tensor([700, Lr], dtype=torch.int32, device="cuda")
    xr = dev((0.1 * np.random.default_rng(1).standard_normal((B, Lr))).astype(np.float32))
    hr = xr * 1.5
    l.check(lib().fd_metrics_logspec_mse(p, l.ptr(hr), l.ptr(xr), l.ptr(lens2), B, Lr, EPS, l.ptr(mse), W, nws, st))
    m = mse.cpu().numpy()
    assert math.isnan(m[0]) and m[1] == call_logspec([hr[1].cpu().numpy()], [xr[1].cpu().numpy()])[0]


# ---- (g) the command line ---------------------------------------------------------------------------------------------------------------
def read_csv(path):
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    return rows[0], rows[1:]


def test_eval_cli_end_to_end(tmp_path):
    from flowdec_amd import eval_cli, metrics
    from flowdec_amd.enhance_cli import save_wav
    rng = np.random.default_rng(21)
    # (name, rate, samples of x_hat, x, y): 44.1 kHz (resampled); a longer x_hat (--crop-to-x matters); a shorter x_hat (unequal under
    # either run: the NaN row); a plain one.  0.3 - 1.2 s each
    spec = [("a", 44100, 30000, 30000, 30000), ("b", 48000, 20000, 19000, 19000), ("c", 48000, 14400, 15000, 15000), ("d", 48000, 57600, 57600, 57600)]
    lines = []
    for name, sr, lh, lx, ly in spec:
        n = max(lh, lx, ly)
        x = (0.1 * rng.standard_normal(n)).astype(np.float32)
        y = (x + 0.05 * rng.standard_normal(n)).astype(np.float32)
        h = (x + 0.01 * rng.standard_normal(n)).astype(np.float32)
        paths = [tmp_path / f"clean_{name}.wav", tmp_path / f"noisy_{name}.wav", tmp_path / f"enh_{name}.wav"]
        for p, s, ln in zip(paths, (x, y, h), (lx, ly, lh)):
            save_wav(str(p), torch.from_numpy(s[:ln]), sr)
        lines.append(" ---> ".join(str(p) for p in paths))
    lst = tmp_path / "triples_list.txt"
    lst.write_text("\n".join(lines) + "\n")

    def run(flags, finite):
        out = tmp_path / ("metrics" + "".join(flags) + ".csv")
        res = eval_cli.run(["--triples", str(lst), "--out", str(out), "--batch-files", "3"] + flags)
        assert res.exit_code == 0 and res.n_scored == 4
        header, rows = read_csv(out)
        assert header == list(eval_cli.CSV_HEADER) and [r[0] for r in rows] == [f"enh_{s[0]}.wav" for s in spec]      # list order
        worst = 0.0
        for i, (row, s) in enumerate(zip(rows, spec)):
            vals = np.array([float(v) for v in row[4:]])
            if s[0] not in finite:
                assert np.isnan(vals).all(), (s[0], vals)
                continue
            sig = eval_cli.crop(*(eval_cli.load_mono(str(tmp_path / f"{k}_{s[0]}.wav"), 48000) for k in ("enh", "clean", "noisy")),
                                "--crop-to-x" in flags, False)
            h, x, y = (v.numpy() for v in sig)
            host = metrics.si_sxr(h, x, y)
            worst = max(worst, float(np.abs(vals[:3] - host).max()))
            np.testing.assert_allclose(vals[:3], host, rtol=0, atol=1e-4)
            lo, hi, ref = mse_interval(h, x)
            host_ls = metrics.logspec_mse(h, x)
            assert lo <= vals[3] <= hi and lo <= host_ls <= hi, (s[0], vals[3], host_ls, lo, hi)
        assert [m[2] for m in res.means] == [len(finite)] * 4
        return worst

    run([], finite="ad")
    worst = run(["--crop-to-x"], finite="abd")
    assert eval_cli.load_mono(str(tmp_path / "enh_a.wav"), 48000).numel() == 32654        # ceil(30000 * 160 / 147): the resample path ran
    report(f"metrics eval_cli 4 triples: max |GPU - host si_sxr| = {worst:.3e} dB (atol 1e-4)")


def test_enhance_cli_eval_writes_metrics_csv(tmp_path):
    from flowdec_amd import enhance_cli
    from test_cli import synthetic_ckpt
    ckpt = synthetic_ckpt()
    for sd in (ckpt["state_dict"], ckpt["_pl_ema_state_dict"]):
        sd["backbone.output_layer.weight"] = sd["backbone.output_layer.weight"] * 0.02
    torch.save(ckpt, tmp_path / "m.ckpt")
    rng = np.random.default_rng(4)
    (tmp_path / "clean").mkdir(); (tmp_path / "noisy").mkdir()
    names = [("p", 14400), ("q", 20000), ("r", 14400)]
    lines = []
    for name, n in names:
        x = (0.1 * rng.standard_normal((1, n))).astype(np.float32)
        enhance_cli.save_wav(str(tmp_path / "clean" / f"{name}.wav"), torch.from_numpy(x), 48000)
        enhance_cli.save_wav(str(tmp_path / "noisy" / f"{name}.wav"), torch.from_numpy(x + 0.05 * rng.standard_normal((1, n)).astype(np.float32)), 48000)
        lines.append(f"{tmp_path / 'clean' / (name + '.wav')} ---> {tmp_path / 'noisy' / (name + '.wav')}")
    (tmp_path / "pairs.txt").write_text("\n".join(lines) + "\n")
    common = ["--ckpt", str(tmp_path / "m.ckpt"), "--files", str(tmp_path / "pairs.txt"), "--N", "1", "--solver", "euler", "--seed", "1"]
    model = enhance_cli.load_from_checkpoint(str(tmp_path / "m.ckpt"), map_location="cuda:0")
    res = enhance_cli.run(common + ["--outdir", str(tmp_path / "off")], model=model)
    assert res.n_done == 3 and (tmp_path / "off" / "triples_list.txt").exists() and not (tmp_path / "off" / "metrics.csv").exists()
    res = enhance_cli.run(common + ["--outdir", str(tmp_path / "on"), "--eval"], model=model)
    assert res.n_done == 3
    header, rows = read_csv(tmp_path / "on" / "metrics.csv")
    assert header[4:] == ["sisdr", "sisir", "sisar", "logspec_mse"] and [r[0] for r in rows] == [f"{n}.wav" for n, _ in names]
    assert all(math.isfinite(float(v)) for r in rows for v in r[4:])
    for n, _ in names:          # --eval changes no output file
        assert (tmp_path / "on" / f"{n}.wav").read_bytes() == (tmp_path / "off" / f"{n}.wav").read_bytes()
