"""CPU-only checks of the host side of csrc/stft.hip (the STFT / iSTFT front and back end): the plan's DFT tables against a NumPy
float64 mirror, the GEMM tile-width rule against a Python mirror, the iSTFT window-envelope rule against torch.istft itself, and the
GEMM's host-side refusals.  The GPU side is tests/test_hip_stft.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

FD_EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from flowdec_amd import _lib
    return _lib.load()


def kpad(n_fft):
    return (2 * (n_fft // 2 + 1) + 127) // 128 * 128


def hann_f32(n_fft):
    k = np.arange(n_fft, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * k / (n_fft - 1))).astype(np.float32)


def tables_f64(n_fft):
    """(Dt, E, w2) in float64 from the float32 window, laid out as documented at fd_stft_tables."""
    K, F = kpad(n_fft), n_fft // 2 + 1
    w = hann_f32(n_fft).astype(np.float64)
    k, f = np.arange(n_fft)[:, None], np.arange(F)[None, :]
    ang = 2.0 * np.pi * ((k * f) % n_fft) / n_fft
    Dt, E = np.zeros((K, K)), np.zeros((K, K))
    Dt[:n_fft, 0:2 * F:2] = w[:, None] * np.cos(ang)
    Dt[:n_fft, 1:2 * F:2] = -w[:, None] * np.sin(ang)
    cf = np.where((f == 0) | (f == n_fft // 2), 1.0, 2.0)
    E[0:2 * F:2, :n_fft] = (w[:, None] * cf * np.cos(ang) / n_fft).T
    E[1:2 * F:2, :n_fft] = (-w[:, None] * cf * np.sin(ang) / n_fft).T
    w32 = hann_f32(n_fft)
    return Dt, E, (w32 * w32)


def ulps_apart(got, want64):
    """|got - f32(want)| in units of the float32 spacing at that magnitude (0 where both are zero)."""
    want = want64.astype(np.float32)
    sp = np.spacing(np.maximum(np.abs(got), np.abs(want)).astype(np.float32))
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / sp.astype(np.float64)


@pytest.mark.parametrize("n_fft", [1534, 510, 512, 64, 16])
def test_tables_match_float64(lib, n_fft):
    """Every entry of Dt / E within 1 float32 ulp of the float64 value (libm and NumPy cos / sin may differ in the last double bit), the
    zero rows / columns beyond n_fft and the 2F spectrum columns exactly zero, w2 bit-exact."""
    from flowdec_amd import ops
    K, F = kpad(n_fft), n_fft // 2 + 1
    assert lib.fd_stft_tables(n_fft, 384, None, None, None) == K
    Dt, E, w2 = ops.stft_tables(n_fft, 384)
    assert Dt.shape == E.shape == (K, K) and K % 128 == 0 and K >= 2 * F > n_fft
    rDt, rE, rw2 = tables_f64(n_fft)
    assert np.array_equal(w2, rw2)
    assert w2[0] == 0 and w2[-1] == 0 and w2.min() == 0 and (w2[1:-1] > 0).all()
    assert ulps_apart(Dt, rDt).max() <= 1.0
    assert ulps_apart(E, rE).max() <= 1.0
    # padding: rows k >= n_fft of Dt, columns >= 2F of Dt, rows >= 2F of E, columns n >= n_fft of E
    assert not Dt[n_fft:].any() and not Dt[:, 2 * F:].any() and not E[2 * F:].any() and not E[:, n_fft:].any()
    # re / im interleave and the sign of the imaginary part: column 2 is cos(2 pi k / n), column 3 is -sin(2 pi k / n)
    w = hann_f32(n_fft).astype(np.float64)
    k = np.arange(n_fft)
    assert np.allclose(Dt[:n_fft, 2], w * np.cos(2 * np.pi * k / n_fft), rtol=0, atol=1e-7)
    assert np.allclose(Dt[:n_fft, 3], -w * np.sin(2 * np.pi * k / n_fft), rtol=0, atol=1e-7)
    # DC and Nyquist: factor 1 and 1/n; every other bin factor 2
    assert np.array_equal(E[0, :n_fft], (w / n_fft).astype(np.float32))
    assert np.allclose(E[2 * (F - 1), :n_fft], w * np.cos(np.pi * k) / n_fft, rtol=1e-6, atol=0)
    assert np.allclose(E[2, :n_fft], 2 * w * np.cos(2 * np.pi * k / n_fft) / n_fft, rtol=1e-6, atol=1e-12)
    # the imaginary parts of DC (exactly) and Nyquist (sin(pi k) in double: ~1e-16 relative) carry nothing
    assert not Dt[:, 1].any() and not E[1].any()
    assert np.abs(Dt[:, 2 * F - 1]).max() <= 1e-12 and np.abs(E[2 * F - 1]).max() <= 1e-12 / n_fft


def test_tables_refuse_bad_geometry(lib):
    for n_fft, hop in ((0, 384), (1533, 384), (-2, 384), (1534, 0)):
        assert lib.fd_stft_tables(n_fft, hop, None, None, None) == FD_EINVAL and lib.fd_last_error()
    buf = np.zeros(16, np.float32)
    assert lib.fd_stft_tables(16, 4, buf.ctypes.data, None, buf.ctypes.data) == FD_EINVAL


def gemm_bn(M, N, K):
    """Mirror of sgemm_bn: None where the host refuses."""
    if M < 1 or N < 128 or N % 128 or K < 16 or K % 16:
        return None
    return 128 if -(-M // 128) * (N // 128) >= 512 else 32


def test_gemm_variant_rule_matches_mirror(lib):
    from flowdec_amd import ops
    Ms = [-1, 0, 1, 31, 127, 128, 129, 2008, 5376, 5377, 8032, 13056, 13057, 16256, 16257, 65408, 65409]
    Ns = [0, 64, 100, 128, 256, 512, 640, 1536, 1600]
    Ks = [0, 8, 16, 24, 128, 512, 640, 1536]
    seen = set()
    for M in Ms:
        for N in Ns:
            for K in Ks:
                want, got = gemm_bn(M, N, K), lib.fd_stft_gemm_variant(M, N, K)
                if want is None:
                    assert got == FD_EINVAL and b"unsupported shape" in lib.fd_last_error(), (M, N, K)
                else:
                    assert got == want == ops.stft_gemm_variant(M, N, K), (M, N, K, got, want)
                    seen.add(want)
    assert seen == {32, 128}
    # the thresholds the transforms meet: K = N = kpad of n_fft 1534 / 512 / 510 / 64
    assert (lib.fd_stft_gemm_variant(5376, 1536, 1536), lib.fd_stft_gemm_variant(5377, 1536, 1536)) == (32, 128)
    assert (lib.fd_stft_gemm_variant(13056, 640, 640), lib.fd_stft_gemm_variant(13057, 640, 640)) == (32, 128)
    assert (lib.fd_stft_gemm_variant(16256, 512, 512), lib.fd_stft_gemm_variant(16257, 512, 512)) == (32, 128)
    assert (lib.fd_stft_gemm_variant(65408, 128, 128), lib.fd_stft_gemm_variant(65409, 128, 128)) == (32, 128)
    assert [kpad(n) for n in (1534, 512, 510, 64, 16)] == [1536, 640, 512, 128, 128]


def torch_istft_raises(n_fft, hop, T, L, win):
    X = torch.zeros(n_fft // 2 + 1, T, dtype=torch.complex128)
    try:
        torch.istft(X, n_fft, hop_length=hop, window=win, center=True, length=L)
    except RuntimeError as e:
        assert "window overlap add min" in str(e), str(e)
        return True
    return False


def envelope_hops(n_fft):
    if n_fft <= 64:
        return range(1, n_fft + 1)
    h = n_fft // 2
    return sorted({1, 2, 3, 7, 64, 100, 384, h - 2, h - 1, h, h + 1, h + 2, h + 50, n_fft - 3, n_fft - 2, n_fft - 1, n_fft} |
                  set(range(5, n_fft, n_fft // 17)))


@pytest.mark.parametrize("n_fft", [16, 64, 512, 1534])
def test_envelope_rule_matches_torch_istft(lib, n_fft):
    """fd_istft_envelope_ok(n_fft, hop, T, L) == not torch.istft(center=True, length=L) raising, float64 and the symmetric Hann window.
    Raising is monotone in L (a longer output keeps more envelope samples), so for each (hop, T) torch's first raising length L* is found
    by bisection and the rule is checked at L* - 1, L*, L* + 1 and around the analytic boundary n_fft/2 + hop (T - 1) of the last sample."""
    from flowdec_amd import ops
    win = torch.signal.windows.hann(n_fft, dtype=torch.float64)
    checked = refused = 0
    for hop in envelope_hops(n_fft):
        for T in (1, 2, 3, 7):
            total = n_fft + hop * (T - 1)
            Lmax = total - n_fft // 2 + 3                 # past the synthesised range: zero tail, no further envelope samples
            lo, hi = 0, Lmax + 1                          # torch accepts lo (or lo = 0), raises at hi (or hi = Lmax + 1: never)
            if torch_istft_raises(n_fft, hop, T, 1, win):
                hi = 1
            else:
                lo = 1
                while hi - lo > 1:
                    mid = (lo + hi) // 2
                    if torch_istft_raises(n_fft, hop, T, mid, win):
                        hi = mid
                    else:
                        lo = mid
            bound = n_fft // 2 + hop * (T - 1)
            for L in {1, 2, hi - 1, hi, hi + 1, bound - 1, bound, bound + 1, Lmax}:
                if L < 1 or L > Lmax:
                    continue
                want = not torch_istft_raises(n_fft, hop, T, L, win)
                assert want == (L < hi)
                got = lib.fd_istft_envelope_ok(n_fft, hop, T, L)
                assert got == int(want), (n_fft, hop, T, L, got, want)
                assert ops.istft_envelope_ok(n_fft, hop, T, L) == want
                checked += 1
                refused += not want
            # enhance's own geometry: T = 1 + L / hop never meets a zero envelope when hop <= n_fft / 2
            if 2 * hop <= n_fft:
                for L in range(max(1, hop * (T - 1)), hop * T):
                    if n_fft // 2 < L:
                        assert lib.fd_istft_envelope_ok(n_fft, hop, 1 + L // hop, L) == 1, (n_fft, hop, L)
    assert checked > 200 and refused > 50
    # the worked example: T = 9 frames at n_fft 1534 / hop 384 take length 3838, not 3839
    if n_fft == 1534:
        assert lib.fd_istft_envelope_ok(1534, 384, 9, 3838) == 1 and lib.fd_istft_envelope_ok(1534, 384, 9, 3839) == 0
    for args in ((n_fft, 0, 3, 100), (n_fft, 4, 0, 100), (n_fft, 4, 3, 0), (n_fft + 1, 4, 3, 100)):
        assert lib.fd_istft_envelope_ok(*args) == FD_EINVAL


REFUSALS = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
from flowdec_amd import _lib
lib = _lib.load()
p, q = C.c_void_p(4096), C.c_void_p(4100)    # never dereferenced: every call below must be refused on the host before any launch
calls = [  # A, B, C, M, N, K
    ("unsupported shape", (p, p, p, 0, 1536, 1536)),
    ("unsupported shape", (p, p, p, -5, 1536, 1536)),
    ("unsupported shape", (p, p, p, 100, 1600, 1536)),
    ("unsupported shape", (p, p, p, 100, 64, 1536)),
    ("unsupported shape", (p, p, p, 100, 0, 1536)),
    ("unsupported shape", (p, p, p, 100, 1536, 1528)),
    ("unsupported shape", (p, p, p, 100, 1536, 0)),
    ("16-byte aligned", (q, p, p, 100, 1536, 1536)),
    ("16-byte aligned", (p, q, p, 6000, 1536, 1536)),
    ("16-byte aligned", (p, p, q, 1, 128, 16)),
    ("null pointer", (None, p, p, 100, 1536, 1536)),
    ("null pointer", (p, p, None, 100, 1536, 1536)),
]
for want, args in calls:
    rc = lib.fd_stft_gemm_f32(*args, None)
    msg = (lib.fd_last_error() or b"").decode()
    assert rc == -1 and want in msg, (want, rc, msg)
print("REFUSED", len(calls))
"""


def test_gemm_refusals_happen_on_the_host():
    """fd_stft_gemm_f32 refuses a shape the kernel cannot take (M < 1, N not a multiple of 128, K not of 16) or a misaligned pointer
    (the kernel loads A and B as float4) with FD_EINVAL before any launch.  The calls run in a child process that sees no GPU, so a
    refusal that went missing shows as a launch error, never as a launch.  (The iSTFT's envelope refusal needs a plan, which needs a
    device: tests/test_hip_stft.py checks that it leaves the output untouched; its rule is test_envelope_rule_matches_torch_istft.)"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", REFUSALS, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "REFUSED 12" in r.stdout, r.stdout + r.stderr
