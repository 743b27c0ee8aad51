"""Spectral distances between an estimate and a reference waveform: the multi-scale STFT distance and the multi-scale mel distance that
codec papers report, i.e. the arithmetic of the reference's MultiScaleSTFTLoss and MelSpectrogramLoss (flowdec/losses.py) at their default
parameters, as metrics without gradients.  Host yardsticks in NumPy float64 and the GPU path over ragged batches (csrc/specdist.hip,
include/flowdec_hip.h "Spectral distances"), which scores a triples list in flowdec_amd/eval_cli.py (--spectral).

All of it is per clip (the reference's value for a batch of one).

* transform   one-sided STFT of window length N, hop N / 4, center=True with reflect padding by N / 2, PERIODIC Hann window
              w[k] = 0.5 - 0.5 cos(2 pi k / N), not normalised: T = 1 + len // hop frames, F = N / 2 + 1 bins
* msstft      N in (4096, 2048, 1024, 512); per scale the mean over F x T of |2 log10 max(A, 1e-5) - 2 log10 max(R, 1e-5)| + |A - R| with
              A = |STFT(x_hat)|, R = |STFT(x)|; the sum over the scales
* mel         (N, n_mels) in ((128, 10), (256, 20), (512, 40), (1024, 80), (2048, 160), (4096, 320)); M = fb^T |X|^2; per scale the mean
              over n_mels x T of |2 log10 max(M_hat, 1e-5) - 2 log10 max(M, 1e-5)| (the square of a spectrogram that is a power already is
              the reference's); no magnitude term (mag_weight 0); the sum over the scales
* bank        fb [F][n_mels]: triangles on the HTK mel scale between 0 and sr // 2 with Slaney's area normalisation (mel_filterbank)

A clip of max(N) / 2 = 2048 samples or fewer cannot be reflect-padded at the largest scale (torch.stft raises): NaN in both metrics.

The reference builds its bank with torchaudio.functional.melscale_fbanks (float32).  torchaudio is not available to the tests, so the bank
is restated here from the published formulas in float64, and parity with the package is UNPINNED (scripts/pin_mel.py prints it where
torchaudio is importable).  What is pinned: the yardsticks against torch.stft in float64, the bank's defining properties, the tables of
the GPU path against this module (tests/test_specdist_cpu.py), and the GPU path against the yardsticks (tests/test_hip_specdist.py).
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L
from .batching import as_clips, ragged_batches
from .metrics import flat

CLAMP_EPS = 1e-5
MSSTFT_SCALES = (4096, 2048, 1024, 512)
MEL_SCALES = ((128, 10), (256, 20), (512, 40), (1024, 80), (2048, 160), (4096, 320))
# both metrics in one pass over six transforms: (N, n_mels or 0, stft term)
PLAN_SCALES = ((128, 10, False), (256, 20, False), (512, 40, True), (1024, 80, True), (2048, 160, True), (4096, 320, True))
MIN_SAMPLES = max(MSSTFT_SCALES) // 2 + 1        # 2049: the shortest clip the largest scale takes
SHORT_RULE = (f"reflect padding of the {max(MSSTFT_SCALES)}-sample window needs at least {MIN_SAMPLES} samples: "
              f"NaN for msstft and mel")
NAMES = ("msstft", "mel")


def hz_to_mel(f: float) -> float:
    return 2595.0 * math.log10(1.0 + f / 700.0)


def mel_points(sr: int, n_mels: int) -> np.ndarray:
    """-> f_pts float64 [n_mels + 2]: the filters' edges and centres in Hz, equally spaced on the HTK mel scale over [0, sr // 2]."""
    m_max = hz_to_mel(float(sr // 2))
    step = m_max / float(n_mels + 1)
    return np.array([700.0 * (math.pow(10.0, (m_max if i == n_mels + 1 else i * step) / 2595.0) - 1.0) for i in range(n_mels + 2)], np.float64)


def mel_filterbank(sr: int, n_fft: int, n_mels: int) -> np.ndarray:
    """-> fb float64 [n_fft / 2 + 1][n_mels]: fb[f][j] = max(0, min((f_f - p_j) / (p_j+1 - p_j), (p_j+2 - f_f) / (p_j+2 - p_j+1))) times
    2 / (p_j+2 - p_j), with f_f = linspace(0, sr // 2, F) and p = mel_points (melscale_fbanks(F, 0, sr // 2, n_mels, sr, norm='slaney',
    mel_scale='htk') in float64)."""
    F = n_fft // 2 + 1
    fmax = float(sr // 2)
    freqs = np.arange(F, dtype=np.float64) * (fmax / float(F - 1))
    freqs[-1] = fmax
    p = mel_points(sr, n_mels)
    down = (freqs[:, None] - p[None, :-2]) / (p[1:-1] - p[:-2])[None, :]
    up = (p[None, 2:] - freqs[:, None]) / (p[2:] - p[1:-1])[None, :]
    return np.maximum(0.0, np.minimum(down, up)) * (2.0 / (p[2:] - p[:-2]))[None, :]


def hann_periodic(n: int) -> np.ndarray:
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n, dtype=np.float64) / n)


def frames(x: np.ndarray, n_fft: int) -> np.ndarray:
    """[T, n_fft] float64: the centred frames at hop n_fft / 4 of the reflect-padded signal, T = 1 + len // hop (no window)."""
    x = np.asarray(x, np.float64).reshape(-1)
    if len(x) <= n_fft // 2:
        raise ValueError(f"specdist: a clip of {len(x)} samples cannot be reflect-padded by {n_fft // 2}")
    xp = np.pad(x, n_fft // 2, mode="reflect")
    return np.lib.stride_tricks.sliding_window_view(xp, n_fft)[::n_fft // 4]


def stft(x: np.ndarray, n_fft: int) -> np.ndarray:
    """[T, F] complex128: the transform above."""
    return np.fft.rfft(frames(x, n_fft) * hann_periodic(n_fft), axis=1)


def _log2(v: np.ndarray) -> np.ndarray:
    return 2.0 * np.log10(np.maximum(v, CLAMP_EPS))


def _pair(x_hat, x):
    x_hat, x = (np.asarray(flat(a), dtype=np.float64) for a in (x_hat, x))
    if len(x_hat) != len(x):
        raise ValueError(f"specdist: the signals differ in length (x_hat {len(x_hat)}, x {len(x)})")
    return x_hat, x


def detail(x_hat, x, sr: int = 48000, scales=PLAN_SCALES) -> dict:
    """Both metrics with their intermediate results, float64: msstft, mel, and per scale (N, n_mels, stft) a dict with spec_hat / spec_x
    ([T, F] complex), mel_hat / mel_x ([T, n_mels] or None), terms (stft log, stft mag, mel log means; 0.0 for a term the scale does not
    have) and energy ([T]: sum of (w x_hat)^2 + (w x)^2 over each frame -- what an error bound of a float32 transform needs).
    A clip too short for the largest scale: msstft = mel = NaN and no scales."""
    x_hat, x = _pair(x_hat, x)
    out = dict(msstft=float("nan"), mel=float("nan"), scales=[])
    if len(x) <= max(n for n, _, _ in scales) // 2:
        return out
    msstft, mel = 0.0, 0.0
    for n_fft, n_mels, has_stft in scales:
        w = hann_periodic(n_fft)
        fh, fx = frames(x_hat, n_fft) * w, frames(x, n_fft) * w
        Sh, Sx = np.fft.rfft(fh, axis=1), np.fft.rfft(fx, axis=1)
        A, R = np.abs(Sh), np.abs(Sx)
        terms = [0.0, 0.0, 0.0]
        if has_stft:
            terms[0] = float(np.mean(np.abs(_log2(A) - _log2(R))))
            terms[1] = float(np.mean(np.abs(A - R)))
            msstft += terms[0]
            msstft += terms[1]
        Mh = Mx = None
        if n_mels:
            fb = mel_filterbank(sr, n_fft, n_mels)
            Mh, Mx = (A ** 2) @ fb, (R ** 2) @ fb
            terms[2] = float(np.mean(np.abs(_log2(Mh) - _log2(Mx))))
            mel += terms[2]
        out["scales"].append(dict(n_fft=n_fft, n_mels=n_mels, stft=bool(has_stft), spec_hat=Sh, spec_x=Sx, mel_hat=Mh, mel_x=Mx, terms=tuple(terms),
                                  energy=np.sum(fh * fh, axis=1) + np.sum(fx * fx, axis=1)))
    out.update(msstft=msstft, mel=mel)
    return out


def multiscale_stft_distance(x_hat, x, scales=MSSTFT_SCALES) -> float:
    """The multi-scale STFT distance of x_hat against x (the definition above; NumPy float64).  NaN for a clip too short for the largest scale."""
    return detail(x_hat, x, scales=tuple((int(n), 0, True) for n in scales))["msstft"]


def mel_distance(x_hat, x, sr: int = 48000, scales=MEL_SCALES) -> float:
    """The multi-scale mel distance of x_hat against x at rate sr (the definition above; NumPy float64).  NaN for a clip too short."""
    return detail(x_hat, x, sr, tuple((int(n), int(m), False) for n, m in scales))["mel"]


def tables(sr: int, n_fft: int, n_mels: int):
    """fd_specdist_tables on the host (no GPU): -> (window float32 [N], twiddle float32 [N / 2][2], first int32 [n_mels], count int32
    [n_mels], weights float32 [sum of count])."""
    lib = L.load()
    nw = lib.fd_specdist_tables(sr, n_fft, n_mels, None, None, None, None, None)
    L.check(min(nw, 0))
    win, tw = np.zeros(n_fft, np.float32), np.zeros((n_fft // 2, 2), np.float32)
    first, count, w = np.zeros(max(n_mels, 1), np.int32), np.zeros(max(n_mels, 1), np.int32), np.zeros(max(nw, 1), np.float32)
    L.check(min(lib.fd_specdist_tables(sr, n_fft, n_mels, win.ctypes.data, tw.ctypes.data, first.ctypes.data, count.ctypes.data, w.ctypes.data), 0))
    return win, tw, first[:n_mels], count[:n_mels], w[:nw]


class SpecdistPlan(L.Handle):
    """The device tables of fd_metrics_specdist for one rate and one list of scales (N, n_mels or 0, stft term)."""

    def __init__(self, sr, scales=PLAN_SCALES):
        super().__init__("fd_specdist_plan_destroy")
        lib = L.load()
        self.sr, self.scales = int(sr), tuple((int(n), int(m), bool(s)) for n, m, s in scales)
        k = len(self.scales)
        arr = [(C.c_int * k)(*[int(s[i]) for s in self.scales]) for i in range(3)]
        L.check(lib.fd_specdist_plan_create(self.sr, k, arr[0], arr[1], arr[2], C.byref(self.handle)))


def specdist_plan(sr: int, device="cuda") -> SpecdistPlan:
    """The default plan (PLAN_SCALES) of one rate on one device, created on first use."""
    return L.cached_plan(device, ("specdist", int(sr)), lambda: SpecdistPlan(sr))


def spectral_distances_batch(x_hats, xs, sr: int = 48000, batch: int = 8, device="cuda", return_terms: bool = False):
    """(msstft, mel) of every (x_hat, x) on the GPU -> [n, 2] float64 (with return_terms also [n, 6, 3]: the stft log, stft mag and mel log
    means of every scale of PLAN_SCALES).  Length-sorted ragged batches of `batch` clips; one cached plan per (sr, device).  A clip of 2048
    samples or fewer cannot be reflect-padded at the largest scale: ValueError naming the clip."""
    lib = L.load()
    x_hats, xs = as_clips(x_hats, xs)
    for i, c in enumerate(xs):
        if int(c.numel()) < MIN_SAMPLES:
            raise ValueError(f"specdist: clip {i} has {int(c.numel())} samples, {SHORT_RULE}")
    plan = specdist_plan(sr, device)
    k = len(plan.scales)
    out, terms = np.zeros((len(xs), 2), np.float64), np.zeros((len(xs), k, 3), np.float64)

    def call(rows, lens, idx, Lmax):
        B = len(idx)
        nws = lib.fd_metrics_specdist_workspace_bytes(plan.handle, B, Lmax)
        ws = torch.empty(nws, dtype=torch.uint8, device=device)
        val = torch.empty(B, 2, dtype=torch.float64, device=device)
        tm = torch.empty(B, k, 3, dtype=torch.float64, device=device)
        L.check(lib.fd_metrics_specdist(plan.handle, L.ptr(rows[0]), L.ptr(rows[1]), L.ptr(lens), B, Lmax, L.ptr(val), L.ptr(tm), L.ptr(ws), nws,
                                        L.stream()))
        return [val.cpu().numpy(), tm.cpu().numpy()]

    ragged_batches((x_hats, xs), batch, device, call, [out, terms])
    return (out, terms) if return_terms else out
