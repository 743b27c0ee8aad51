"""Parity metrics between two waveforms: the reference's own evaluation formulas, used here
to express build-vs-reference differences in the units the paper reports.  Host-side NumPy / torch-CPU, not on the hot path.

* si_sxr      -- SI-SDR / SI-SIR / SI-SAR (flowdec/eval/metrics.py:256-270, components :554-563); pinned by
                 tests/golden/g14_metrics.npz (reference code run on seeded signals).
* logspec_mse -- mean squared error of 10*log10 power spectrograms, 32 ms symmetric-Hann window / 8 ms hop
                 (eval/metrics.py:333-372).  The reference computes the spectrogram with torchaudio, which is not in
                 this image: restated with torch.stft, parity unpinned.

The two of them also run on the GPU over ragged batches (csrc/metrics.hip, include/flowdec_hip.h "Evaluation metrics"): si_sxr_batch and
logspec_mse_batch below, which score a triples list in flowdec_amd/eval_cli.py.  The host functions stay the yardstick of those.

* estoi       -- extended STOI (eval/metrics.py:273-283: pystoi.stoi(x, x_hat, sr, extended=True)), restated from the published
                 algorithm at the end of this file, with estoi_batch on the GPU (csrc/stoi.hip).  The resampler is pinned against
                 scipy.signal.resample_poly; parity with the pystoi package is unpinned (absent offline: scripts/pin_estoi.py).
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L
from . import ops
from .batching import as_clips, length_sorted_batches, ragged_batches  # noqa: F401  (length_sorted_batches: callers take it from here)


def flat(a) -> np.ndarray:
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64).reshape(-1) if np.asarray(a).dtype == np.float64 else np.asarray(a).reshape(-1)


def si_sxr_components(s_hat, s, n):
    s_target = (np.dot(s_hat, s) / np.linalg.norm(s) ** 2) * s
    e_noise = (np.dot(s_hat, n) / np.linalg.norm(n) ** 2) * n
    return s_target, e_noise, s_hat - s_target - e_noise


def si_sxr(x_hat, x, y):
    """-> (si_sdr, si_sir, si_sar) in dB; x = reference signal, y = degraded input (noise n = y - x, or y + x when that has
    less power: the reference's global-phase-flip guard)."""
    x_hat, x, y = flat(x_hat), flat(x), flat(y)
    n = y - x
    if np.linalg.norm(y + x) < np.linalg.norm(y - x):
        n = y + x
    s_target, e_noise, e_art = si_sxr_components(x_hat, x, n)
    p = np.linalg.norm(s_target) ** 2
    return (10 * np.log10(p / np.linalg.norm(e_noise + e_art) ** 2), 10 * np.log10(p / np.linalg.norm(e_noise) ** 2),
            10 * np.log10(p / np.linalg.norm(e_art) ** 2))


def si_sdr(x_hat, x) -> float:
    """Plain scale-invariant SDR of x_hat against x (no noise decomposition), for build-vs-reference comparisons."""
    x_hat, x = flat(x_hat).astype(np.float64), flat(x).astype(np.float64)
    s_target = (np.dot(x_hat, x) / np.dot(x, x)) * x
    return float(10 * np.log10(np.dot(s_target, s_target) / max(np.dot(x_hat - s_target, x_hat - s_target), 1e-300)))


def logspec_mse(x_hat, x, sr: int = 48000, win_dur: float = 32e-3, hop_dur: float = 8e-3, eps: float = 1e-8) -> float:
    n_fft, hop = int(win_dur * sr), int(hop_dur * sr)
    win = torch.signal.windows.hann(n_fft)

    def logspec(a):
        a = torch.as_tensor(np.asarray(flat(a), dtype=np.float32))
        S = torch.stft(a, n_fft, hop_length=hop, win_length=n_fft, window=win, center=True, pad_mode="reflect", return_complex=True)
        return 10 * torch.log10(torch.clamp(S.abs() ** 2, min=eps))
    return float(torch.mean(torch.square(logspec(x) - logspec(x_hat))))


# ---- the same two metrics on the GPU, over ragged batches (csrc/metrics.hip) -------------------------------------------------------------
SISXR_SUMS = ("x.x", "x_hat.x", "x_hat.n", "n.n", "|s_target|^2", "|e_noise|^2", "|e_art|^2", "|e_noise+e_art|^2")   # fd_metrics_sisxr


def sisxr_from_sums(sums) -> np.ndarray:
    """[n, 8] float64 sums of fd_metrics_sisxr (layout SISXR_SUMS) -> [n, 3] float64 (si_sdr, si_sir, si_sar) in dB, formed on the host."""
    s = np.asarray(sums, dtype=np.float64).reshape(-1, 8)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.stack([10 * np.log10(s[:, 4] / s[:, 7]), 10 * np.log10(s[:, 4] / s[:, 5]), 10 * np.log10(s[:, 4] / s[:, 6])], axis=1)


def si_sxr_sums_batch(x_hats, xs, ys, batch: int = 8, device="cuda") -> np.ndarray:
    """The float64 sums of fd_metrics_sisxr per clip, [n, 8] (layout SISXR_SUMS)."""
    lib = L.load()
    x_hats, xs, ys = as_clips(x_hats, xs, ys)
    out = np.zeros((len(xs), 8), np.float64)

    def call(rows, lens, idx, Lmax):
        B = len(idx)
        nws = lib.fd_metrics_workspace_bytes(B, Lmax, 0, 0)
        ws = torch.empty(nws, dtype=torch.uint8, device=device)
        sums = torch.empty(B, 8, dtype=torch.float64, device=device)
        L.check(lib.fd_metrics_sisxr(L.ptr(rows[0]), L.ptr(rows[1]), L.ptr(rows[2]), L.ptr(lens), B, Lmax, L.ptr(sums), L.ptr(ws), nws, L.stream()))
        return [sums.cpu().numpy()]

    ragged_batches((x_hats, xs, ys), batch, device, call, [out])
    return out


def si_sxr_batch(x_hats, xs, ys, batch: int = 8, device="cuda") -> np.ndarray:
    """si_sxr of every (x_hat, x, y) on the GPU: lists of 1-D signals of any lengths -> [n, 3] float64 (si_sdr, si_sir, si_sar) in dB.
    Sorted by length, cut into batches of `batch` clips, summed in float64 on the device (two passes), dB formed here."""
    return sisxr_from_sums(si_sxr_sums_batch(x_hats, xs, ys, batch, device))


def logspec_mse_batch(x_hats, xs, sr: int = 48000, win_dur: float = 32e-3, hop_dur: float = 8e-3, eps: float = 1e-8, batch: int = 8,
                      device="cuda") -> np.ndarray:
    """logspec_mse of every (x_hat, x) on the GPU -> [n] float64.  One cached transform plan per (n_fft, hop) (ops.stft_plan).  A clip of
    n_fft / 2 samples or fewer cannot be reflect-padded (torch.stft raises): ValueError naming the clip."""
    lib = L.load()
    n_fft, hop = int(win_dur * sr), int(hop_dur * sr)
    x_hats, xs = as_clips(x_hats, xs)
    lengths = [int(c.numel()) for c in xs]
    for i, l in enumerate(lengths):
        if l <= n_fft // 2:
            raise ValueError(f"logspec_mse: clip {i} has {l} samples, reflect padding of n_fft {n_fft} needs more than {n_fft // 2}")
    out = np.zeros(len(xs), np.float64)
    plan = ops.stft_plan(n_fft, hop, device)

    def call(rows, lens, idx, Lmax):
        B = len(idx)
        nws = lib.fd_metrics_workspace_bytes(B, Lmax, n_fft, hop)
        ws = torch.empty(nws, dtype=torch.uint8, device=device)
        mse = torch.empty(B, dtype=torch.float64, device=device)
        L.check(lib.fd_metrics_logspec_mse(plan, L.ptr(rows[0]), L.ptr(rows[1]), L.ptr(lens), B, Lmax, float(eps), L.ptr(mse), L.ptr(ws), nws,
                                           L.stream()))
        return [mse.cpu().numpy()]

    ragged_batches((x_hats, xs), batch, device, call, [out])
    return out


# ---- ESTOI: the extended short-time objective intelligibility measure ------------------------------------------------------------------
# The reference's ESTOI (eval/metrics.py:273-283) is pystoi.stoi(x, x_hat, sr, extended=True).  pystoi is not in this image, so its
# published arithmetic (Jensen & Taal 2016; pystoi/stoi.py, pystoi/utils.py) is restated here in NumPy float64 -- the yardstick of the
# kernels in csrc/stoi.hip -- and parity with the package itself is UNPINNED (scripts/pin_estoi.py prints it where pystoi is importable).
# What is pinned: the resampling bank against scipy.signal.resample_poly, the band edges and the frame arithmetic (tests/test_estoi_cpu.py).
#   1. resample to 10 kHz when sr differs (pystoi.utils.resample_oct): p = 10000 / g, q = sr / g, fc = 1 / (2 max(p, q)),
#      L = ceil(52 / (28.714 fc / 10)), h = 2 p fc sinc(2 fc t) kaiser(2 L + 1, 0.1102 (60 - 8.7)) over t = -L..L, w = h / sum(h);
#      output m = sum_j x[j] p w[q m - p j + L], ceil(p len / q) outputs
#   2. frames of 256 at hop 128 from range(0, len - 256, 128), window hanning(258)[1:-1]; e_t = 20 log10(||win x_t|| + eps); frame t is
#      kept iff max e - 40 - e_t < 0 (from x alone); the kept windowed frames of both signals are overlap-added at hop 128
#   3. the same framing of the compacted signals (k kept frames -> k - 1 spectral frames), windowed again, rfft(512), 15 third-octave
#      bands from 150 Hz: sqrt of the sum of |X|^2 over [lo_i, hi_i)
#   4. fewer than 30 spectral frames: 1e-5 (pystoi's value, with its warning)
#   5. every block of 30 consecutive frames x 15 bands of either signal: rows centred and divided by their 2-norm, then columns;
#      estoi = sum(x_n y_n) / 30 / segments
# The one deliberate deviation: pystoi adds eps * randn before each normalisation (an effect below 1e-12); it is left out, and a row or
# column whose sum of squares is exactly 0 normalises to zeros (pystoi: a random unit vector, expected contribution 0).
ESTOI_FS, ESTOI_FRAME, ESTOI_HOP, ESTOI_NFFT, ESTOI_NBANDS, ESTOI_SEG, ESTOI_DYN_DB = 10000, 256, 128, 512, 15, 30, 40.0
ESTOI_TOO_SHORT = 1e-5
ESTOI_EPS = float(np.finfo(float).eps)
ESTOI_SHORT_RULE = (f"fewer than {ESTOI_SEG} spectral frames are left at 10 kHz after the silent frames are removed "
                    f"(frames of {ESTOI_FRAME} at hop {ESTOI_HOP}): ESTOI is {ESTOI_TOO_SHORT:g} by pystoi's rule")


def estoi_band_edges():
    """-> [(lo, hi)] * 15: the rfft bins [lo, hi) of the third-octave bands (pystoi.utils.thirdoct(10000, 512, 15, 150))."""
    f = np.linspace(0, ESTOI_FS, ESTOI_NFFT + 1)[:ESTOI_NFFT // 2 + 1]
    k = np.arange(ESTOI_NBANDS, dtype=np.float64)
    lo, hi = 150.0 * np.power(2.0, (2 * k - 1) / 6), 150.0 * np.power(2.0, (2 * k + 1) / 6)
    return [(int(np.argmin(np.square(f - a))), int(np.argmin(np.square(f - b)))) for a, b in zip(lo, hi)]


def estoi_filter(sr: int):
    """-> (w float64 [2 L + 1], p, q, L): the normalised Kaiser-windowed sinc of pystoi.utils.resample_oct for sr -> 10 kHz."""
    sr = int(sr)
    if sr < 1:
        raise ValueError(f"estoi: the rate must be positive (got {sr})")
    g = math.gcd(ESTOI_FS, sr)
    p, q = ESTOI_FS // g, sr // g
    fc = 1.0 / (2 * max(p, q))
    L = int(math.ceil(52.0 / (28.714 * fc / 10)))
    t = np.arange(-L, L + 1, dtype=np.float64)
    h = 2 * p * fc * np.sinc(2 * fc * t) * np.kaiser(2 * L + 1, 0.1102 * (60 - 8.7))
    return h / np.sum(h), p, q, L


def _estoi_bank64(sr: int):
    w, p, q, L = estoi_filter(sr)
    o, n = q, p
    width = -(-L // p)
    K = 2 * width + o
    idx = o * np.arange(n)[:, None] - n * (np.arange(K)[None, :] - width) + L
    ok = (idx >= 0) & (idx <= 2 * L)
    return np.where(ok, p * w[np.clip(idx, 0, 2 * L)], 0.0), o, n, width


def estoi_bank(sr: int):
    """-> (bank float32 [n][K], o, n, width): pystoi's resampling filter for sr -> 10 kHz as the polyphase bank of fd_resample_plan_create
    (K = 2 width + o; bank[i][k] = p w[o i - n (k - width) + L] inside the filter, else 0), computed in float64 and rounded once."""
    bank, o, n, width = _estoi_bank64(sr)
    return np.ascontiguousarray(bank.astype(np.float32)), o, n, width


def polyphase_resample(x: np.ndarray, bank: np.ndarray, o: int, n: int, width: int) -> np.ndarray:
    """fd_resample's documented loop on the host: output q n + i = sum_k bank[i][k] x[q o + k - width] (zero outside the signal), float64
    sums, ceil(n len / o) outputs."""
    x = np.asarray(x, np.float64).reshape(-1)
    K = bank.shape[1]
    M = -(-n * len(x) // o)
    Q = max(-(-M // n), 1)
    xp = np.zeros(max((Q - 1) * o + K, width + len(x)), np.float64)
    xp[width:width + len(x)] = x
    win = np.lib.stride_tricks.sliding_window_view(xp, K)[::o][:Q]
    return (win @ np.asarray(bank, np.float64).T).reshape(-1)[:M]


def _estoi_frames(sig: np.ndarray) -> np.ndarray:
    """[T, 256] frames from range(0, len - 256, 128) (a view): the frame that would end exactly at len is not taken (pystoi's loop)."""
    starts = np.arange(0, len(sig) - ESTOI_FRAME, ESTOI_HOP)
    if len(starts) == 0:
        return np.zeros((0, ESTOI_FRAME), np.float64)
    return np.lib.stride_tricks.sliding_window_view(sig, ESTOI_FRAME)[starts]


def _unit_rows(a: np.ndarray, axis: int) -> np.ndarray:
    a = a - a.mean(axis=axis, keepdims=True)
    nrm = np.sqrt(np.sum(a * a, axis=axis, keepdims=True))
    return np.divide(a, nrm, out=np.zeros_like(a), where=nrm > 0)


def estoi_detail(x_hat, x, sr: int, precision: str = "float64", keep_spectra: bool = False) -> dict:
    """ESTOI with its intermediate results: value, too_short, frames / kept (source frame of every kept frame) / spectral_frames,
    margin_db (the least distance of a frame's energy from the 40 dB threshold), tob_x / tob_x_hat ([T, 15] band magnitudes or None).
    precision='float32' rounds to float32 where the kernels of csrc/stoi.hip round (the resampled signals -- through the float32 bank --,
    |X|^2 and the band magnitudes): it measures what those roundings move, it is not a second yardstick.
    keep_spectra adds spec_x / spec_x_hat ([T, 257] complex rfft of the doubly windowed frames) and abs1_x / abs1_x_hat ([T], the sum of
    |samples| of every such frame): what an error bound of a float32 transform needs."""
    if precision not in ("float64", "float32"):
        raise ValueError(f"estoi: precision is 'float64' or 'float32' (got {precision!r})")
    f32 = precision == "float32"
    x, y = (np.asarray(flat(a), dtype=np.float64) for a in (x, x_hat))
    if len(x) != len(y):
        raise ValueError(f"estoi: the signals differ in length (x_hat {len(y)}, x {len(x)})")
    if int(sr) != ESTOI_FS:
        if f32:
            bank, o, n, width = estoi_bank(sr)
            x, y = (polyphase_resample(a.astype(np.float32), bank, o, n, width).astype(np.float32).astype(np.float64) for a in (x, y))
        else:
            bank, o, n, width = _estoi_bank64(sr)
            x, y = (polyphase_resample(a, bank, o, n, width) for a in (x, y))
    win = np.hanning(ESTOI_FRAME + 2)[1:-1]
    out = dict(value=ESTOI_TOO_SHORT, too_short=True, frames=0, kept=np.zeros(0, np.int64), spectral_frames=0, margin_db=float("inf"), tob_x=None,
               tob_x_hat=None)
    xf, yf = _estoi_frames(x) * win, _estoi_frames(y) * win
    out["frames"] = len(xf)
    if len(xf) == 0:
        return out
    e = 20 * np.log10(np.linalg.norm(xf, axis=1) + ESTOI_EPS)
    gap = np.max(e) - ESTOI_DYN_DB - e
    kept = np.nonzero(gap < 0)[0]
    k = len(kept)
    out.update(kept=kept, spectral_frames=max(k - 1, 0), margin_db=float(np.min(np.abs(gap))))
    if k < 2:
        return out

    def bands(fr):
        sig = np.zeros((k + 1) * ESTOI_HOP, np.float64)                   # overlap-add of the kept frames: (k - 1) 128 + 256 samples
        sig[:k * ESTOI_HOP].reshape(k, ESTOI_HOP)[:] += fr[kept, :ESTOI_HOP]
        sig[ESTOI_HOP:].reshape(k, ESTOI_HOP)[:] += fr[kept, ESTOI_HOP:]
        z = _estoi_frames(sig) * win
        X = np.fft.rfft(z, n=ESTOI_NFFT, axis=1)
        P = np.abs(X) ** 2
        if f32:
            P = P.astype(np.float32).astype(np.float64)
        tob = np.sqrt(np.stack([P[:, lo:hi].sum(axis=1) for lo, hi in estoi_band_edges()], axis=1))
        return (tob.astype(np.float32).astype(np.float64) if f32 else tob), X, np.abs(z).sum(axis=1)

    (tx, Xx, ax), (ty, Xy, ay) = bands(xf), bands(yf)
    out.update(tob_x=tx, tob_x_hat=ty)
    if keep_spectra:
        out.update(spec_x=Xx, spec_x_hat=Xy, abs1_x=ax, abs1_x_hat=ay)
    T = len(tx)
    if T < ESTOI_SEG:
        return out

    def segments(tob):                                                      # [J, 15, 30], rows then columns normalised
        s = np.lib.stride_tricks.sliding_window_view(tob, ESTOI_SEG, axis=0)
        return _unit_rows(_unit_rows(s, 2), 1)

    xn, yn = segments(tx), segments(ty)
    out.update(value=float(np.sum(xn * yn / ESTOI_SEG) / xn.shape[0]), too_short=False)
    return out


def estoi(x_hat, x, sr: int, precision: str = "float64") -> float:
    """ESTOI of estimate x_hat against clean x at rate sr (the algorithm above; float64, NumPy only).  1e-5 under the 30-frame rule."""
    return estoi_detail(x_hat, x, sr, precision)["value"]


class _EstoiPlans:
    """The device tables of fd_metrics_estoi and the 10 kHz resample plan of one rate (None at 10 kHz)."""

    def __init__(self, sr):
        lib = L.load()
        self._estoi, self._resample = L.Handle("fd_estoi_plan_destroy"), None
        self.estoi, self.resample, self.o, self.n = self._estoi.handle, None, 1, 1
        if int(sr) != ESTOI_FS:
            bank, o, n, width = estoi_bank(sr)
            if n * bank.shape[1] > (1 << 24):
                raise ValueError(f"estoi: the 10 kHz filter bank of {sr} Hz has {n} x {bank.shape[1]} coefficients, over the device resampler's cap")
            self._resample = L.Handle("fd_resample_plan_destroy")
            self.resample, self.o, self.n = self._resample.handle, o, n
            L.check(lib.fd_resample_plan_create(bank.ctypes.data_as(C.c_void_p), o, n, width, C.byref(self.resample)))
        L.check(lib.fd_estoi_plan_create(C.byref(self.estoi)))


def estoi_plans(sr: int, device="cuda") -> _EstoiPlans:
    """The plans of one rate on one device, created on first use."""
    return L.cached_plan(device, ("estoi", int(sr)), lambda: _EstoiPlans(sr))


def estoi_batch(x_hats, xs, sr: int = 48000, batch: int = 8, device="cuda", return_frames: bool = False):
    """estoi of every (x_hat, x) on the GPU -> [n] float64 (with return_frames also [n, 3] int32: frames, kept, spectral frames; fewer than
    30 spectral frames: 1e-5).  Length-sorted ragged batches of `batch` clips; the plans are cached per (sr, device)."""
    lib = L.load()
    x_hats, xs = as_clips(x_hats, xs)
    out, frames = np.zeros(len(xs), np.float64), np.zeros((len(xs), 3), np.int32)
    plans = estoi_plans(sr, device)

    def call(rows, lens, idx, Lmax):
        B = len(idx)
        nws = lib.fd_metrics_estoi_workspace_bytes(B, Lmax, plans.o, plans.n)
        ws = torch.empty(nws, dtype=torch.uint8, device=device)
        val = torch.empty(B, dtype=torch.float64, device=device)
        fr = torch.empty(B, 3, dtype=torch.int32, device=device)
        L.check(lib.fd_metrics_estoi(plans.estoi, plans.resample, L.ptr(rows[0]), L.ptr(rows[1]), L.ptr(lens), B, Lmax, L.ptr(val), L.ptr(fr),
                                     L.ptr(ws), nws, L.stream()))
        return [val.cpu().numpy(), fr.cpu().numpy()]

    ragged_batches((x_hats, xs), batch, device, call, [out, frames])
    return (out, frames) if return_frames else out
