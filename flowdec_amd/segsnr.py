"""Segmental SNR (`SSNR`) and frequency-weighted segmental SNR (`fwSSNR`) of an estimate against a reference waveform: the two columns of
the reference's default metric list (flowdec/eval/metrics.py InitializeMetrics) that it takes from the pysepm package (SNRseg and fwSNRseg
with frameLen=0.03, overlap=0.75), i.e. Hu & Loizou's comp_snr.m / comp_fwseg.m.  Host yardsticks in NumPy float64 -- the definition -- and
the GPU path over ragged batches (csrc/segsnr.hip, include/flowdec_hip.h "Segmental SNRs"), which scores a triples list in
flowdec_amd/eval_cli.py (--ssnr).

Shared by both, at rate sr, with eps = 2^-52:

* frames      win = round(0.03 sr) samples, skip = floor(0.25 * 0.03 * sr), frame t = samples [t skip, t skip + win), T = (len - win) // skip
              frames: no centring, no reflection, and the last full frame is dropped (SNRseg builds (len - win + skip) // skip frames and
              removes the last one; fwSNRseg cuts the signal to int(len / skip - win / skip) skip + win - skip samples before an unpadded
              STFT).  T = 0 (len < win + skip): NaN in both.
* window      w[n] = 0.5 (1 - cos(2 pi (n + 1) / (win + 1))), n < win
* SSNR        a = w x, b = w x_hat (float32 samples widened to float64); per frame 10 log10(sum a^2 / (sum (a - b)^2 + eps) + eps), clipped to
              [-10, 35]; the mean over the frames.  A frame where x is digitally silent scores -10 (the package's behaviour).
* fwSSNR      both signals + eps; per signal |DFT| of the windowed frame at n_fft = 2^ceil(log2(2 win)) points, bins 0 .. n_fft / 2 - 1
              (the Nyquist bin is dropped), divided by its sum over those bins; ce = bank @ clean, pe = bank @ processed over the 25
              critical bands below; err = max((ce - pe)^2, eps); per frame sum(ce^0.2 10 log10(ce^2 / err)) / sum(ce^0.2), clipped to
              [-10, 35]; the mean over the frames.
* bank        with h = n_fft / 2, f0 = floor(cent / (sr / 2) h), bw = band / (sr / 2) h: filter i at bin j is
              exp(-11 ((j - f0) / bw)^2 + ln 70 - ln band_i), set to 0 where it is not above exp(-30 / (2 * 2.303)).  The bands stop at
              3.8 kHz whatever sr is: that is the published measure.

The 25 centre frequencies and bandwidths are the table of comp_fwseg.m: seven bands of 70 Hz, then band_i = cent_(i+1) - cent_i up to
346.136 Hz at 3597.63 Hz (tests/test_segsnr_cpu.py checks that relation).

pysepm is not available to the tests, so the arithmetic is restated here from the published algorithm and parity with the package is
UNPINNED (scripts/pin_segsnr.py prints it where pysepm is importable).  What is pinned: the yardstick against a transcription through
scipy.signal.stft, the frame rule, the bank's defining properties and hand values, the tables of the GPU path against this module
(tests/test_segsnr_cpu.py), and the GPU path against the yardstick (tests/test_hip_segsnr.py).
"""
import ctypes as C
import functools
import math

import numpy as np
import torch

from . import _lib as L
from .batching import as_clips, ragged_batches
from .metrics import flat

EPS = 2.0 ** -52
MIN_SNR, MAX_SNR = -10.0, 35.0
FRAME_LEN, OVERLAP, GAMMA = 0.03, 0.75, 0.2
CENT_FREQ = (50.0, 120.0, 190.0, 260.0, 330.0, 400.0, 470.0, 540.0, 617.372, 703.378, 798.717, 904.128, 1020.38, 1148.30, 1288.72, 1442.54,
             1610.70, 1794.16, 1993.93, 2211.08, 2446.71, 2701.97, 2978.04, 3276.17, 3597.63)
BANDWIDTH = (70.0, 70.0, 70.0, 70.0, 70.0, 70.0, 70.0, 77.3724, 86.0056, 95.3398, 105.411, 116.256, 127.914, 140.423, 153.823, 168.154,
             183.457, 199.776, 217.153, 235.631, 255.255, 276.072, 298.126, 321.465, 346.136)
NUM_BANDS = len(CENT_FREQ)
MIN_FACTOR = math.exp(-30.0 / (2.0 * 2.303))
NAMES = ("fwSSNR", "SSNR")          # the reference's metric names, in the order of its default list


def frame_params(sr: int):
    """-> (win, skip, n_fft) of rate sr."""
    win = int(round(FRAME_LEN * sr))
    skip = int(math.floor(0.25 * FRAME_LEN * sr))
    return win, skip, 2 ** int(math.ceil(math.log2(2 * win)))


def num_frames(length: int, sr: int) -> int:
    """T of a clip of `length` samples: (length - win) // skip, 0 below win + skip."""
    win, skip, _ = frame_params(sr)
    return (length - win) // skip if length >= win + skip else 0


def min_samples(sr: int) -> int:
    """The shortest clip with a frame: win + skip."""
    win, skip, _ = frame_params(sr)
    return win + skip


def short_rule(sr: int) -> str:
    win, skip, _ = frame_params(sr)
    return f"the segmental SNRs drop the last {win}-sample frame and need at least {win + skip} samples (win + skip): NaN for fwSSNR and SSNR"


@functools.lru_cache(maxsize=None)
def _window(win: int) -> np.ndarray:
    w = np.array([0.5 * (1.0 - math.cos(2.0 * math.pi * (n + 1) / (win + 1))) for n in range(win)], np.float64)
    w.setflags(write=False)
    return w


def window(win: int) -> np.ndarray:
    """w[n] = 0.5 (1 - cos(2 pi (n + 1) / (win + 1))), float64 [win] (libm's cos, one call per sample)."""
    return _window(int(win))


@functools.lru_cache(maxsize=None)
def _bank(sr: int, n_fft: int) -> np.ndarray:
    h = n_fft // 2
    max_freq = sr / 2.0
    out = np.zeros((NUM_BANDS, h), np.float64)
    for i, (cent, band) in enumerate(zip(CENT_FREQ, BANDWIDTH)):
        f0 = math.floor(cent / max_freq * h)
        bw = band / max_freq * h
        norm = math.log(BANDWIDTH[0]) - math.log(band)
        for j in range(h):
            q = (j - f0) / bw
            v = math.exp(-11.0 * (q * q) + norm)
            out[i, j] = v if v > MIN_FACTOR else 0.0
    out.setflags(write=False)
    return out


def critical_band_bank(sr: int, n_fft: int) -> np.ndarray:
    """-> float64 [25][n_fft / 2]: the Gaussian critical-band filters of the definition above (libm's exp and log, one call per tap)."""
    return _bank(int(sr), int(n_fft))


def band_centres(sr: int, n_fft: int) -> np.ndarray:
    """-> int [25]: f0 of every filter, the bin of its peak."""
    return np.array([math.floor(c / (sr / 2.0) * (n_fft // 2)) for c in CENT_FREQ], np.int64)


def _pair(x_hat, x):
    x_hat, x = (np.asarray(flat(a), dtype=np.float64) for a in (x_hat, x))
    if len(x_hat) != len(x):
        raise ValueError(f"segsnr: the signals differ in length (x_hat {len(x_hat)}, x {len(x)})")
    return x_hat, x


def _frames(sig: np.ndarray, win: int, skip: int, T: int) -> np.ndarray:
    return np.lib.stride_tricks.sliding_window_view(sig, win)[::skip][:T]


def segsnr_detail(x_hat, x, sr: int) -> dict:
    """Both metrics with their per-frame values, float64: fwssnr, ssnr (NaN without a frame), fw_frames, ss_frames ([T], clipped), frames
    (T), and clean_spec / proc_spec ([T, n_fft / 2]: the normalised magnitudes)."""
    x_hat, x = _pair(x_hat, x)
    win, skip, n_fft = frame_params(sr)
    T = (len(x) - win) // skip if len(x) >= win + skip else 0
    out = dict(fwssnr=float("nan"), ssnr=float("nan"), fw_frames=np.zeros(0), ss_frames=np.zeros(0), frames=T, clean_spec=None, proc_spec=None)
    if T == 0:
        return out
    w = window(win)
    a, b = _frames(x, win, skip, T) * w, _frames(x_hat, win, skip, T) * w
    signal, noise = np.sum(a ** 2, axis=1), np.sum((a - b) ** 2, axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        ss = np.clip(10.0 * np.log10(signal / (noise + EPS) + EPS), MIN_SNR, MAX_SNR)
        h = n_fft // 2
        clean = np.abs(np.fft.rfft(_frames(x + EPS, win, skip, T) * w, n_fft, axis=1))[:, :h]
        proc = np.abs(np.fft.rfft(_frames(x_hat + EPS, win, skip, T) * w, n_fft, axis=1))[:, :h]
        clean, proc = clean / clean.sum(axis=1, keepdims=True), proc / proc.sum(axis=1, keepdims=True)
        bank = critical_band_bank(sr, n_fft)
        ce, pe = clean @ bank.T, proc @ bank.T
        err = np.maximum((ce - pe) ** 2, EPS)
        wf = ce ** GAMMA
        fw = np.clip(np.sum(wf * (10.0 * np.log10(ce ** 2 / err)), axis=1) / np.sum(wf, axis=1), MIN_SNR, MAX_SNR)
    out.update(fwssnr=float(np.mean(fw)), ssnr=float(np.mean(ss)), fw_frames=fw, ss_frames=ss, clean_spec=clean, proc_spec=proc)
    return out


def segmental_snr(x_hat, x, sr: int) -> float:
    """SSNR of x_hat against x at rate sr in dB (the definition above; NumPy float64).  NaN for a clip shorter than win + skip."""
    return segsnr_detail(x_hat, x, sr)["ssnr"]


def fw_segmental_snr(x_hat, x, sr: int) -> float:
    """fwSSNR of x_hat against x at rate sr in dB (the definition above; NumPy float64).  NaN for a clip shorter than win + skip."""
    return segsnr_detail(x_hat, x, sr)["fwssnr"]


def tables(sr: int):
    """fd_segsnr_tables on the host (no GPU): -> ((win, skip, n_fft), window float64 [win], twiddle float32 [n_fft / 2][2], first int32
    [25], count int32 [25], weights float64 [sum of count])."""
    lib = L.load()
    dims = np.zeros(3, np.int32)
    nw = lib.fd_segsnr_tables(sr, dims.ctypes.data, None, None, None, None, None)
    L.check(min(nw, 0))
    win, skip, n_fft = (int(v) for v in dims)
    w, tw = np.zeros(win, np.float64), np.zeros((n_fft // 2, 2), np.float32)
    first, count, wgt = np.zeros(NUM_BANDS, np.int32), np.zeros(NUM_BANDS, np.int32), np.zeros(nw, np.float64)
    L.check(min(lib.fd_segsnr_tables(sr, None, w.ctypes.data, tw.ctypes.data, first.ctypes.data, count.ctypes.data, wgt.ctypes.data), 0))
    return (win, skip, n_fft), w, tw, first, count, wgt


class SegsnrPlan(L.Handle):
    """The device tables of fd_metrics_segsnr for one rate."""

    def __init__(self, sr):
        super().__init__("fd_segsnr_plan_destroy")
        self.sr = int(sr)
        self.win, self.skip, self.n_fft = frame_params(self.sr)
        L.check(L.load().fd_segsnr_plan_create(self.sr, C.byref(self.handle)))


def segsnr_plan(sr: int, device="cuda") -> SegsnrPlan:
    """The plan of one rate on one device, created on first use."""
    return L.cached_plan(device, ("segsnr", int(sr)), lambda: SegsnrPlan(sr))


def segsnr_batch(x_hats, xs, sr: int = 48000, batch: int = 8, device="cuda", return_frames: bool = False):
    """(fwSSNR, SSNR) of every (x_hat, x) on the GPU -> [n, 2] float64 (with return_frames also a list of [T_i, 2] arrays: the per-frame
    values).  Length-sorted ragged batches of `batch` clips; one cached plan per (sr, device).  A clip shorter than win + skip has no
    frame: NaN in its row."""
    lib = L.load()
    x_hats, xs = as_clips(x_hats, xs)
    plan = segsnr_plan(sr, device)
    out = np.zeros((len(xs), 2), np.float64)

    def call(rows, lens, idx, Lmax):
        B = len(idx)
        T = num_frames(Lmax, sr)
        nws = lib.fd_metrics_segsnr_workspace_bytes(plan.handle, B, Lmax)
        ws = torch.empty(nws, dtype=torch.uint8, device=device)
        val = torch.empty(B, 2, dtype=torch.float64, device=device)
        fr = torch.empty(B, max(T, 1), 2, dtype=torch.float64, device=device) if return_frames else None
        L.check(lib.fd_metrics_segsnr(plan.handle, L.ptr(rows[0]), L.ptr(rows[1]), L.ptr(lens), B, Lmax, L.ptr(val), L.ptr(fr), L.ptr(ws), nws,
                                      L.stream()))
        got = [val.cpu().numpy()]
        if return_frames:
            host, ln = fr.cpu().numpy(), lens.cpu().numpy()
            boxed = np.empty(B, object)
            for b in range(B):
                boxed[b] = host[b, :num_frames(int(ln[b]), sr)].copy()
            got.append(boxed)
        return got

    outs = [out]
    if return_frames:
        frames_out = np.empty(len(xs), object)
        outs.append(frames_out)
    ragged_batches((x_hats, xs), batch, device, call, outs)
    return (out, list(frames_out)) if return_frames else out
