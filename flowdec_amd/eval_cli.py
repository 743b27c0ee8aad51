"""Scores a triples list on the GPU: the enhance -> evaluate loop of the reference (enhance.py:142 writes `triples_list.txt`,
flowdec/eval/metrics.py get_metrics_df / get_metrics_df_parallel reads it) for those of its metrics that need no outside model or program.

    python -m flowdec_amd.eval_cli --triples out/triples_list.txt --out out/metrics.csv [--batch-files 8] [--crop-to-x] [--crop-to-x-hat]
                                   [--sr 48000] [--estoi] [--spectral] [--align MS [--align-frac] [--align-polarity] [--align-q 64]
                                   [--align-taps 32]] [--loudness] [--match-loudness] [--loudness-range] [--true-peak] [--ssnr]

Input: lines `clean ---> noisy ---> enhanced` (x, y, x_hat), split like enhance_cli's lists (audio.split_pair) (a comma inside an arrow line is part of the
path).  Every file is loaded like the reference's load48000 (util/other.py:137-): mean of the channels, resampled to --sr with
lowpass_filter_width=256 when its rate differs.  --crop-to-x then --crop-to-x-hat cut as in get_metrics_df (eval/metrics.py:85-90), in
that order.

Output: one CSV row per triple, in the list's order: name (the enhanced file's base name), x_hat, x, y, sisdr, sisir, sisar, logspec_mse
(the reference's metric names), and a last printed block with the mean of every metric over its finite rows.  The metrics run on the GPU
in length-sorted ragged batches of --batch-files triples (flowdec_amd/metrics.py: si_sxr_batch, logspec_mse_batch); a triple's numbers do
not depend on the batch it ran in.

A triple whose signals still differ in length after cropping gets NaN in all four columns and a warning (the reference gets there through
its exception handler); so does the spectral column of a triple too short for the transform's reflect padding.  A triple with a file that
cannot be read is skipped and counted, and the exit status is then 3 (enhance_cli's status of a partly done run), else 0.

--estoi (off by default; without it every byte of the output is what it was) adds a last CSV column `estoi` and a fifth summary line: the
reference's ESTOI (eval/metrics.py:273-283, pystoi.stoi(extended=True)) of x_hat against x, resampled to 10 kHz and scored on the GPU in the
same ragged batches (csrc/stoi.hip; flowdec_amd/metrics.py estoi_batch, host yardstick estoi).  A triple that leaves fewer than 30 spectral
frames after the silent frames are removed gets pystoi's value 1e-05 and a warning naming the rule.  pystoi itself is not available to the
tests: the host function is pinned against SciPy's resampler and the published algorithm, parity with the package is UNPINNED
(scripts/pin_estoi.py prints it where pystoi is importable).

--spectral (off by default; without it every byte of the output is what it was, with or without --estoi) adds two last CSV columns,
`msstft` and `mel` (after `estoi` when both switches are given), and two summary lines: the multi-scale STFT distance and the multi-scale
mel distance of x_hat against x -- the arithmetic of the reference's MultiScaleSTFTLoss and MelSpectrogramLoss (flowdec/losses.py) at their
default parameters, as metrics -- scored on the GPU in the same ragged batches (csrc/specdist.hip: a fused in-LDS FFT per frame pair;
flowdec_amd/specdist.py spectral_distances_batch, host yardsticks multiscale_stft_distance and mel_distance).  A triple of 2048 samples or
fewer cannot be reflect-padded for the 4096-sample window (the 2049-sample rule): NaN in those two columns and a warning.  The reference
builds its mel bank with torchaudio, which is not available to the tests: the bank is restated in float64 and pinned by its defining
properties, parity with the package is UNPINNED (scripts/pin_mel.py prints it where torchaudio is importable).

--align MS (off by default; without it every byte of the output is what it was, with any of the switches above) is for a row of the
comparison that does not come from this project's own chain -- a codec with look-ahead, a decoder that keeps or drops its priming samples,
a file cut a few milliseconds off -- where x_hat[n] and y[n] no longer belong to x[n] and a delay of a few samples costs SI-SDR tens of
dB.  With M = round(MS sr / 1000) samples (1 <= M <= 2^20, else a parser error), after loading and resampling and before the crop flags
(which then find nothing to cut and may be given too), every triple gets lag_x_hat = best_lag(x, x_hat, M) and lag_y = best_lag(x, y, M):
the lag of the peak of the bounded-lag cross-correlation c[l] = sum_n x[n] s[n + l], |l| <= M, in float64 (flowdec_amd/align.py: xcorr,
pick_lag; ties go to the smallest |l| and to +l), found on the GPU for all triples of the run in length-sorted ragged batches
(csrc/xcorr.hip; align.lags_batch, host yardstick align.host_lags).  The three signals are cut to their common support (align_triple) and
scored as above.  Two last CSV columns, `lag_x_hat` and `lag_y` (after `mel` / `estoi` when those are on): integers in samples at --sr,
positive = late; two summary lines with the minimum, the maximum and the count of non-zero lags.  A lag equal to +-M gets a warning (the
peak sits at the edge of the search; the triple is still scored); a triple whose common support is empty gets NaN in every metric and a
warning.

--align-frac and --align-polarity (each needs --align MS; without them every byte of the output is what --align MS alone writes) are for a
codec with a resampler in its path, whose delay is no whole number of samples, and for one that inverts the polarity.  --align-frac finds
each delay on a grid of 1 / Q samples (--align-q, default 64): the peak of the correlation interpolated by a Hann-windowed sinc of 2 W
taps (--align-taps W, default 32) around its integer peak (align.refine_lag; csrc/xcorr.hip fd_xcorr_lags_frac), and reads x_hat and y
that much later through the same interpolator (align.frac_shift; csrc/fracshift.hip), cut to the samples for which no tap leaves the file
(align.support_frac).  `lag_x_hat` and `lag_y` then print lag_q / Q in full (an exact binary fraction for the default Q).  A signal whose
delay is a whole number of samples is cut as --align cuts it, so such a triple scores the same bits.  --align-polarity picks the peak of
|c| and multiplies a signal whose peak is negative by -1 before it is scored: two further last columns `pol_x_hat`, `pol_y` (1 or -1)
and a summary line with the count of inverted signals.  No drift.

--loudness and --match-loudness (off by default; without them every byte of the output is what it was, with any of the switches above)
are for a row that plays at another level: of the seven metrics only the SI-SxR three are scale-invariant.  --loudness measures the
integrated loudness of ITU-R BS.1770-4 / EBU R 128 (K-weighting, 400 ms blocks, the absolute and the relative gate; mono) of x_hat, x and
y as they are scored -- after alignment and cropping -- on the GPU for all triples of the run in length-sorted ragged batches
(csrc/loudness.hip; flowdec_amd/loudness.py loudness_batch, host yardstick integrated_loudness): three CSV columns `lufs_x_hat`, `lufs_x`,
`lufs_y` after `mel` / `estoi` when those are on and before the `lag_*` / `pol_*` columns, and three summary lines.  A signal shorter
than 400 ms reads nan, a silent one -inf.  The measure is defined at 48 kHz: at another --sr the signals are resampled to 48 kHz for the
measurement only.  --match-loudness implies --loudness and then multiplies x_hat and y by the one float32 factor each that brings them
to x's loudness (loudness.match_loudness) before every metric; the three columns report the loudness before matching.  A signal whose
loudness, or whose reference's, is nan or -inf is left as it is, with a warning.  The coefficients and the conformance readings of the
standard pin the host function; parity with the pyloudnorm package is UNPINNED (scripts/pin_loudness.py).

--loudness-range and --true-peak (off by default; without them every byte of the output is what it was, with any of the switches above)
complete the level report after EBU R 128: did the enhancer flatten or inflate the dynamics, and do the files overshoot between samples.
--loudness-range adds three columns `lra_x_hat`, `lra_x`, `lra_y` (loudness range after EBU Tech 3342, in LU: the spread between the 10th
and the 95th percentile of the gated 3 s loudness; nan under 3 s), --true-peak three columns `dbtp_x_hat`, `dbtp_x`, `dbtp_y` (the true
peak of BS.1770-4 Annex 2 in dBTP, read through the project's own 4x Hann-windowed-sinc interpolator of 24 taps per phase, not the
standard's example filter).  Both stand behind the `lufs_*` columns (when those are on) and before the `lag_*` / `pol_*` columns, each
with three summary lines, and both measure the signals as they are scored -- after --align and the crops -- and before --match-loudness
scales, as `lufs_*` does (csrc/loudness_range.hip; loudness.py loudness_range_batch and true_peak_batch, host yardsticks loudness_range
and true_peak).

--ssnr (off by default; without it every byte of the output is what it was, with any of the switches above) adds two CSV columns,
`fwSSNR` and `SSNR` -- the reference's names for the frequency-weighted segmental SNR and the segmental SNR it takes from the pysepm package
(eval/metrics.py:511-547: fwSNRseg and SNRseg with 30 ms frames at 75 % overlap; Hu & Loizou's comp_fwseg.m / comp_snr.m), in the order of
its default list -- after `estoi` / `msstft` / `mel` when those are on and before the `lufs_*`, `lag_*` and `pol_*` columns, and two
summary lines.  Scored on the GPU in the same ragged batches (csrc/segsnr.hip: one fused kernel per frame pair, a float32 FFT in LDS and
float64 band arithmetic; flowdec_amd/segsnr.py segsnr_batch, host yardsticks fw_segmental_snr and segmental_snr), on the signals as every
other metric that is not scale-invariant sees them: after --align and --match-loudness.  Both drop the last frame, so a triple shorter
than win + skip = round(0.03 sr) + floor(0.0075 sr) samples has none: NaN in those two columns and a warning.  pysepm is not available to
the tests: the host functions are pinned against a transcription through scipy.signal.stft and the published algorithm, parity with the
package is UNPINNED (scripts/pin_segsnr.py prints it where pysepm is importable).

The reference's other metrics (PESQ, DNSMOS, SIGMOS, ViSQOL) need outside programs or models: out of scope.
"""
import argparse
import csv
import math
import os
import sys
from dataclasses import InitVar, dataclass, field, fields
from typing import Callable, List, Optional

import numpy as np
import torch

from . import align, loudness, metrics, segsnr, specdist
from .audio import RESAMPLE_HELP, load_mono, split_pair

METRIC_NAMES = ("sisdr", "sisir", "sisar", "logspec_mse")
CSV_HEADER = ("name", "x_hat", "x", "y") + METRIC_NAMES
ESTOI_NAME = "estoi"                # the optional fifth metric (--estoi), the last column without --spectral
SPECTRAL_NAMES = specdist.NAMES     # the optional metrics of --spectral (msstft, mel), always the last two columns
SSNR_NAMES = segsnr.NAMES          # the optional metrics of --ssnr (fwSSNR, SSNR), behind every other metric column
LAG_NAMES = ("lag_x_hat", "lag_y")  # the optional columns of --align, always the last two (before POL_NAMES)
POL_NAMES = ("pol_x_hat", "pol_y")  # the optional columns of --align-polarity, always the last two
LUFS_NAMES = ("lufs_x_hat", "lufs_x", "lufs_y")  # the optional columns of --loudness, behind the metrics and before LAG_NAMES
LRA_NAMES = ("lra_x_hat", "lra_x", "lra_y")     # the optional columns of --loudness-range, behind LUFS_NAMES and before LAG_NAMES
DBTP_NAMES = ("dbtp_x_hat", "dbtp_x", "dbtp_y")  # the optional columns of --true-peak, behind LRA_NAMES and before LAG_NAMES
WIN_DUR, HOP_DUR = 32e-3, 8e-3      # LogSpecMSE (eval/metrics.py:333-372)


@dataclass
class Triple:
    x: str          # clean
    y: str          # noisy
    x_hat: str      # enhanced

    @property
    def name(self) -> str:
        return os.path.basename(self.x_hat)


def read_triples(listfile: str) -> List[Triple]:
    """`clean ---> noisy ---> enhanced` per line; blank lines are skipped; any other field count is a ValueError naming the line."""
    out = []
    with open(listfile, "r") as f:
        for lineno, raw in enumerate(f, 1):
            entry = raw.strip()
            if not entry:
                continue
            parts = [p.strip() for p in split_pair(entry)]
            if len(parts) != 3:
                raise ValueError(f"{listfile}:{lineno}: {len(parts)} fields, a triples line is `clean ---> noisy ---> enhanced`")
            out.append(Triple(parts[0], parts[1], parts[2]))
    return out


def crop(x_hat: torch.Tensor, x: torch.Tensor, y: torch.Tensor, crop_to_x: bool, crop_to_x_hat: bool):
    """get_metrics_df's crops (eval/metrics.py:85-90), in its order."""
    if crop_to_x:
        x_hat, y = x_hat[..., :x.shape[-1]], y[..., :x.shape[-1]]
    if crop_to_x_hat:
        x, y = x[..., :x_hat.shape[-1]], y[..., :x_hat.shape[-1]]
    return x_hat, x, y


def min_spectral_samples(sr: int) -> int:
    """Shortest clip the spectral metric takes: reflect padding by n_fft / 2 needs one sample more."""
    return int(WIN_DUR * sr) // 2 + 1


@dataclass(frozen=True)
class Scorer:
    """si_sxr(x_hats, xs, ys, batch) -> [n, 3] (si_sdr, si_sir, si_sar); logspec(x_hats, xs, sr, batch) -> [n]; estoi(x_hats, xs, sr,
    batch) -> [n] (optional: only --estoi calls it); spectral(x_hats, xs, sr, batch) -> [n, 2] (msstft, mel) (optional: only --spectral
    calls it); align(as_, bs, max_lag, batch) -> int64 [n], the lag of each b against its a (optional: only --align calls it);
    align_frac(as_, bs, max_lag, Q, W, polarity, batch) -> (lag_q int64 [n], sign int32 [n]) and shift(signals, lag_q, sign, windows, Q, W,
    batch) -> float32 tensors (optional: only --align-frac / --align-polarity call them); loudness(signals, sr, batch) -> float64 [n] in
    LUFS (optional: only --loudness / --match-loudness call it); segsnr(x_hats, xs, sr, batch) -> [n, 2] (fwSSNR, SSNR) (optional: only --ssnr
    calls it); loudness_range(signals, sr, batch) -> float64 [n] in LU (optional: only --loudness-range calls it); true_peak(signals, sr,
    batch) -> float64 [n] in dBTP (optional: only --true-peak calls it).
    The last two are constructor arguments and attributes like the others but NOT dataclass fields: `dataclasses.fields(Scorer)` stays the
    list it was, ending with segsnr.  Equality, the hash's consistency with it and the repr take them in through the methods below;
    `dataclasses.replace` does not know them and would hand back a Scorer without them: use `Scorer.replace`, which carries them over."""
    si_sxr: Callable
    logspec: Callable
    estoi: Optional[Callable] = None
    spectral: Optional[Callable] = None
    align: Optional[Callable] = None
    align_frac: Optional[Callable] = None
    shift: Optional[Callable] = None
    loudness: Optional[Callable] = None
    segsnr: Optional[Callable] = None
    # the two functions of the level report: constructor arguments (appended, default None) and attributes like the others, but not
    # dataclass fields -- dataclasses.fields(Scorer) stays the list of the scoring functions it was, ending with segsnr
    loudness_range: InitVar[Optional[Callable]] = None
    true_peak: InitVar[Optional[Callable]] = None

    def __post_init__(self, loudness_range, true_peak):
        object.__setattr__(self, "loudness_range", loudness_range)
        object.__setattr__(self, "true_peak", true_peak)

    def _all(self) -> tuple:
        return tuple(getattr(self, f.name) for f in fields(self)) + (self.loudness_range, self.true_peak)

    def replace(self, **changes) -> "Scorer":
        """A copy with the named functions changed, the two level functions included."""
        names = [f.name for f in fields(self)] + ["loudness_range", "true_peak"]
        return Scorer(**{**dict(zip(names, self._all())), **changes})

    def __eq__(self, other):
        return self._all() == other._all() if other.__class__ is self.__class__ else NotImplemented

    def __hash__(self):
        return hash(self._all())

    def __repr__(self):
        names = [f.name for f in fields(self)] + ["loudness_range", "true_peak"]
        return "Scorer(" + ", ".join(f"{n}={v!r}" for n, v in zip(names, self._all())) + ")"


def _gpu_si_sxr(x_hats, xs, ys, batch):
    return metrics.si_sxr_batch(x_hats, xs, ys, batch=batch)


def _gpu_logspec(x_hats, xs, sr, batch):
    return metrics.logspec_mse_batch(x_hats, xs, sr=sr, win_dur=WIN_DUR, hop_dur=HOP_DUR, batch=batch)


def _host_si_sxr(x_hats, xs, ys, batch):
    return np.array([metrics.si_sxr(h, x, y) for h, x, y in zip(x_hats, xs, ys)], np.float64).reshape(-1, 3)


def _host_logspec(x_hats, xs, sr, batch):
    return np.array([metrics.logspec_mse(h, x, sr=sr, win_dur=WIN_DUR, hop_dur=HOP_DUR) for h, x in zip(x_hats, xs)], np.float64)


def _gpu_estoi(x_hats, xs, sr, batch):
    return metrics.estoi_batch(x_hats, xs, sr=sr, batch=batch)


def _host_estoi(x_hats, xs, sr, batch):
    return np.array([metrics.estoi(h, x, sr) for h, x in zip(x_hats, xs)], np.float64)


def _gpu_spectral(x_hats, xs, sr, batch):
    return specdist.spectral_distances_batch(x_hats, xs, sr=sr, batch=batch)


def _host_spectral(x_hats, xs, sr, batch):
    return np.array([(specdist.multiscale_stft_distance(h, x), specdist.mel_distance(h, x, sr)) for h, x in zip(x_hats, xs)], np.float64).reshape(-1, 2)


def _gpu_loudness(signals, sr, batch):
    return loudness.loudness_batch(signals, sr=sr, batch=batch)


def _gpu_loudness_range(signals, sr, batch):
    return loudness.loudness_range_batch(signals, sr=sr, batch=batch)


def _gpu_true_peak(signals, sr, batch):
    return loudness.true_peak_batch(signals, sr=sr, batch=batch)


def _gpu_segsnr(x_hats, xs, sr, batch):
    return segsnr.segsnr_batch(x_hats, xs, sr=sr, batch=batch)


def _host_segsnr(x_hats, xs, sr, batch):
    details = [segsnr.segsnr_detail(h, x, sr) for h, x in zip(x_hats, xs)]
    return np.array([(d["fwssnr"], d["ssnr"]) for d in details], np.float64).reshape(-1, 2)


# ragged batches on the device (csrc/loudness.hip, csrc/metrics.hip, csrc/stoi.hip, csrc/specdist.hip, csrc/segsnr.hip, csrc/xcorr.hip)
GPU_SCORER = Scorer(_gpu_si_sxr, _gpu_logspec, _gpu_estoi, _gpu_spectral, align.lags_batch, align.lags_batch_frac, align.shift_batch,
                    _gpu_loudness, _gpu_segsnr, _gpu_loudness_range, _gpu_true_peak)
# the host functions of metrics.py, specdist.py, segsnr.py and align.py, one triple at a time: the yardstick
HOST_SCORER = Scorer(_host_si_sxr, _host_logspec, _host_estoi, _host_spectral, align.host_lags, align.host_lags_frac, align.host_shift,
                     loudness.host_loudness, _host_segsnr, loudness.host_loudness_range, loudness.host_true_peak)


def metric_columns(estoi: bool = False, spectral: bool = False, ssnr: bool = False) -> tuple:
    """The names of the value columns, in order: the four metrics, then estoi, then msstft and mel, then fwSSNR and SSNR."""
    return METRIC_NAMES + ((ESTOI_NAME,) if estoi else ()) + (SPECTRAL_NAMES if spectral else ()) + (SSNR_NAMES if ssnr else ())


def score(signals, sr: int, batch: int, scorer: Scorer = GPU_SCORER, names: Optional[List[str]] = None, estoi: bool = False,
          spectral: bool = False, ssnr: bool = False) -> np.ndarray:
    """signals: one (x_hat, x, y) of 1-D tensors per triple, cropped -> [n, 4] float64 in METRIC_NAMES order, row i for triple i whatever
    order the batches ran in.  Unequal lengths: NaN in all four; too short for the transform: NaN in the spectral column.
    estoi=True: [n, 5], the last column ESTOI (1e-5 and a warning under the 30-frame rule; NaN with the others for unequal lengths).
    spectral=True: two more last columns, msstft and mel (metric_columns gives the layout); NaN and a warning for a triple under the
    2049-sample rule, NaN with the others for unequal lengths.
    ssnr=True: two more last columns, fwSSNR and SSNR; NaN and a warning for a triple shorter than win + skip, NaN with the others for
    unequal lengths."""
    def warn(i, msg):
        print(f"warning: {names[i] if names else 'triple %d' % i}: {msg}", file=sys.stderr)

    def column(idx, k):
        return [signals[i][k] for i in idx]

    out = np.full((len(signals), len(metric_columns(estoi, spectral, ssnr))), np.nan, np.float64)
    n_spec = len(METRIC_NAMES) + (1 if estoi else 0) + (len(SPECTRAL_NAMES) if spectral else 0)     # the columns before fwSSNR
    ok = []
    for i, (h, x, y) in enumerate(signals):
        if not (h.shape[-1] == x.shape[-1] == y.shape[-1]):
            warn(i, f"lengths differ (x_hat {h.shape[-1]}, x {x.shape[-1]}, y {y.shape[-1]}): NaN for every metric "
                    f"(--crop-to-x / --crop-to-x-hat cut them to one length)")
        elif x.shape[-1] < 1:
            warn(i, "empty signals: NaN for every metric")
        else:
            ok.append(i)
    framed = [i for i in ok if signals[i][1].shape[-1] >= min_spectral_samples(sr)]
    for i in sorted(set(ok) - set(framed)):
        warn(i, f"{signals[i][1].shape[-1]} samples are too few for the spectral metric (needs {min_spectral_samples(sr)}): NaN for logspec_mse")
    if ok:
        out[ok, :3] = scorer.si_sxr(column(ok, 0), column(ok, 1), column(ok, 2), batch)
    if framed:
        out[framed, 3] = scorer.logspec(column(framed, 0), column(framed, 1), sr, batch)
    if estoi and ok:
        if scorer.estoi is None:
            raise ValueError("score: estoi=True needs a Scorer with an estoi function")
        out[ok, 4] = scorer.estoi(column(ok, 0), column(ok, 1), sr, batch)
        for i in ok:
            if out[i, 4] == metrics.ESTOI_TOO_SHORT:
                warn(i, metrics.ESTOI_SHORT_RULE)
    if spectral:
        if scorer.spectral is None:
            raise ValueError("score: spectral=True needs a Scorer with a spectral function")
        long_enough = [i for i in ok if signals[i][1].shape[-1] >= specdist.MIN_SAMPLES]
        for i in sorted(set(ok) - set(long_enough)):
            warn(i, f"{signals[i][1].shape[-1]} samples: {specdist.SHORT_RULE}")
        if long_enough:
            out[long_enough, n_spec - 2:n_spec] = scorer.spectral(column(long_enough, 0), column(long_enough, 1), sr, batch)
    if ssnr:
        if scorer.segsnr is None:
            raise ValueError("score: ssnr=True needs a Scorer with a segsnr function")
        with_frame = [i for i in ok if signals[i][1].shape[-1] >= segsnr.min_samples(sr)]
        for i in sorted(set(ok) - set(with_frame)):
            warn(i, f"{signals[i][1].shape[-1]} samples: {segsnr.short_rule(sr)}")
        if with_frame:
            out[with_frame, n_spec:] = scorer.segsnr(column(with_frame, 0), column(with_frame, 1), sr, batch)
    return out


def fmt(v: float) -> str:
    return "nan" if math.isnan(v) else repr(float(v))


def _columns_of(values: np.ndarray, columns) -> tuple:
    """columns=None: the four metrics, and estoi for [n, 5] values; else the caller's names (metric_columns), one per column of values."""
    if columns is None:
        return METRIC_NAMES + ((ESTOI_NAME,) if values.ndim == 2 and values.shape[1] == len(METRIC_NAMES) + 1 else ())
    if values.ndim != 2 or values.shape[1] != len(columns):
        raise ValueError(f"eval: {len(columns)} column names for values of shape {values.shape}")
    return tuple(columns)


def write_csv(path: str, triples: List[Triple], values: np.ndarray, columns=None, lags=None, lag_q=None, Q: int = 1, pols=None, lufs=None, lra=None,
              dbtp=None) -> None:
    """lags (--align): int [n, 2], written as the two last columns LAG_NAMES.  lag_q (--align-frac) instead: int [n, 2] in units of 1 / Q
    sample, written as lag_q / Q.  pols (--align-polarity): int [n, 2] of 1 / -1, written behind them as POL_NAMES.  lufs
    (--loudness): float64 [n, 3], written as LUFS_NAMES behind the metrics and before all of those (nan and -inf as `fmt` prints them);
    lra (--loudness-range) and dbtp (--true-peak): float64 [n, 3] each, written as LRA_NAMES and DBTP_NAMES behind LUFS_NAMES."""
    level = [(names, v) for names, v in ((LUFS_NAMES, lufs), (LRA_NAMES, lra), (DBTP_NAMES, dbtp)) if v is not None]
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(CSV_HEADER[:4] + _columns_of(values, columns) + tuple(c for names, _ in level for c in names) + (LAG_NAMES if lags is not None or lag_q is not None else ())
                   + (POL_NAMES if pols is not None else ()))
        for i, (t, row) in enumerate(zip(triples, values)):
            w.writerow([t.name, t.x_hat, t.x, t.y] + [fmt(v) for v in row] + [fmt(v) for _, lv in level for v in lv[i]] + ([str(int(l)) for l in lags[i]] if lags is not None else [])
                       + ([align.lag_text(l, Q) for l in lag_q[i]] if lag_q is not None else []) + ([str(int(g)) for g in pols[i]] if pols is not None else []))


def summary(values: np.ndarray, columns=None):
    """-> [(metric, mean over its finite rows or NaN, count of finite rows)]; five entries for the [n, 5] values of --estoi; with
    columns= (metric_columns) one entry per name."""
    out = []
    for k, name in enumerate(_columns_of(values, columns)):
        col = values[:, k] if len(values) else np.zeros(0)
        fin = col[np.isfinite(col)]
        out.append((name, float(fin.mean()) if len(fin) else float("nan"), int(len(fin))))
    return out


@dataclass
class EvalResult:
    n_triples: int = 0
    n_scored: int = 0          # rows written (NaN rows included)
    n_unreadable: int = 0      # triples skipped: a file could not be read
    means: list = field(default_factory=list)
    csv_path: Optional[str] = None
    lags: list = field(default_factory=list)   # --align: [(column, min, max, count of non-zero lags)], empty without it
    inverted: list = field(default_factory=list)   # --align-polarity: [(column, count of inverted signals)], empty without it
    loudness: list = field(default_factory=list)   # --loudness: [(column, mean over its finite rows, count of finite rows)], empty without it
    loudness_range: list = field(default_factory=list)   # --loudness-range: the same for LRA_NAMES
    true_peak: list = field(default_factory=list)        # --true-peak: the same for DBTP_NAMES

    @property
    def exit_code(self) -> int:
        return 3 if self.n_unreadable else 0


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Score a triples list (clean ---> noisy ---> enhanced) on MI355X: SI-SDR / SI-SIR / SI-SAR and LogSpecMSE")
    p.add_argument("--triples", type=str, required=True, help="the triples_list.txt of an enhance_cli run on a pair list")
    p.add_argument("--out", type=str, required=True, help="the CSV to write")
    p.add_argument("--batch-files", type=int, default=8, help="triples per native call (length-sorted ragged batches)")
    p.add_argument("--crop-to-x", action="store_true", help="cut x_hat and y to the length of x (eval/metrics.py:85-87)")
    p.add_argument("--crop-to-x-hat", action="store_true", help="then cut x and y to the length of x_hat (eval/metrics.py:88-90)")
    p.add_argument("--sr", type=int, default=48000, help="the rate every file is brought to (the reference evaluates at 48 kHz)")
    p.add_argument("--resample", type=str, default="host", choices=["host", "device"], help=RESAMPLE_HELP)
    p.add_argument("--estoi", action="store_true",
                   help="also score ESTOI (pystoi.stoi(extended=True) restated; 10 kHz, on the GPU): a last CSV column `estoi` and a fifth mean")
    p.add_argument("--spectral", action="store_true",
                   help="also score the multi-scale STFT and mel distances (the reference's MultiScaleSTFTLoss / MelSpectrogramLoss as metrics; on "
                        "the GPU): two last CSV columns `msstft` and `mel` and two more means")
    p.add_argument("--align", type=float, default=None, metavar="MS",
                   help="before scoring, find the delay of x_hat and of y against x within +-MS milliseconds (peak of the cross-correlation, on "
                        "the GPU) and cut the three signals to their common support: two last CSV columns `lag_x_hat` and `lag_y` in samples "
                        "at --sr (positive = late)")
    p.add_argument("--align-frac", action="store_true",
                   help="with --align MS: find the delays on a grid of 1 / Q samples and read x_hat and y through a windowed-sinc interpolator "
                        "(on the GPU); `lag_x_hat` and `lag_y` then print fractions of a sample")
    p.add_argument("--align-polarity", action="store_true",
                   help="with --align MS: pick the peak of |c| and undo an inverted polarity before scoring: two further last CSV columns "
                        "`pol_x_hat` and `pol_y` (1 or -1)")
    p.add_argument("--loudness", action="store_true",
                   help="also measure the integrated loudness (ITU-R BS.1770-4 / EBU R 128, mono; on the GPU) of x_hat, x and y as they are "
                        "scored: three CSV columns `lufs_x_hat`, `lufs_x`, `lufs_y` behind the metrics and three more means")
    p.add_argument("--match-loudness", action="store_true",
                   help="implies --loudness: scale x_hat and y to the loudness of x (one float32 factor each) before every metric; the three "
                        "columns report the loudness before matching")
    p.add_argument("--loudness-range", action="store_true",
                   help="also measure the loudness range (EBU Tech 3342; on the GPU) of x_hat, x and y as they are scored, before "
                        "--match-loudness scales: three CSV columns `lra_x_hat`, `lra_x`, `lra_y` behind the `lufs_*` columns and three more "
                        "means (nan under 3 s)")
    p.add_argument("--true-peak", action="store_true",
                   help="also measure the true peak (ITU-R BS.1770-4 Annex 2 with the project's 4x windowed-sinc interpolator; on the GPU) of "
                        "x_hat, x and y as they are scored, before --match-loudness scales: three CSV columns `dbtp_x_hat`, `dbtp_x`, "
                        "`dbtp_y` behind the `lufs_*` / `lra_*` columns and three more means")
    p.add_argument("--ssnr", action="store_true",
                   help="also score the frequency-weighted segmental SNR and the segmental SNR (pysepm's fwSNRseg / SNRseg restated; on the "
                        "GPU): two CSV columns `fwSSNR` and `SSNR` behind the other metrics and two more means")
    p.add_argument("--align-q", type=int, default=align.FRAC_Q, metavar="Q", help="--align-frac: grid steps per sample (2 to 1024)")
    p.add_argument("--align-taps", type=int, default=align.FRAC_W, metavar="W", help="--align-frac: the interpolator has 2 W taps (W from 1 to 256)")
    return p


def check_align_args(parser, args) -> None:
    """--align-frac / --align-polarity need --align MS; --align-q and --align-taps stay inside what the kernels take."""
    if (args.align_frac or args.align_polarity) and args.align is None:
        parser.error("--align-frac and --align-polarity need --align MS")
    if not 2 <= args.align_q <= align.MAX_Q or not 1 <= args.align_taps <= align.MAX_W:
        parser.error(f"--align-q takes 2 to {align.MAX_Q} and --align-taps 1 to {align.MAX_W}")


def align_max_lag(ms: float, sr: int) -> int:
    """--align MS at rate sr -> M = round(MS sr / 1000) samples; ValueError outside [1, 2^20]."""
    if not math.isfinite(ms):
        raise ValueError(f"--align {ms}: not a number of milliseconds")
    M = int(round(ms * sr / 1000.0))
    if M < 1 or M > align.MAX_LAG_CAP:
        raise ValueError(f"--align {ms:g} ms is {M} samples at {sr} Hz: the search takes 1 to {align.MAX_LAG_CAP} samples")
    return M


def align_signals(loaded, M: int, batch: int, scorer: Scorer, names: Optional[List[str]] = None):
    """loaded: one (x_hat, x, y) of 1-D tensors per triple, as read -> (the triples cut to their common support: views, int64 [n, 2] =
    lag_x_hat, lag_y).  All lags come from ONE call of scorer.align.  |lag| = M: a warning; an empty support: a warning (and NaN later)."""
    if scorer.align is None:
        raise ValueError("align_signals: --align needs a Scorer with an align function")
    n = len(loaded)
    lags = np.zeros((n, 2), np.int64)
    if n:
        xs = [x for _, x, _ in loaded]
        got = np.asarray(scorer.align(xs + xs, [h for h, _, _ in loaded] + [y for _, _, y in loaded], M, batch), np.int64).reshape(-1)
        lags[:, 0], lags[:, 1] = got[:n], got[n:]
    out = []
    for i, (h, x, y) in enumerate(loaded):
        who = names[i] if names else "triple %d" % i
        for k, col in enumerate(LAG_NAMES):
            if abs(int(lags[i, k])) == M:
                print(f"warning: {who}: {col} = {int(lags[i, k])} is at the edge of the search (+-{M} samples): the true delay may lie "
                      f"outside it (a larger --align)", file=sys.stderr)
        cut = align.align_triple(h, x, y, int(lags[i, 0]), int(lags[i, 1]))
        if cut[1].shape[-1] < 1:
            print(f"warning: {who}: the common support of the aligned signals is empty (lag_x_hat {int(lags[i, 0])}, lag_y {int(lags[i, 1])}; "
                  f"x_hat {h.shape[-1]}, x {x.shape[-1]}, y {y.shape[-1]} samples): NaN for every metric", file=sys.stderr)
        out.append(cut)
    return out, lags


def align_signals_frac(loaded, M: int, batch: int, scorer: Scorer, frac: bool, polarity: bool, Q: int, W: int, names: Optional[List[str]] = None):
    """align_signals for --align-frac / --align-polarity -> (the triples on their common support, lag_q int64 [n, 2] in units of 1 / Q
    sample, sign int32 [n, 2]).  All lags come from ONE call of scorer.align_frac (or scorer.align, for whole samples with polarity), all
    signals that are not cut as views from ONE call of scorer.shift."""
    if scorer.align is None or scorer.align_frac is None or scorer.shift is None:
        raise ValueError("align_signals_frac: --align-frac / --align-polarity need a Scorer with align, align_frac and shift functions")
    n = len(loaded)
    xs = [x for _, x, _ in loaded]
    got_q, got_s = align.find_lags(xs + xs, [h for h, _, _ in loaded] + [y for _, _, y in loaded], M, frac, polarity, Q, W, batch, scorer.align,
                                   scorer.align_frac)
    lag_q, sign = np.stack([got_q[:n], got_q[n:]], axis=1).reshape(n, 2), np.stack([got_s[:n], got_s[n:]], axis=1).reshape(n, 2)
    windows = []
    for i, (h, x, y) in enumerate(loaded):
        who = names[i] if names else "triple %d" % i
        for k, col in enumerate(LAG_NAMES):
            if abs(int(lag_q[i, k])) == M * Q:
                print(f"warning: {who}: {col} = {align.lag_text(lag_q[i, k], Q)} is at the edge of the search (+-{M} samples): the true delay may "
                      f"lie outside it (a larger --align)", file=sys.stderr)
        n0, n1 = align.common_support_frac(x.shape[-1], (h.shape[-1], y.shape[-1]), lag_q[i], Q, W)
        if n1 <= n0:
            print(f"warning: {who}: the common support of the aligned signals is empty (lag_x_hat {align.lag_text(lag_q[i, 0], Q)}, lag_y "
                  f"{align.lag_text(lag_q[i, 1], Q)}; x_hat {h.shape[-1]}, x {x.shape[-1]}, y {y.shape[-1]} samples): NaN for every metric", file=sys.stderr)
        windows.append((n0, max(n1, n0)))
    cut = align.cut_frac([h for h, _, _ in loaded] + [y for _, _, y in loaded], np.concatenate([lag_q[:, 0], lag_q[:, 1]]),
                         np.concatenate([sign[:, 0], sign[:, 1]]), windows + windows, Q, W, scorer.shift, batch)
    return [(cut[i], x[..., n0:n1], cut[n + i]) for i, ((_, x, _), (n0, n1)) in enumerate(zip(loaded, windows))], lag_q, sign


def _measure_level(fn, signals, sr: int, batch: int) -> np.ndarray:
    loudness.check_rate(sr)
    n = len(signals)
    if not n:
        return np.zeros((0, 3), np.float64)
    got = np.asarray(fn([s[k] for k in range(3) for s in signals], sr, batch), np.float64).reshape(3, n)
    return np.ascontiguousarray(got.T)


def measure_loudness(signals, sr: int, batch: int, scorer: Scorer) -> np.ndarray:
    """signals: one (x_hat, x, y) of 1-D tensors per triple, as they will be scored -> float64 [n, 3] LUFS in LUFS_NAMES order, from ONE
    call of scorer.loudness."""
    if scorer.loudness is None:
        raise ValueError("measure_loudness: --loudness / --match-loudness need a Scorer with a loudness function")
    return _measure_level(scorer.loudness, signals, sr, batch)


def measure_loudness_range(signals, sr: int, batch: int, scorer: Scorer) -> np.ndarray:
    """measure_loudness for --loudness-range: float64 [n, 3] LU in LRA_NAMES order, from ONE call of scorer.loudness_range."""
    if scorer.loudness_range is None:
        raise ValueError("measure_loudness_range: --loudness-range needs a Scorer with a loudness_range function")
    return _measure_level(scorer.loudness_range, signals, sr, batch)


def measure_true_peak(signals, sr: int, batch: int, scorer: Scorer) -> np.ndarray:
    """measure_loudness for --true-peak: float64 [n, 3] dBTP in DBTP_NAMES order, from ONE call of scorer.true_peak."""
    if scorer.true_peak is None:
        raise ValueError("measure_true_peak: --true-peak needs a Scorer with a true_peak function")
    return _measure_level(scorer.true_peak, signals, sr, batch)


def match_signals(signals, lufs: np.ndarray, names: Optional[List[str]] = None):
    """--match-loudness: x_hat and y of every triple times the float32 factor that brings them to x's loudness (loudness.match_loudness).
    A signal whose loudness, or whose reference's, is not finite stays as it is, with a warning naming the triple."""
    out = []
    for i, (h, x, y) in enumerate(signals):
        who = names[i] if names else "triple %d" % i
        scaled = []
        for sig, k in ((h, 0), (y, 2)):
            if math.isfinite(lufs[i, k]) and math.isfinite(lufs[i, 1]):
                scaled.append(loudness.match_loudness(sig, lufs[i, k], lufs[i, 1]))
            else:
                print(f"warning: {who}: {LUFS_NAMES[k]} = {fmt(lufs[i, k])}, {LUFS_NAMES[1]} = {fmt(lufs[i, 1])}: no loudness to match "
                      f"(under 400 ms, silent or not finite); {'x_hat' if k == 0 else 'y'} is scored as it is", file=sys.stderr)
                scaled.append(sig)
        out.append((scaled[0], x, scaled[1]))
    return out


def lag_summary_frac(lag_q: np.ndarray, Q: int):
    """lag_summary of lag_q / Q: the minimum and the maximum as the text the CSV holds."""
    return [(name, align.lag_text(lag_q[:, k].min(), Q) if len(lag_q) else "0", align.lag_text(lag_q[:, k].max(), Q) if len(lag_q) else "0",
             int(np.count_nonzero(lag_q[:, k]))) for k, name in enumerate(LAG_NAMES)]


def lag_summary(lags: np.ndarray):
    """-> [(column, min, max, count of non-zero lags)] of int [n, 2] lags; 0, 0, 0 for no rows."""
    return [(name, int(lags[:, k].min()) if len(lags) else 0, int(lags[:, k].max()) if len(lags) else 0, int(np.count_nonzero(lags[:, k])))
            for k, name in enumerate(LAG_NAMES)]


def run(argv=None, scorer: Scorer = GPU_SCORER) -> EvalResult:
    parser = build_parser()
    args = parser.parse_args(list(sys.argv[1:] if argv is None else argv))
    max_lag = None
    if args.align is not None:
        try:
            max_lag = align_max_lag(args.align, args.sr)
        except ValueError as err:
            parser.error(str(err))
    check_align_args(parser, args)
    if args.loudness or args.match_loudness or args.loudness_range or args.true_peak:
        try:
            loudness.check_rate(args.sr)
        except ValueError as err:
            parser.error(str(err))
    triples = read_triples(args.triples)
    res = EvalResult(n_triples=len(triples), csv_path=args.out)
    kept, signals = [], []
    for t in triples:
        try:
            x_hat, x, y = (load_mono(f, args.sr, args.resample) for f in (t.x_hat, t.x, t.y))
        except Exception as err:      # a missing or broken file: the reference skips the triple too (eval/metrics.py:95-96)
            print(f"warning: skipping {t.name}: {type(err).__name__}: {err}", file=sys.stderr)
            res.n_unreadable += 1
            continue
        kept.append(t)
        signals.append((x_hat, x, y))
    names, lags, lag_q, sign = [t.name for t in kept], None, None, None
    if max_lag is not None and (args.align_frac or args.align_polarity):
        signals, lag_q, sign = align_signals_frac(signals, max_lag, args.batch_files, scorer, args.align_frac, args.align_polarity, args.align_q,
                                                  args.align_taps, names=names)
    elif max_lag is not None:
        signals, lags = align_signals(signals, max_lag, args.batch_files, scorer, names=names)
    signals = [crop(x_hat, x, y, args.crop_to_x, args.crop_to_x_hat) for x_hat, x, y in signals]
    lufs, lra, dbtp = None, None, None
    if args.loudness_range:
        lra = measure_loudness_range(signals, args.sr, args.batch_files, scorer)
    if args.true_peak:
        dbtp = measure_true_peak(signals, args.sr, args.batch_files, scorer)
    if args.loudness or args.match_loudness:
        lufs = measure_loudness(signals, args.sr, args.batch_files, scorer)
        if args.match_loudness:
            signals = match_signals(signals, lufs, names=names)
    values = score(signals, args.sr, args.batch_files, scorer, names=names, estoi=args.estoi, spectral=args.spectral, ssnr=args.ssnr)
    columns = metric_columns(args.estoi, args.spectral, args.ssnr)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if lag_q is not None:
        pols = sign if args.align_polarity else None
        write_csv(args.out, kept, values, columns=columns, lag_q=lag_q, Q=args.align_q, pols=pols, lufs=lufs, lra=lra, dbtp=dbtp)
        res.lags = lag_summary_frac(lag_q, args.align_q)
        res.inverted = [(name, int(np.count_nonzero(sign[:, k] < 0))) for k, name in enumerate(POL_NAMES)] if pols is not None else []
    elif lags is None:
        write_csv(args.out, kept, values, columns=columns, lufs=lufs, lra=lra, dbtp=dbtp)
    else:
        write_csv(args.out, kept, values, columns=columns, lags=lags, lufs=lufs, lra=lra, dbtp=dbtp)
        res.lags = lag_summary(lags)
    res.n_scored, res.means = len(kept), summary(values, columns=columns)
    res.loudness = summary(lufs, columns=LUFS_NAMES) if lufs is not None else []
    res.loudness_range = summary(lra, columns=LRA_NAMES) if lra is not None else []
    res.true_peak = summary(dbtp, columns=DBTP_NAMES) if dbtp is not None else []
    print(f"eval: {res.n_triples} triples, {res.n_scored} rows in {args.out}, {res.n_unreadable} skipped (unreadable)")
    for name, mean, count in res.means:
        print(f"  {name:12s} mean = {mean:.6g}  over {count} finite rows")
    for name, mean, count in res.loudness + res.loudness_range + res.true_peak:
        print(f"  {name:12s} mean = {mean:.6g}  over {count} finite rows")
    for name, lo, hi, nonzero in res.lags:
        print(f"  {name:12s} min = {lo}  max = {hi}  non-zero in {nonzero} of {res.n_scored} rows")
    for name, count in res.inverted:
        print(f"  {name:12s} inverted in {count} of {res.n_scored} rows")
    return res


def cli(argv=None) -> int:
    return run(argv).exit_code


if __name__ == "__main__":
    sys.exit(cli())
